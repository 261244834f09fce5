"""The error pass of surrogate scoring alone (csrc/recon_out.hip: recon_score_kernel, recon_frames_kernel; include/sgvae.h:
sgv_test_recon_score): reductions of  e[b, t, n] = val[b, t, n] - truth[b, t, n],  val = (tanh(GroupNorm(y)) - min_n) / scale_n,
that store neither val nor e.  Inputs as tests/test_summary_kernel_gpu.py builds them (a quarter of the scales negative); truth is
the float64 reference rounded to fp32 and perturbed, ref * (1 + 0.1 g1) + 0.05 g2 / |scale_n|, so that the errors are neither zero
nor dominated by cancellation.

u = 2^-24.  The summation bound of an fp32 sum of m terms in any order: (m - 1) u sum|terms|, plus 2 u sum|terms| for the rounding
of each square (absent under a fused multiply-add) and the one division; m = T for the node sums, m = the channels of one column
block (at most 512) for the frame sums, whose block partials are combined in fp64.

Two references.
  * The existing output pass (sgv_test_recon_physical, layout [B][T][N]) on the same inputs, F, and E = F - truth in numpy float32
    (exact IEEE, as the kernel's one subtraction): max |E| over t and over n and their np.argmax (first occurrence) bit for bit;
    bias, the mean squares and the mean of truth^2 against float64 sums of E, E^2, truth^2 within the summation bound.
  * float64 end to end: tests/ew_reference.gn_forward + a float64 descale, the element bound tol of
    tests/test_generate_kernel_gpu.py widened by the subtraction,  te = tol + u |e_ref|.  A maximum is within the largest te over
    the reduced axis; an index i is accepted iff | |e_ref[i]| - |e_ref[j]| | <= te[i] + te[j], j the reference's own argmax; the
    bias within mean(te) + the summation bound; a mean square within mean(2 |e_ref| te + te^2) + the summation bound (the terms
    of the summation bound taken as |e_ref| + te).  Derived, not fitted.
Measured on an MI355X over all cases, worst err / bound per output -- against F: bias 0.26, node mse 0.45, frame mse 0.07, frame
truth^2 0.13 (maxima and indices exact); against float64: node max 0.27, frame max 0.27, bias 0.12, node mse 0.12, frame mse 0.09
(DESIGN.md section 18).

Shapes: the five of tests/test_generate_kernel_gpu.py; 2080 channels are five column blocks, so the frame finalize combines
partials, and 200 rows keep every row lane busy; (2, 10, 72, 80) has padding columns: they hold a canary and must come back
unchanged."""
import ctypes as C
import itertools
import os
import sys

import numpy as np
import pytest

import simulgen_vae_amd  # noqa: F401
from simulgen_vae_amd import engine as E

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ew_reference as R  # noqa: E402
from recon_kernel_common import (CANARY, ELT32, ICANARY, _bf16, _groups, base_inputs, bits, canary_buffers, device_inputs, field, hook_inputs,  # noqa: E402
                                 margins_intact, padding_intact)

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
SHAPES = [(1, 1, 8, 8), (3, 5, 40, 40), (2, 33, 72, 72), (2, 10, 72, 80), (2, 200, 2080, 2080)]     # (B, T, C, ldy)
OUTPUTS = ("node_err", "node_when", "frame_err", "frame_where")
BLOCK_CHANNELS = 512          # 8 channels x 64 column lanes


def make_inputs(B, T, Cn, dtype, variant=None):
    """the inputs of tests/test_summary_kernel_gpu.py, with the truth.  variant "rows": every row a copy of row 0; variant (n1, n2):
    node n2 a copy of node n1 (column of y, gamma, beta, scale, min and truth), dominant in |e|.  Adds the float64 reference `ref`,
    its element bound `tol` and `truth` (fp32)."""
    import torch
    c = base_inputs(B, T, Cn, dtype)
    y, gamma, beta, scale, mn = (c[k] for k in ("y", "gamma", "beta", "scale", "mn"))
    if variant == "rows":
        y[:] = y[:, :1]
    elif variant is not None:
        n1, n2 = variant
        scale[n1], mn[n1] = 1e-8, 0.0          # |val| up to 1e8 at the pair and |e| about a tenth of that; elsewhere |e| stays below 1e5
        y[:, :, n2] = y[:, :, n1]
        for a in (gamma, beta, scale, mn):
            a[n2] = a[n1]
    if dtype == 1:
        y = _bf16(torch, y)
    c = dict(y=y, gamma=gamma, beta=beta, scale=scale, mn=mn)
    xhat = R.gn_forward(y, _groups(Cn), gamma, beta, 2)["out"]
    mn64, sc64 = mn.astype(np.float64), scale.astype(np.float64)
    c["ref"] = (xhat - mn64) / sc64
    c["tol"] = (ELT32 * np.abs(xhat).max() + 4 * U * (np.abs(xhat) + np.abs(mn64))) / np.abs(sc64)
    g = np.random.default_rng(77 + 1000 * Cn + 10 * T + B + dtype)
    g1, g2 = g.standard_normal((B, T, Cn)), g.standard_normal((B, T, Cn))
    if variant == "rows":
        g1[:], g2[:] = g1[:, :1], g2[:, :1]
    elif variant is not None:
        g1[:, :, n2], g2[:, :, n2] = g1[:, :, n1], g2[:, :, n1]
    c["truth"] = (c["ref"].astype(np.float32).astype(np.float64) * (1 + 0.1 * g1) + 0.05 * g2 / np.abs(sc64)).astype(np.float32)
    return c


_CASES = {}


def case(B, T, Cn, dtype):
    """inputs, truth and the float64 reference of one (shape, dtype), computed once and left alone"""
    key = (B, T, Cn, dtype)
    if key not in _CASES:
        _CASES[key] = make_inputs(B, T, Cn, dtype)
        assert (_CASES[key]["scale"] < 0).any() or Cn == 8
    return _CASES[key]


def out_buffers(B, T, Cn, which=OUTPUTS):
    """name -> (whole buffer with canary margins, the output's view)"""
    sizes = dict(node_err=B * 3 * Cn, node_when=B * Cn, frame_err=B * T * 3, frame_where=B * T)
    return canary_buffers({name: sizes[name] for name in which}, integer=("node_when", "frame_where"))


def score(c, B, T, Cn, ldy, dtype, which=OUTPUTS, truth=None):
    """one call of the hook -> (dict of numpy outputs in their documented shapes, dict of the raw buffers)"""
    import torch
    lib = E.load_library()
    d = device_inputs(c, c["y"], ldy, dtype)
    tr = torch.from_numpy(np.ascontiguousarray(c["truth"] if truth is None else truth, np.float32)).cuda()
    keep = tr.clone()
    bufs = out_buffers(B, T, Cn, which)
    for _, view in bufs.values():
        view.fill_(float("nan") if view.dtype == torch.float32 else -1)
    so = E.ScoreOut(**{name: view.data_ptr() for name, (_, view) in bufs.items()})
    rc = lib.sgv_test_recon_score(dtype, *hook_inputs(d, ldy), tr.data_ptr(), C.byref(so), B, T, Cn, None)
    assert rc == 0, lib.sgv_last_error().decode()
    assert margins_intact(bufs), "a margin around an output was written"
    assert padding_intact(d, Cn), "the padding columns of y were written"
    assert bool((tr.view(torch.int32) == keep.view(torch.int32)).all()), "the truth was written"
    shapes = dict(node_err=(B, 3, Cn), node_when=(B, Cn), frame_err=(B, T, 3), frame_where=(B, T))
    return {n: v.cpu().numpy().reshape(shapes[n]) for n, (_, v) in bufs.items()}, {n: b.clone() for n, (b, _) in bufs.items()}


_RUNS = {}


def run_once(B, T, Cn, ldy, dtype):
    key = (B, T, Cn, ldy, dtype)
    if key not in _RUNS:
        c = case(B, T, Cn, dtype)
        got, raw = score(c, B, T, Cn, ldy, dtype)
        _RUNS[key] = (got, raw, field(c, c["y"], ldy, dtype))
    return _RUNS[key]


def sum_bound(abs_terms, axis, m):
    """of a mean: the fp32 sum of m-term groups in any order, the squares' rounding and the division, over the count"""
    return (m - 1 + 2) * U * abs_terms.sum(axis=axis) / abs_terms.shape[axis]


def assert_exact(got, E32):
    """maxima and indices against numpy reductions of E = F - truth (float32), bit for bit"""
    A = np.abs(E32)
    assert np.array_equal(bits(got["node_err"][:, 0]), bits(A.max(axis=1))) and np.array_equal(got["node_when"], A.argmax(axis=1))
    assert np.array_equal(bits(got["frame_err"][:, :, 0]), bits(A.max(axis=2))) and np.array_equal(got["frame_where"], A.argmax(axis=2))


@pytest.mark.parametrize("dtype", [0, 1], ids=["f32", "bf16"])
@pytest.mark.parametrize("B,T,Cn,ldy", SHAPES)
def test_score_equals_reductions_of_the_stored_field_minus_truth(B, T, Cn, ldy, dtype):
    got, _, F = run_once(B, T, Cn, ldy, dtype)
    truth = case(B, T, Cn, dtype)["truth"]
    assert np.isfinite(F).all()
    E32 = F - truth
    assert E32.dtype == np.float32
    assert_exact(got, E32)
    E64, t64 = E32.astype(np.float64), truth.astype(np.float64)
    mf = min(Cn, BLOCK_CHANNELS)
    checks = {
        "node bias": (np.abs(got["node_err"][:, 1] - E64.mean(axis=1)), sum_bound(np.abs(E64), 1, T)),
        "node mse": (np.abs(got["node_err"][:, 2] - (E64 ** 2).mean(axis=1)), sum_bound(E64 ** 2, 1, T)),
        "frame mse": (np.abs(got["frame_err"][:, :, 1] - (E64 ** 2).mean(axis=2)), sum_bound(E64 ** 2, 2, mf)),
        "frame truth^2": (np.abs(got["frame_err"][:, :, 2] - (t64 ** 2).mean(axis=2)), sum_bound(t64 ** 2, 2, mf)),
    }
    worst = {k: float(np.max(e / b)) for k, (e, b) in checks.items()}
    print(f"  vs F (B, T, C, ldy) = {(B, T, Cn, ldy)} dtype {dtype}: worst err/bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    for k, (e, b) in checks.items():
        assert np.all(e <= b), f"{k}: {int((e > b).sum())} off, worst err/bound {worst[k]:.3f}"


def _index_ok(a_ref, te, idx, axis):
    j = a_ref.argmax(axis=axis)
    pick = lambda a, i: np.take_along_axis(a, np.expand_dims(i, axis), axis).squeeze(axis)
    return np.abs(pick(a_ref, idx) - pick(a_ref, j)) <= pick(te, idx) + pick(te, j)


@pytest.mark.parametrize("dtype", [0, 1], ids=["f32", "bf16"])
@pytest.mark.parametrize("B,T,Cn,ldy", SHAPES)
def test_score_matches_float64(B, T, Cn, ldy, dtype):
    got, _, _ = run_once(B, T, Cn, ldy, dtype)
    c = case(B, T, Cn, dtype)
    e = c["ref"] - c["truth"].astype(np.float64)
    a = np.abs(e)
    te = c["tol"] + U * a
    for name in ("node_err", "frame_err"):
        assert np.isfinite(got[name]).all(), f"an element of {name} was not written"
    sq_el, up = 2 * a * te + te ** 2, a + te          # the elements' share of a square's error; an upper bound of the kernel's |e|
    mf = min(Cn, BLOCK_CHANNELS)
    checks = {
        "node max": (np.abs(got["node_err"][:, 0] - a.max(axis=1)), te.max(axis=1)),
        "frame max": (np.abs(got["frame_err"][:, :, 0] - a.max(axis=2)), te.max(axis=2)),
        "node bias": (np.abs(got["node_err"][:, 1] - e.mean(axis=1)), te.mean(axis=1) + sum_bound(up, 1, T)),
        "node mse": (np.abs(got["node_err"][:, 2] - (e ** 2).mean(axis=1)), sq_el.mean(axis=1) + sum_bound(up ** 2, 1, T)),
        "frame mse": (np.abs(got["frame_err"][:, :, 1] - (e ** 2).mean(axis=2)), sq_el.mean(axis=2) + sum_bound(up ** 2, 2, mf)),
    }
    worst = {k: float(np.max(err / b)) for k, (err, b) in checks.items()}
    print(f"  vs float64 (B, T, C, ldy) = {(B, T, Cn, ldy)} dtype {dtype}: worst err/bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    for k, (err, b) in checks.items():
        assert np.all(err <= b), f"{k}: {int((err > b).sum())} off, worst err/bound {worst[k]:.3f}"
    assert _index_ok(a, te, got["node_when"], 1).all() and _index_ok(a, te, got["frame_where"], 2).all()
    assert (got["node_when"] >= 0).all() and (got["node_when"] < T).all() and (got["frame_where"] >= 0).all() and (got["frame_where"] < Cn).all()


@pytest.mark.parametrize("dtype", [0, 1], ids=["f32", "bf16"])
@pytest.mark.parametrize("B,T,Cn,ldy", SHAPES)
def test_truth_equal_to_the_stored_field_scores_exactly_zero(B, T, Cn, ldy, dtype):
    _, _, F = run_once(B, T, Cn, ldy, dtype)
    got, _ = score(case(B, T, Cn, dtype), B, T, Cn, ldy, dtype, truth=F)
    assert not bits(got["node_err"]).any(), "a node maximum, bias or mean square is not +0.0"
    assert not bits(got["frame_err"][:, :, :2]).any(), "a frame maximum or mean square is not +0.0"
    assert not got["node_when"].any() and not got["frame_where"].any()
    t64 = F.astype(np.float64)
    assert np.all(np.abs(got["frame_err"][:, :, 2] - (t64 ** 2).mean(axis=2)) <= sum_bound(t64 ** 2, 2, min(Cn, BLOCK_CHANNELS)))


@pytest.mark.parametrize("dtype", [0, 1], ids=["f32", "bf16"])
@pytest.mark.parametrize("B,T,Cn,ldy", [SHAPES[2], SHAPES[4]])
def test_identical_rows_tie_at_the_first(B, T, Cn, ldy, dtype):
    c = make_inputs(B, T, Cn, dtype, "rows")
    got, _ = score(c, B, T, Cn, ldy, dtype, ("node_err", "node_when"))
    assert (got["node_when"] == 0).all()


@pytest.mark.parametrize("dtype", [0, 1], ids=["f32", "bf16"])
@pytest.mark.parametrize("B,T,Cn,ldy,pair", [SHAPES[2] + ((0, 8),), SHAPES[4] + ((511, 512),)])
def test_identical_nodes_tie_at_the_smaller(B, T, Cn, ldy, pair, dtype):
    """(0, 8): neighbouring threads of one block; (511, 512): the last thread of column block 0 and the first of block 1, so the
    tie is settled by the frame finalize.  Both pairs lie in one group (Cg = 9 and 260)."""
    n1, n2 = pair
    Cg = Cn // _groups(Cn)
    assert n1 // Cg == n2 // Cg and n1 // 8 != n2 // 8 and (Cn < 2080 or n1 // BLOCK_CHANNELS != n2 // BLOCK_CHANNELS)
    c = make_inputs(B, T, Cn, dtype, pair)
    got, _ = score(c, B, T, Cn, ldy, dtype)
    E32 = field(c, c["y"], ldy, dtype) - c["truth"]
    assert np.array_equal(bits(E32[:, :, n1]), bits(E32[:, :, n2]))
    assert_exact(got, E32)
    at_max = np.abs(E32[:, :, n1]) == np.abs(E32).max(axis=2)
    assert at_max.mean() > 0.9, "the pair does not dominate the frames"
    assert (got["frame_where"][at_max] == n1).all()


@pytest.mark.parametrize("dtype", [0, 1], ids=["f32", "bf16"])
@pytest.mark.parametrize("B,T,Cn,ldy", SHAPES)
def test_two_launches_are_bitwise_equal(B, T, Cn, ldy, dtype):
    import torch
    _, raw, _ = run_once(B, T, Cn, ldy, dtype)
    _, raw2 = score(case(B, T, Cn, dtype), B, T, Cn, ldy, dtype)          # margins, padding and truth are checked inside
    for name in OUTPUTS:
        assert bool((raw[name].view(torch.int32) == raw2[name].view(torch.int32)).all()), f"{name}: two launches differ"


def test_every_proper_subset_of_the_outputs():
    """any subset of the outputs may be asked for; what is computed does not depend on the others"""
    B, T, Cn, ldy = SHAPES[2]
    full, _, _ = run_once(B, T, Cn, ldy, 1)
    for k in (1, 2, 3):
        for which in itertools.combinations(OUTPUTS, k):
            got, _ = score(case(B, T, Cn, 1), B, T, Cn, ldy, 1, which)
            assert set(got) == set(which)
            for name in which:
                assert np.array_equal(got[name].view(np.int32), full[name].view(np.int32)), (which, name)


def test_argument_errors_launch_nothing():
    import torch
    lib = E.load_library()
    B, T, Cn = 2, 3, 16
    y = torch.zeros((B * T, Cn), dtype=torch.float32, device="cuda")
    v = torch.ones(Cn, dtype=torch.float32, device="cuda")
    tr = torch.ones(B * T * Cn + 4, dtype=torch.float32, device="cuda")
    sums = torch.zeros(B * 4 * 2, dtype=torch.float64, device="cuda")
    bufs = out_buffers(B, T, Cn)
    for _, view in bufs.values():
        view.fill_(ICANARY if view.dtype == torch.int32 else CANARY)
    good = dict(y=y.data_ptr(), sums=sums.data_ptr(), gamma=v.data_ptr(), beta=v.data_ptr(), scale=v.data_ptr(), mn=v.data_ptr(), truth=tr.data_ptr())
    outs = {name: view.data_ptr() for name, (_, view) in bufs.items()}

    def call(out=outs, Cn=Cn, ldy=Cn, **kw):
        a = dict(good, **kw)
        so = None if out is None else C.byref(E.ScoreOut(**out))
        return lib.sgv_test_recon_score(0, a["y"], ldy, a["sums"], a["gamma"], a["beta"], a["scale"], a["mn"], a["truth"], so, B, T, Cn, None)

    def rejected(msg, **kw):
        assert call(**kw) == -1, kw          # SGV_ERR_ARG
        assert msg in lib.sgv_last_error().decode(), lib.sgv_last_error().decode()

    for name in good:
        rejected("null argument", **{name: None})
    rejected("null argument", out=None)
    rejected("all four outputs are NULL", out={})
    rejected("C % 8 == 0 required", Cn=12, ldy=16)
    rejected("C % 8 == 0 required", Cn=0)
    rejected("row stride", ldy=Cn - 8)
    for name, step in (("node_err", 4), ("node_when", 8), ("frame_err", 2), ("frame_where", 1)):
        rejected("misaligned pointer", out=dict(outs, **{name: outs[name] + step}))
    rejected("misaligned pointer", y=good["y"] + 8)
    rejected("misaligned pointer", truth=good["truth"] + 4)
    torch.cuda.synchronize()
    for name, (buf, _) in bufs.items():
        assert bool((buf == buf[0]).all()), f"a rejected call wrote {name}"
    assert call() == 0
    for name, (_, view) in bufs.items():
        assert not bool((view == (ICANARY if view.dtype == torch.int32 else CANARY)).any()), name
    # frame outputs need 4-byte alignment only
    odd = dict(outs, frame_err=outs["frame_err"] + 4, frame_where=outs["frame_where"] + 4)
    assert call(out=odd) == 0
    assert margins_intact({k: v for k, v in bufs.items() if k.startswith("node")})
