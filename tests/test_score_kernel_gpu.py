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
import itertools
import os
import sys

import numpy as np
import pytest

import simulgen_vae_amd  # noqa: F401
from simulgen_vae_amd import engine as E

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ew_reference as R  # noqa: E402
import recon_kernel_common as H  # noqa: E402
from recon_kernel_common import CANARY, DTYPES, ELT32, ICANARY, _groups, bits  # noqa: E402

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
SHAPES = [(1, 1, 8, 8), (3, 5, 40, 40), (2, 33, 72, 72), (2, 10, 72, 80), (2, 200, 2080, 2080)]     # (B, T, C, ldy)
OUTPUTS = ("node_err", "node_when", "frame_err", "frame_where")
BLOCK_CHANNELS = 512          # 8 channels x 64 column lanes
PASS = H.Pass("score", lambda b, T, Cn: dict(truth=(b, T, Cn), node_err=(b, 3, Cn), node_when=(b, Cn), frame_err=(b, T, 3), frame_where=(b, T)), OUTPUTS,
              lambda a: (a["truth"], H.struct(E.ScoreOut, a, OUTPUTS)), integer=("node_when", "frame_where"))


def variant(kind):
    """an edit of the inputs of tests/test_summary_kernel_gpu.py: "rows": every row a copy of row 0; (n1, n2): node n2 a copy of node
    n1 (column of y, gamma, beta, scale, min), dominant in |e|"""
    def edit(c):
        y, gamma, beta, scale, mn = (c[k] for k in ("y", "gamma", "beta", "scale", "mn"))
        if kind == "rows":
            y[:] = y[:, :1]
        else:
            n1, n2 = kind
            scale[n1], mn[n1] = 1e-8, 0.0          # |val| up to 1e8 at the pair and |e| about a tenth of that; elsewhere |e| stays below 1e5
            y[:, :, n2] = y[:, :, n1]
            for a in (gamma, beta, scale, mn):
                a[n2] = a[n1]
    return edit


def reference(dtype, kind=None):
    """-> what to add to the inputs c: the float64 reference `ref`, its element bound `tol` and `truth` (fp32), which follows the
    variant's copies of rows or of a node"""
    def extras(c):
        B, T, Cn = c["y"].shape
        xhat = R.gn_forward(c["y"], _groups(Cn), c["gamma"], c["beta"], 2)["out"]
        mn64, sc64 = c["mn"].astype(np.float64), c["scale"].astype(np.float64)
        ref = (xhat - mn64) / sc64
        g = np.random.default_rng(77 + 1000 * Cn + 10 * T + B + dtype)
        g1, g2 = g.standard_normal((B, T, Cn)), g.standard_normal((B, T, Cn))
        if kind == "rows":
            g1[:], g2[:] = g1[:, :1], g2[:, :1]
        elif kind is not None:
            n1, n2 = kind
            g1[:, :, n2], g2[:, :, n2] = g1[:, :, n1], g2[:, :, n1]
        return {"ref": ref, "tol": (ELT32 * np.abs(xhat).max() + 4 * U * (np.abs(xhat) + np.abs(mn64))) / np.abs(sc64),
                "truth": (ref.astype(np.float32).astype(np.float64) * (1 + 0.1 * g1) + 0.05 * g2 / np.abs(sc64)).astype(np.float32)}
    return extras


def make_inputs(B, T, Cn, dtype, kind):
    c = H.inputs(B, T, Cn, dtype, variant(kind))
    c.update(reference(dtype, kind)(c))
    return c


def case(B, T, Cn, ldy, dtype):
    """inputs, the stored field F, truth and the float64 reference of one (shape, dtype), computed once and left alone"""
    c = H.case(__name__, B, T, Cn, ldy, dtype, extras=reference(dtype))
    assert (c["scale"] < 0).any() or Cn == 8
    return c


def score(c, ldy, dtype, which=OUTPUTS, truth=None):
    """one call of the hook on all of c["y"] -> dict of the outputs in `which`, in their documented shapes"""
    res = H.launch(PASS, c, c["y"], ldy, dtype, {"truth": c["truth"] if truth is None else truth}, want=which)
    return {k: res[k] for k in which}


_RUNS = {}


def run_once(B, T, Cn, ldy, dtype):
    key = (B, T, Cn, ldy, dtype)
    if key not in _RUNS:
        c = case(B, T, Cn, ldy, dtype)
        _RUNS[key] = (score(c, ldy, dtype), c["F"])
    return _RUNS[key]


def sum_bound(abs_terms, axis, m):
    """of a mean: the fp32 sum of m-term groups in any order, the squares' rounding and the division, over the count"""
    return (m - 1 + 2) * U * abs_terms.sum(axis=axis) / abs_terms.shape[axis]


def assert_exact(got, E32):
    """maxima and indices against numpy reductions of E = F - truth (float32), bit for bit"""
    A = np.abs(E32)
    assert np.array_equal(bits(got["node_err"][:, 0]), bits(A.max(axis=1))) and np.array_equal(got["node_when"], A.argmax(axis=1))
    assert np.array_equal(bits(got["frame_err"][:, :, 0]), bits(A.max(axis=2))) and np.array_equal(got["frame_where"], A.argmax(axis=2))


@DTYPES
@pytest.mark.parametrize("B,T,Cn,ldy", SHAPES)
def test_score_equals_reductions_of_the_stored_field_minus_truth(B, T, Cn, ldy, dtype):
    got, F = run_once(B, T, Cn, ldy, dtype)
    truth = case(B, T, Cn, ldy, dtype)["truth"]
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


@DTYPES
@pytest.mark.parametrize("B,T,Cn,ldy", SHAPES)
def test_score_matches_float64(B, T, Cn, ldy, dtype):
    got, _ = run_once(B, T, Cn, ldy, dtype)
    c = case(B, T, Cn, ldy, dtype)
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


@DTYPES
@pytest.mark.parametrize("B,T,Cn,ldy", SHAPES)
def test_truth_equal_to_the_stored_field_scores_exactly_zero(B, T, Cn, ldy, dtype):
    _, F = run_once(B, T, Cn, ldy, dtype)
    got = score(case(B, T, Cn, ldy, dtype), ldy, dtype, truth=F)
    assert not bits(got["node_err"]).any(), "a node maximum, bias or mean square is not +0.0"
    assert not bits(got["frame_err"][:, :, :2]).any(), "a frame maximum or mean square is not +0.0"
    assert not got["node_when"].any() and not got["frame_where"].any()
    t64 = F.astype(np.float64)
    assert np.all(np.abs(got["frame_err"][:, :, 2] - (t64 ** 2).mean(axis=2)) <= sum_bound(t64 ** 2, 2, min(Cn, BLOCK_CHANNELS)))


@DTYPES
@pytest.mark.parametrize("B,T,Cn,ldy", [SHAPES[2], SHAPES[4]])
def test_identical_rows_tie_at_the_first(B, T, Cn, ldy, dtype):
    c = make_inputs(B, T, Cn, dtype, "rows")
    got = score(c, ldy, dtype, ("node_err", "node_when"))
    assert (got["node_when"] == 0).all()


@DTYPES
@pytest.mark.parametrize("B,T,Cn,ldy,pair", [SHAPES[2] + ((0, 8),), SHAPES[4] + ((511, 512),)])
def test_identical_nodes_tie_at_the_smaller(B, T, Cn, ldy, pair, dtype):
    """(0, 8): neighbouring threads of one block; (511, 512): the last thread of column block 0 and the first of block 1, so the
    tie is settled by the frame finalize.  Both pairs lie in one group (Cg = 9 and 260)."""
    n1, n2 = pair
    Cg = Cn // _groups(Cn)
    assert n1 // Cg == n2 // Cg and n1 // 8 != n2 // 8 and (Cn < 2080 or n1 // BLOCK_CHANNELS != n2 // BLOCK_CHANNELS)
    c = make_inputs(B, T, Cn, dtype, pair)
    got = score(c, ldy, dtype)
    E32 = H.field(c, c["y"], ldy, dtype) - c["truth"]
    assert np.array_equal(bits(E32[:, :, n1]), bits(E32[:, :, n2]))
    assert_exact(got, E32)
    at_max = np.abs(E32[:, :, n1]) == np.abs(E32).max(axis=2)
    assert at_max.mean() > 0.9, "the pair does not dominate the frames"
    assert (got["frame_where"][at_max] == n1).all()


@DTYPES
@pytest.mark.parametrize("B,T,Cn,ldy", SHAPES)
def test_two_launches_are_bitwise_equal(B, T, Cn, ldy, dtype):
    got, _ = run_once(B, T, Cn, ldy, dtype)
    assert not H.same(score(case(B, T, Cn, ldy, dtype), ldy, dtype), got)          # margins, padding and truth are checked inside


def test_every_proper_subset_of_the_outputs():
    """any subset of the outputs may be asked for; what is computed does not depend on the others"""
    B, T, Cn, ldy = SHAPES[2]
    full, _ = run_once(B, T, Cn, ldy, 1)
    for k in (1, 2, 3):
        for which in itertools.combinations(OUTPUTS, k):
            got = score(case(B, T, Cn, ldy, 1), ldy, 1, which)
            assert set(got) == set(which)
            for name in which:
                assert np.array_equal(got[name].view(np.int32), full[name].view(np.int32)), (which, name)


def test_argument_errors_launch_nothing():
    import torch
    B, T, Cn = 2, 3, 16
    c = H.inputs(B, T, Cn, 0)
    d = H.device_inputs(c, c["y"], Cn, 0)
    bufs = H.canary_buffers(H.sizes(PASS, B, T, Cn), integer=PASS.integer)
    bufs["truth"][1].fill_(1.0)
    good = H.hook_args(d, bufs, Cn, 0, B, T, Cn)
    bad = H.common_rejections(good)          # among them C = 12 under ldy = 16 and ldy = C - 8
    bad += [(dict(truth=None), "null argument"), (dict(no_struct=True), "null argument"), ({k: None for k in OUTPUTS}, "all four outputs are NULL")]
    bad += [({name: good[name] + step}, "misaligned pointer") for name, step in (("node_err", 4), ("node_when", 8), ("frame_err", 2), ("frame_where", 1))]
    bad += [(dict(y=good["y"] + 8), "misaligned pointer"), (dict(truth=good["truth"] + 4), "misaligned pointer")]
    H.reject_all(PASS, d, bufs, good, bad)
    for name in OUTPUTS:
        view = bufs[name][1]
        assert not bool((view == (ICANARY if view.dtype == torch.int32 else CANARY)).any()), name
    # frame outputs need 4-byte alignment only
    assert H.call(PASS, dict(good, frame_err=good["frame_err"] + 4, frame_where=good["frame_where"] + 4)) == 0
    assert H.margins_intact({k: v for k, v in bufs.items() if k.startswith("node")})
