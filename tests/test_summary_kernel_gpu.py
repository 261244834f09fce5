"""The summary pass of the surrogate sweep alone (csrc/recon_out.hip: recon_summary_*, recon_probe_kernel; include/sgvae.h:
sgv_test_recon_summary): reductions of  val[b, t, n] = (tanh(GroupNorm(y)[b, t, n]) - min_n) / scale_n  that never store val.

Two references.
  * The existing output pass (sgv_test_recon_physical, layout [B][T][N]) on the same inputs, F.  The summary kernels form val with
    the same device function, so extrema, their indices and the probes are the numpy reductions / gather of F bit for bit
    (np.argmax / np.argmin return the first occurrence: the smallest index wins a tie).
  * float64: tests/ew_reference.gn_forward + a float64 descale, with the element bound of tests/test_generate_kernel_gpu.py,
        tol[b, t, n] = (ELT32 * max|x_hat_ref| + 4 * 2^-24 * (|x_hat_ref| + |min_n|)) / |scale_n|.
    An extremum is within the largest tol over the reduced axis; a probe within tol.
    An index i is accepted iff  |ref[i] - ref[j]| <= tol[i] + tol[j],  j the reference's own arg-extremum: the kernel picked i
    because val[i] >= val[j], and val is within tol of ref at both places, so ref[i] >= ref[j] - tol[i] - tol[j] (at most twice the
    largest tol; the reference's own index passes by construction).
    The mean is within  mean_t(tol) + (T + 2) * 2^-24 * max_t|ref|:  the elements' own error, plus the worst case of an fp32 sum of
    T terms in any order (T - 1 additions, each rounding a partial sum of at most T max|val|: (T - 1) 2^-24 max|val| relative to
    the mean after the division) plus the division and one to spare.  Derived, not fitted.
Measured on an MI355X over all cases: worst err / bound 0.27 (frame min, bf16, (2, 200, 2080)); node extrema <= 0.25, probes <= 0.21,
the mean <= 0.11.

About a quarter of scale_n is negative (scaler_vectors admits that): a kernel that reduced x_hat and descaled afterwards would swap
max and min there.  Shapes: the five of tests/test_generate_kernel_gpu.py; 2080 channels are five column blocks of the summary
kernel, so the frame finalize combines partials; (2, 10, 72, 80) has padding columns: they hold a canary, must come back unchanged, and
no frame index may point at them."""
import ctypes as C
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

SHAPES = [(1, 1, 8, 8), (3, 5, 40, 40), (2, 33, 72, 72), (2, 10, 72, 80), (2, 200, 2080, 2080)]     # (B, T, C, ldy)
OUTPUTS = ("node_stats", "node_when", "frame_stats", "frame_where", "probes")


def probe_list(Cn, K):
    return np.array([Cn // 2] if K == 1 else [0, Cn - 1, Cn // 3, Cn // 3, min(5, Cn - 2)], np.int32)


def make_inputs(B, T, Cn, dtype, variant=None):
    """the inputs of tests/test_generate_kernel_gpu.py with a quarter of the scales negative; variant "rows": every row a copy of
    row 0; variant (n1, n2): node n2 a copy of node n1 (column of y, gamma, beta, scale, min), dominant in magnitude"""
    import torch
    c = base_inputs(B, T, Cn, dtype)
    y, gamma, beta, scale, mn = (c[k] for k in ("y", "gamma", "beta", "scale", "mn"))
    if variant == "rows":
        y[:] = y[:, :1]
    elif variant is not None:
        n1, n2 = variant
        scale[n1], mn[n1] = 1e-6, 0.0          # |val| up to 1e6 at the pair: the frame maximum where tanh > 0, the minimum where < 0
        y[:, :, n2] = y[:, :, n1]
        for a in (gamma, beta, scale, mn):
            a[n2] = a[n1]
    if dtype == 1:
        y = _bf16(torch, y)
    return dict(y=y, gamma=gamma, beta=beta, scale=scale, mn=mn)


_CASES = {}


def case(B, T, Cn, dtype):
    """inputs and the float64 reference of one (shape, dtype), computed once and left alone"""
    key = (B, T, Cn, dtype)
    if key not in _CASES:
        c = make_inputs(B, T, Cn, dtype)
        xhat = R.gn_forward(c["y"], _groups(Cn), c["gamma"], c["beta"], 2)["out"]
        mn64, sc64 = c["mn"].astype(np.float64), c["scale"].astype(np.float64)
        c["ref"] = (xhat - mn64) / sc64
        c["tol"] = (ELT32 * np.abs(xhat).max() + 4 * 2.0 ** -24 * (np.abs(xhat) + np.abs(mn64))) / np.abs(sc64)
        assert (c["scale"] < 0).any() or Cn == 8
        _CASES[key] = c
    return _CASES[key]


def out_buffers(B, T, Cn, K, which=OUTPUTS):
    """name -> (whole buffer with canary margins, the output's view)"""
    sizes = dict(node_stats=B * 3 * Cn, node_when=B * 2 * Cn, frame_stats=B * T * 2, frame_where=B * T * 2, probes=B * T * K)
    return canary_buffers({name: sizes[name] for name in which}, integer=("node_when", "frame_where"))


def summary(c, B, T, Cn, ldy, dtype, K, which=OUTPUTS):
    """one call of the hook -> (dict of numpy outputs in their documented shapes, dict of the raw buffers)"""
    import torch
    lib = E.load_library()
    d = device_inputs(c, c["y"], ldy, dtype)
    bufs = out_buffers(B, T, Cn, K, which)
    for _, view in bufs.values():
        view.fill_(float("nan") if view.dtype == torch.float32 else -1)
    so = E.SummaryOut(**{name: view.data_ptr() for name, (_, view) in bufs.items()})
    nodes = probe_list(Cn, K)
    rc = lib.sgv_test_recon_summary(dtype, *hook_inputs(d, ldy), C.byref(so), nodes.ctypes.data_as(C.c_void_p), K, B, T, Cn, None)
    assert rc == 0, lib.sgv_last_error().decode()
    assert margins_intact(bufs), "a margin around an output was written"
    assert padding_intact(d, Cn), "the padding columns of y were written"
    shapes = dict(node_stats=(B, 3, Cn), node_when=(B, 2, Cn), frame_stats=(B, T, 2), frame_where=(B, T, 2), probes=(B, T, K))
    return {n: v.cpu().numpy().reshape(shapes[n]) for n, (_, v) in bufs.items()}, {n: b.clone() for n, (b, _) in bufs.items()}


_RUNS = {}


def run_once(B, T, Cn, ldy, dtype, K):
    key = (B, T, Cn, ldy, dtype, K)
    if key not in _RUNS:
        c = case(B, T, Cn, dtype)
        got, raw = summary(c, B, T, Cn, ldy, dtype, K)
        if (B, T, Cn, ldy, dtype) not in _RUNS:
            _RUNS[(B, T, Cn, ldy, dtype)] = field(c, c["y"], ldy, dtype)
        _RUNS[key] = (got, raw, _RUNS[(B, T, Cn, ldy, dtype)])
    return _RUNS[key]


def assert_exact(got, F, nodes):
    """extrema, indices and probes against numpy reductions of the stored field F, bit for bit"""
    assert np.isfinite(F).all()
    assert np.array_equal(bits(got["node_stats"][:, 0]), bits(F.max(axis=1))) and np.array_equal(bits(got["node_stats"][:, 1]), bits(F.min(axis=1)))
    assert np.array_equal(got["node_when"][:, 0], F.argmax(axis=1)) and np.array_equal(got["node_when"][:, 1], F.argmin(axis=1))
    assert np.array_equal(bits(got["frame_stats"][:, :, 0]), bits(F.max(axis=2))) and np.array_equal(bits(got["frame_stats"][:, :, 1]), bits(F.min(axis=2)))
    assert np.array_equal(got["frame_where"][:, :, 0], F.argmax(axis=2)) and np.array_equal(got["frame_where"][:, :, 1], F.argmin(axis=2))
    if "probes" in got:
        assert np.array_equal(bits(got["probes"]), bits(F[:, :, nodes]))


def mean_bound(ref, tol):
    T = ref.shape[1]
    return tol.mean(axis=1) + (T + 2) * 2.0 ** -24 * np.abs(ref).max(axis=1)


@pytest.mark.parametrize("K", [1, 5])
@pytest.mark.parametrize("dtype", [0, 1], ids=["f32", "bf16"])
@pytest.mark.parametrize("B,T,Cn,ldy", SHAPES)
def test_summaries_equal_reductions_of_the_stored_field(B, T, Cn, ldy, dtype, K):
    got, _, F = run_once(B, T, Cn, ldy, dtype, K)
    assert_exact(got, F, probe_list(Cn, K))
    # the mean is a sum in another order than numpy's: against the float64 mean of F with the summation part of the bound
    err = np.abs(got["node_stats"][:, 2].astype(np.float64) - F.astype(np.float64).mean(axis=1))
    assert np.all(err <= (T + 2) * 2.0 ** -24 * np.abs(F).max(axis=1))


def _index_ok(ref, tol, idx, axis, largest):
    j = ref.argmax(axis=axis) if largest else ref.argmin(axis=axis)
    pick = lambda a, i: np.take_along_axis(a, np.expand_dims(i, axis), axis).squeeze(axis)
    return np.abs(pick(ref, idx) - pick(ref, j)) <= pick(tol, idx) + pick(tol, j)


@pytest.mark.parametrize("dtype", [0, 1], ids=["f32", "bf16"])
@pytest.mark.parametrize("B,T,Cn,ldy", SHAPES)
def test_summaries_match_float64(B, T, Cn, ldy, dtype):
    K = 5
    got, _, _ = run_once(B, T, Cn, ldy, dtype, K)
    c = case(B, T, Cn, dtype)
    ref, tol = c["ref"], c["tol"]
    for name in ("node_stats", "frame_stats", "probes"):
        assert np.isfinite(got[name]).all(), f"an element of {name} was not written"
    checks = {
        "node max": (np.abs(got["node_stats"][:, 0] - ref.max(axis=1)), tol.max(axis=1)),
        "node min": (np.abs(got["node_stats"][:, 1] - ref.min(axis=1)), tol.max(axis=1)),
        "node mean": (np.abs(got["node_stats"][:, 2] - ref.mean(axis=1)), mean_bound(ref, tol)),
        "frame max": (np.abs(got["frame_stats"][:, :, 0] - ref.max(axis=2)), tol.max(axis=2)),
        "frame min": (np.abs(got["frame_stats"][:, :, 1] - ref.min(axis=2)), tol.max(axis=2)),
        "probes": (np.abs(got["probes"] - ref[:, :, probe_list(Cn, K)]), tol[:, :, probe_list(Cn, K)]),
    }
    worst = {k: float(np.max(e / b)) for k, (e, b) in checks.items()}
    print(f"  (B, T, C, ldy) = {(B, T, Cn, ldy)} dtype {dtype}: worst err/bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    for k, (e, b) in checks.items():
        assert np.all(e <= b), f"{k}: {int((e > b).sum())} off, worst err/bound {worst[k]:.3f}"
    assert _index_ok(ref, tol, got["node_when"][:, 0], 1, True).all() and _index_ok(ref, tol, got["node_when"][:, 1], 1, False).all()
    assert _index_ok(ref, tol, got["frame_where"][:, :, 0], 2, True).all() and _index_ok(ref, tol, got["frame_where"][:, :, 1], 2, False).all()
    assert (got["node_when"] >= 0).all() and (got["node_when"] < T).all() and (got["frame_where"] >= 0).all() and (got["frame_where"] < Cn).all()


@pytest.mark.parametrize("dtype", [0, 1], ids=["f32", "bf16"])
@pytest.mark.parametrize("B,T,Cn,ldy", [SHAPES[2], SHAPES[4]])
def test_identical_rows_tie_at_the_first(B, T, Cn, ldy, dtype):
    c = make_inputs(B, T, Cn, dtype, "rows")
    got, _ = summary(c, B, T, Cn, ldy, dtype, 1, ("node_stats", "node_when"))
    assert (got["node_when"] == 0).all()
    assert np.array_equal(bits(got["node_stats"][:, 0]), bits(got["node_stats"][:, 1]))


@pytest.mark.parametrize("dtype", [0, 1], ids=["f32", "bf16"])
@pytest.mark.parametrize("B,T,Cn,ldy,pair", [SHAPES[2] + ((0, 8),), SHAPES[4] + ((500, 515),)])
def test_identical_nodes_tie_at_the_smaller(B, T, Cn, ldy, pair, dtype):
    """(0, 8): neighbouring threads of one block; (500, 515): the last and the first thread of neighbouring column blocks, so the
    tie is settled by the frame finalize.  Both pairs lie in one group (Cg = 9 and 260)."""
    n1, n2 = pair
    Cg = Cn // _groups(Cn)
    assert n1 // Cg == n2 // Cg and n2 - n1 >= 8
    c = make_inputs(B, T, Cn, dtype, pair)
    got, _ = summary(c, B, T, Cn, ldy, dtype, 1)
    F = field(c, c["y"], ldy, dtype)
    assert np.array_equal(bits(F[:, :, n1]), bits(F[:, :, n2]))
    assert_exact(got, F, probe_list(Cn, 1))
    at_max, at_min = F[:, :, n1] == F.max(axis=2), F[:, :, n1] == F.min(axis=2)
    assert at_max.any() and at_min.any(), "the pair never ties for a frame extremum"
    assert (got["frame_where"][:, :, 0][at_max] == n1).all() and (got["frame_where"][:, :, 1][at_min] == n1).all()


@pytest.mark.parametrize("dtype", [0, 1], ids=["f32", "bf16"])
@pytest.mark.parametrize("B,T,Cn,ldy", SHAPES)
def test_two_launches_are_bitwise_equal(B, T, Cn, ldy, dtype):
    import torch
    _, raw, _ = run_once(B, T, Cn, ldy, dtype, 5)
    _, raw2 = summary(case(B, T, Cn, dtype), B, T, Cn, ldy, dtype, 5)          # margins and padding are checked inside
    for name in OUTPUTS:
        assert bool((raw[name].view(torch.int32) == raw2[name].view(torch.int32)).all()), f"{name}: two launches differ"


def test_each_output_alone():
    """any subset of the outputs may be asked for; what is computed does not depend on the others"""
    B, T, Cn, ldy = SHAPES[2]
    full, _, _ = run_once(B, T, Cn, ldy, 1, 5)
    for name in OUTPUTS:
        got, _ = summary(case(B, T, Cn, 1), B, T, Cn, ldy, 1, 5, (name,))
        assert np.array_equal(got[name].view(np.int32), full[name].view(np.int32)), name


def test_argument_errors_launch_nothing():
    import torch
    lib = E.load_library()
    B, T, Cn, K = 2, 3, 16, 2
    y = torch.zeros((B * T, Cn), dtype=torch.float32, device="cuda")
    v = torch.ones(Cn, dtype=torch.float32, device="cuda")
    sums = torch.zeros(B * 4 * 2, dtype=torch.float64, device="cuda")
    bufs = out_buffers(B, T, Cn, K)
    for _, view in bufs.values():
        view.fill_(ICANARY if view.dtype == torch.int32 else CANARY)
    good = dict(y=y.data_ptr(), sums=sums.data_ptr(), gamma=v.data_ptr(), beta=v.data_ptr(), scale=v.data_ptr(), mn=v.data_ptr())
    outs = {name: view.data_ptr() for name, (_, view) in bufs.items()}
    nodes = np.array([3, 15], np.int32)

    def call(out=outs, probes=nodes, k=K, **kw):
        a = dict(good, **kw)
        so = None if out is None else C.byref(E.SummaryOut(**out))
        pp = None if probes is None else probes.ctypes.data_as(C.c_void_p)
        return lib.sgv_test_recon_summary(0, a["y"], Cn, a["sums"], a["gamma"], a["beta"], a["scale"], a["mn"], so, pp, k, B, T, Cn, None)

    def rejected(msg, **kw):
        assert call(**kw) == -1, kw
        assert msg in lib.sgv_last_error().decode(), lib.sgv_last_error().decode()

    for name in good:
        rejected("null argument", **{name: None})
    rejected("null argument", out=None)
    rejected("all five outputs are NULL", out={})
    rejected("no probe nodes are given", probes=None)
    rejected("no probe nodes are given", k=0)
    rejected("probe nodes[1] = 16 is outside [0, 16)", probes=np.array([3, 16], np.int32))
    rejected("probe nodes[0] = -1 is outside [0, 16)", probes=np.array([-1, 16], np.int32))
    for name, step in (("node_stats", 4), ("node_when", 8), ("frame_stats", 4), ("frame_where", 4), ("probes", 2)):
        rejected("misaligned pointer", out=dict(outs, **{name: outs[name] + step}))
    rejected("misaligned pointer", y=good["y"] + 8)
    torch.cuda.synchronize()
    for name, (buf, _) in bufs.items():
        assert bool((buf == buf[0]).all()), f"a rejected call wrote {name}"
    assert call() == 0
    for name, (_, view) in bufs.items():
        assert not bool((view == (ICANARY if view.dtype == torch.int32 else CANARY)).any()), name
    assert margins_intact(bufs)
