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
import recon_kernel_common as H  # noqa: E402
from recon_kernel_common import CANARY, DTYPES, ELT32, ICANARY, _groups, bits  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 8, 8), (3, 5, 40, 40), (2, 33, 72, 72), (2, 10, 72, 80), (2, 200, 2080, 2080)]     # (B, T, C, ldy)
OUTPUTS = ("node_stats", "node_when", "frame_stats", "frame_where", "probes")
PASS = H.Pass("summary", lambda b, T, Cn, nodes, n_probes: dict(node_stats=(b, 3, Cn), node_when=(b, 2, Cn), frame_stats=(b, T, 2), frame_where=(b, T, 2),
                                                               probes=(b, T, n_probes)), OUTPUTS,
              lambda a: (H.struct(E.SummaryOut, a, OUTPUTS), None if a["nodes"] is None else a["nodes"].ctypes.data_as(C.c_void_p), a["n_probes"]),
              integer=("node_when", "frame_where"))


def probe_list(Cn, K):
    return np.array([Cn // 2] if K == 1 else [0, Cn - 1, Cn // 3, Cn // 3, min(5, Cn - 2)], np.int32)


def variant(kind):
    """an edit of the inputs (a quarter of the scales negative): "rows": every row a copy of row 0; (n1, n2): node n2 a copy of node
    n1 (column of y, gamma, beta, scale, min), dominant in magnitude"""
    def edit(c):
        y, gamma, beta, scale, mn = (c[k] for k in ("y", "gamma", "beta", "scale", "mn"))
        if kind == "rows":
            y[:] = y[:, :1]
        else:
            n1, n2 = kind
            scale[n1], mn[n1] = 1e-6, 0.0          # |val| up to 1e6 at the pair: the frame maximum where tanh > 0, the minimum where < 0
            y[:, :, n2] = y[:, :, n1]
            for a in (gamma, beta, scale, mn):
                a[n2] = a[n1]
    return edit


def reference(c):
    Cn = c["y"].shape[2]
    xhat = R.gn_forward(c["y"], _groups(Cn), c["gamma"], c["beta"], 2)["out"]
    mn64, sc64 = c["mn"].astype(np.float64), c["scale"].astype(np.float64)
    return {"ref": (xhat - mn64) / sc64, "tol": (ELT32 * np.abs(xhat).max() + 4 * 2.0 ** -24 * (np.abs(xhat) + np.abs(mn64))) / np.abs(sc64)}


def case(B, T, Cn, ldy, dtype):
    """inputs, the stored field F and the float64 reference of one (shape, dtype), computed once and left alone"""
    c = H.case(__name__, B, T, Cn, ldy, dtype, extras=reference)
    assert (c["scale"] < 0).any() or Cn == 8
    return c


def summary(c, ldy, dtype, K, which=OUTPUTS):
    """one call of the hook on all of c["y"] -> dict of the outputs in `which`, in their documented shapes"""
    res = H.launch(PASS, c, c["y"], ldy, dtype, want=which, nodes=probe_list(c["y"].shape[2], K), n_probes=K)
    return {k: res[k] for k in which}


_RUNS = {}


def run_once(B, T, Cn, ldy, dtype, K):
    key = (B, T, Cn, ldy, dtype, K)
    if key not in _RUNS:
        c = case(B, T, Cn, ldy, dtype)
        _RUNS[key] = (summary(c, ldy, dtype, K), c["F"])
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
@DTYPES
@pytest.mark.parametrize("B,T,Cn,ldy", SHAPES)
def test_summaries_equal_reductions_of_the_stored_field(B, T, Cn, ldy, dtype, K):
    got, F = run_once(B, T, Cn, ldy, dtype, K)
    assert_exact(got, F, probe_list(Cn, K))
    # the mean is a sum in another order than numpy's: against the float64 mean of F with the summation part of the bound
    err = np.abs(got["node_stats"][:, 2].astype(np.float64) - F.astype(np.float64).mean(axis=1))
    assert np.all(err <= (T + 2) * 2.0 ** -24 * np.abs(F).max(axis=1))


def _index_ok(ref, tol, idx, axis, largest):
    j = ref.argmax(axis=axis) if largest else ref.argmin(axis=axis)
    pick = lambda a, i: np.take_along_axis(a, np.expand_dims(i, axis), axis).squeeze(axis)
    return np.abs(pick(ref, idx) - pick(ref, j)) <= pick(tol, idx) + pick(tol, j)


@DTYPES
@pytest.mark.parametrize("B,T,Cn,ldy", SHAPES)
def test_summaries_match_float64(B, T, Cn, ldy, dtype):
    K = 5
    got, _ = run_once(B, T, Cn, ldy, dtype, K)
    c = case(B, T, Cn, ldy, dtype)
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


@DTYPES
@pytest.mark.parametrize("B,T,Cn,ldy", [SHAPES[2], SHAPES[4]])
def test_identical_rows_tie_at_the_first(B, T, Cn, ldy, dtype):
    c = H.inputs(B, T, Cn, dtype, variant("rows"))
    got = summary(c, ldy, dtype, 1, ("node_stats", "node_when"))
    assert (got["node_when"] == 0).all()
    assert np.array_equal(bits(got["node_stats"][:, 0]), bits(got["node_stats"][:, 1]))


@DTYPES
@pytest.mark.parametrize("B,T,Cn,ldy,pair", [SHAPES[2] + ((0, 8),), SHAPES[4] + ((500, 515),)])
def test_identical_nodes_tie_at_the_smaller(B, T, Cn, ldy, pair, dtype):
    """(0, 8): neighbouring threads of one block; (500, 515): the last and the first thread of neighbouring column blocks, so the
    tie is settled by the frame finalize.  Both pairs lie in one group (Cg = 9 and 260)."""
    n1, n2 = pair
    Cg = Cn // _groups(Cn)
    assert n1 // Cg == n2 // Cg and n2 - n1 >= 8
    c = H.inputs(B, T, Cn, dtype, variant(pair))
    got = summary(c, ldy, dtype, 1)
    F = H.field(c, c["y"], ldy, dtype)
    assert np.array_equal(bits(F[:, :, n1]), bits(F[:, :, n2]))
    assert_exact(got, F, probe_list(Cn, 1))
    at_max, at_min = F[:, :, n1] == F.max(axis=2), F[:, :, n1] == F.min(axis=2)
    assert at_max.any() and at_min.any(), "the pair never ties for a frame extremum"
    assert (got["frame_where"][:, :, 0][at_max] == n1).all() and (got["frame_where"][:, :, 1][at_min] == n1).all()


@DTYPES
@pytest.mark.parametrize("B,T,Cn,ldy", SHAPES)
def test_two_launches_are_bitwise_equal(B, T, Cn, ldy, dtype):
    got, _ = run_once(B, T, Cn, ldy, dtype, 5)
    assert not H.same(summary(case(B, T, Cn, ldy, dtype), ldy, dtype, 5), got)          # margins and padding are checked inside


def test_each_output_alone():
    """any subset of the outputs may be asked for; what is computed does not depend on the others"""
    B, T, Cn, ldy = SHAPES[2]
    full, _ = run_once(B, T, Cn, ldy, 1, 5)
    for name in OUTPUTS:
        got = summary(case(B, T, Cn, ldy, 1), ldy, 1, 5, (name,))
        assert np.array_equal(got[name].view(np.int32), full[name].view(np.int32)), name


def test_argument_errors_launch_nothing():
    import torch
    B, T, Cn, K = 2, 3, 16, 2
    c = H.inputs(B, T, Cn, 0)
    d = H.device_inputs(c, c["y"], Cn, 0)
    nodes = np.array([3, 15], np.int32)
    bufs = H.canary_buffers(H.sizes(PASS, B, T, Cn, nodes=nodes, n_probes=K), integer=PASS.integer)
    good = H.hook_args(d, bufs, Cn, 0, B, T, Cn, nodes=nodes, n_probes=K)
    bad = H.common_rejections(good)
    bad += [(dict(no_struct=True), "null argument"), ({k: None for k in OUTPUTS}, "all five outputs are NULL")]
    bad += [(dict(nodes=None), "no probe nodes are given"), (dict(n_probes=0), "no probe nodes are given")]
    bad += [(dict(nodes=np.array([3, 16], np.int32)), "probe nodes[1] = 16 is outside [0, 16)"), (dict(nodes=np.array([-1, 16], np.int32)), "probe nodes[0] = -1 is outside [0, 16)")]
    bad += [({name: good[name] + step}, "misaligned pointer") for name, step in (("node_stats", 4), ("node_when", 8), ("frame_stats", 4), ("frame_where", 4), ("probes", 2))]
    bad += [(dict(y=good["y"] + 8), "misaligned pointer")]
    H.reject_all(PASS, d, bufs, good, bad)
    for name, (_, view) in bufs.items():
        assert not bool((view == (ICANARY if view.dtype == torch.int32 else CANARY)).any()), name
    assert H.margins_intact(bufs)
