"""The distribution pass alone (csrc/recon_out.hip: recon_hist_kernel; include/sgvae.h: sgv_test_recon_distribution): the values
val[b, t, n] = (tanh(GroupNorm(y)) - min_n) / scale_n  of the members b of a launch are counted, per (t, n), into K uniform bins
between lo[t, n] and hi[t, n], with a row for the members below and one for those above, and never stored.  Inputs as
tests/test_ensemble_kernel_gpu.py builds them; a quarter of the scales are negative.

Everything here is bit for bit: integer counts against tests/distribution_reference.py, the numpy float32 emulation of the rule, run
on the field F that the existing output pass (sgv_test_recon_physical, layout [B][T][N]) stores for the same inputs.

Shapes (B, T, C, ldy) are those of the ensemble kernel tests: the smallest case; C = 40 has groups of 5 channels (the general path of
the group table); (2, 33, 72, 80) has padding columns and ragged row lanes; 16 members are four rounds of loads; 2080 channels are
five column blocks, the last partly filled; 40 members are more than a launch takes (32: a counter of a launch is a byte), so the
launcher cuts the batch.  Bins: 2 (the smallest), 7 (odd, and K + 2 = 9 rows are not a multiple of the rows the flush takes per
round), 32 (two blocks per CU), 64 (the largest: 132 KiB of LDS, which needs the raised limit)."""
import os
import sys

import numpy as np
import pytest

import simulgen_vae_amd  # noqa: F401
from simulgen_vae_amd import engine as E

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import distribution_reference as DR  # noqa: E402
import recon_kernel_common as H  # noqa: E402
from recon_kernel_common import DTYPES, ICANARY  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 8, 8), (3, 5, 40, 40), (2, 33, 72, 80), (16, 3, 72, 72), (4, 9, 2080, 2080), (40, 2, 72, 72)]     # (B, T, C, ldy)
BINS = [2, 7, 32, 64]
PASS = H.Pass("distribution", lambda b, T, Cn, bins, count_before: {"lo": (T, Cn), "hi": (T, Cn), "counts": (bins + 2, T, Cn)}, ("counts",),
              lambda a: (a["count_before"], H.struct(E.DistributionState, a, ("lo", "hi", "counts"), bins=a["bins"])), integer=("counts",))


def case(B, T, Cn, ldy, dtype):
    """inputs, the stored field F and its envelope of one (shape, dtype), computed once and left alone"""
    c = H.case(__name__, B, T, Cn, ldy, dtype, extras=lambda c: {"lo": c["F"].min(0), "hi": c["F"].max(0)})
    assert np.isfinite(c["F"]).all()
    return c


def launch(c, y, ldy, dtype, K, lo, hi, counts=None, count_before=0):
    """one call of the hook on the members y [b, T, C] -> counts [K + 2, T, C] int32.  counts: the state to add to (None: zeros)."""
    b, T, Cn = y.shape
    state = {"counts": np.zeros((K + 2, T, Cn), np.int32) if counts is None else counts}
    return H.launch(PASS, c, y, ldy, dtype, {"lo": lo, "hi": hi}, state=state, bins=K, count_before=count_before)["counts"]


def report(got, want):
    i = np.argwhere(got != want)
    print(len(i), "mismatches, first (row, t, n):", i[:4].tolist(), got[tuple(i[:4].T)], want[tuple(i[:4].T)])


_RUNS = {}


def run_once(B, T, Cn, ldy, dtype, K):
    """the single launch into zeros between the members' own extrema"""
    key = (B, T, Cn, ldy, dtype, K)
    if key not in _RUNS:
        c = case(*key[:5])
        _RUNS[key] = launch(c, c["y"], ldy, dtype, K, c["lo"], c["hi"])
    return _RUNS[key]


@DTYPES
@pytest.mark.parametrize("K", BINS)
@pytest.mark.parametrize("B,T,Cn,ldy", SHAPES)
def test_counts_between_the_extrema_equal_the_emulation_on_the_stored_field(B, T, Cn, ldy, K, dtype):
    c = case(B, T, Cn, ldy, dtype)
    got = run_once(B, T, Cn, ldy, dtype, K)
    want = DR.update(c["F"], c["lo"], c["hi"], K)
    if not np.array_equal(got, want):
        report(got, want)
    assert got.dtype == np.int32 and np.array_equal(got, want)
    assert not got[0].any() and not got[K + 1].any()                                   # nothing outside the members' own envelope
    assert np.array_equal(got.sum(0), np.full((T, Cn), B))
    assert (got[1] >= 1).all() and (got[K][c["hi"] > c["lo"]] >= 1).all()              # the minimum is in bin 1, the maximum in bin K


@DTYPES
@pytest.mark.parametrize("K", [7, 64])
@pytest.mark.parametrize("B,T,Cn,ldy", SHAPES[1:])
def test_a_narrower_range_counts_what_is_below_and_above(B, T, Cn, ldy, K, dtype):
    c = case(B, T, Cn, ldy, dtype)
    F, span = c["F"], c["hi"] - c["lo"]
    lo, hi = (c["lo"] + np.float32(0.3) * span).astype(np.float32), (c["hi"] - np.float32(0.2) * span).astype(np.float32)
    got = launch(c, c["y"], ldy, dtype, K, lo, hi)
    assert np.array_equal(got[0], (F < lo).sum(0)) and np.array_equal(got[K + 1], (F > hi).sum(0))
    assert got[0].sum() > 0 and got[K + 1].sum() > 0
    want = DR.update(F, lo, hi, K)
    if not np.array_equal(got, want):
        report(got, want)
    assert np.array_equal(got, want) and np.array_equal(got.sum(0), np.full((T, Cn), B))


SPLITS = [((16, 3, 72, 72), (5, 11)), ((3, 5, 40, 40), (1, 1, 1)), ((4, 9, 2080, 2080), (3, 1)), ((40, 2, 72, 72), (33, 7))]


@DTYPES
@pytest.mark.parametrize("K", [7, 32])
@pytest.mark.parametrize("shape,parts", SPLITS, ids=[f"{s[0]}={'+'.join(map(str, p))}" for s, p in SPLITS])
def test_any_split_added_to_a_state_gives_the_bits_of_one_launch_plus_that_state(shape, parts, K, dtype):
    B, T, Cn, ldy = shape
    assert sum(parts) == B
    c = case(B, T, Cn, ldy, dtype)
    base = np.random.default_rng(K).integers(0, 1 << 20, (K + 2, T, Cn)).astype(np.int32)          # a state that is not zero
    state, at = base, 0
    for n in parts:
        state = launch(c, c["y"][at:at + n], ldy, dtype, K, c["lo"], c["hi"], counts=state, count_before=at)
        at += n
    assert np.array_equal(state, base + run_once(B, T, Cn, ldy, dtype, K))


@DTYPES
@pytest.mark.parametrize("K", BINS)
@pytest.mark.parametrize("B,T,Cn,ldy", [(3, 5, 40, 40), (4, 9, 2080, 2080)])
def test_a_value_equal_to_a_bound_is_inside(B, T, Cn, ldy, K, dtype):
    c = case(B, T, Cn, ldy, dtype)
    F = c["F"]
    b0, t0 = B - 1, T // 2
    far = (c["hi"] - c["lo"]) + np.float32(1)
    # lo[t0] = the stored values of member b0: it is in bin 1 there and not below
    lo, hi = np.array(c["lo"] - far), np.array(c["hi"] + far)
    lo[t0] = F[b0, t0]
    got = launch(c, c["y"], ldy, dtype, K, lo, hi)
    assert np.array_equal(got, DR.update(F, lo, hi, K))
    others = np.delete(F[:, t0], b0, axis=0)
    assert np.array_equal(got[0, t0], (others < lo[t0]).sum(0))                        # member b0 itself is not counted below
    assert (got[1, t0] >= 1 + (others == lo[t0]).sum(0)).all() and (DR.rows(F[b0, t0], lo[t0], hi[t0], K) == 1).all()
    # hi[t0] = them: it is in bin K there and not above
    lo, hi = np.array(c["lo"] - far), np.array(c["hi"] + far)
    hi[t0] = F[b0, t0]
    got = launch(c, c["y"], ldy, dtype, K, lo, hi)
    assert np.array_equal(got, DR.update(F, lo, hi, K))
    assert np.array_equal(got[K + 1, t0], (others > hi[t0]).sum(0))
    assert (got[K, t0] >= 1).all() and (DR.rows(F[b0, t0], lo[t0], hi[t0], K) == K).all()


@DTYPES
@pytest.mark.parametrize("K", [2, 64])
def test_duplicated_members_in_a_degenerate_range_all_land_in_bin_one(K, dtype):
    B, T, Cn, ldy = 2, 33, 72, 80
    c = dict(case(B, T, Cn, ldy, dtype))
    y = np.array(c["y"])
    y[1] = y[0]                                   # identical rows and identical statistics
    F = H.field(c, y, ldy, dtype)
    assert np.array_equal(F[0].view(np.int32), F[1].view(np.int32))
    got = launch(c, y, ldy, dtype, K, F[0], F[0])
    want = np.zeros((K + 2, T, Cn), np.int32)
    want[1] = 2
    assert np.array_equal(got, want)


@DTYPES
@pytest.mark.parametrize("B,T,Cn,ldy", SHAPES)
def test_two_launches_are_bitwise_equal(B, T, Cn, ldy, dtype):
    c = case(B, T, Cn, ldy, dtype)
    assert np.array_equal(launch(c, c["y"], ldy, dtype, 32, c["lo"], c["hi"]), run_once(B, T, Cn, ldy, dtype, 32))


def test_the_largest_count_is_accepted():
    B, T, Cn, ldy, dtype, K = 3, 5, 40, 40, 0, 7
    c = case(B, T, Cn, ldy, dtype)
    got = launch(c, c["y"], ldy, dtype, K, c["lo"], c["hi"], count_before=(1 << 24) - B)
    assert np.array_equal(got, run_once(B, T, Cn, ldy, dtype, K))          # count_before does not reach the counts


def test_rejected_arguments_write_nothing():
    import torch
    B, T, Cn, ldy, dtype, K = 3, 5, 40, 40, 0, 7
    c = case(B, T, Cn, ldy, dtype)
    d = H.device_inputs(c, c["y"], ldy, dtype)
    bufs = H.canary_buffers(H.sizes(PASS, B, T, Cn, bins=K, count_before=0), integer=PASS.integer)
    bufs["lo"][1].copy_(torch.from_numpy(np.array(c["lo"]).reshape(-1)).cuda())
    bufs["hi"][1].copy_(torch.from_numpy(np.array(c["hi"]).reshape(-1)).cuda())
    bufs["counts"][1].zero_()
    good = H.hook_args(d, bufs, ldy, dtype, B, T, Cn, bins=K, count_before=0)
    bad = H.common_rejections(good) + [(dict(no_struct=True), "null argument")]
    bad += [({k: None}, "lo, hi and counts are all required") for k in bufs]
    bad += [(dict(bins=v), "is outside [2, 64]") for v in (-1, 0, 1, 65, 1 << 20)]
    bad += [({k: good[k] + 4}, "misaligned pointer") for k in bufs]
    bad += [(dict(count_before=v), "outside [0, 2^24]") for v in (-1, (1 << 24) - B + 1, 1 << 40)]
    H.reject_all(PASS, d, bufs, good, bad)
    assert int(bufs["counts"][0][0]) == ICANARY
    assert np.array_equal(H.outputs_of(PASS, bufs, B, T, Cn, bins=K, count_before=0)["counts"], run_once(B, T, Cn, ldy, dtype, K))
