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
import ctypes as C
import os
import sys

import numpy as np
import pytest

import simulgen_vae_amd  # noqa: F401
from simulgen_vae_amd import engine as E

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import distribution_reference as DR  # noqa: E402
from recon_kernel_common import (ICANARY, _bf16, base_inputs, canary_buffers, device_inputs, field, hook_inputs, margins_intact,  # noqa: E402
                                 padding_intact)

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 8, 8), (3, 5, 40, 40), (2, 33, 72, 80), (16, 3, 72, 72), (4, 9, 2080, 2080), (40, 2, 72, 72)]     # (B, T, C, ldy)
BINS = [2, 7, 32, 64]
DTYPES = pytest.mark.parametrize("dtype", [0, 1], ids=["f32", "bf16"])

_CASES = {}


def case(B, T, Cn, ldy, dtype):
    """inputs, the stored field F and its envelope of one (shape, dtype), computed once and left alone"""
    key = (B, T, Cn, ldy, dtype)
    if key not in _CASES:
        import torch
        c = base_inputs(B, T, Cn, dtype)
        if dtype == 1:
            c["y"] = _bf16(torch, c["y"])
        c["F"] = field(c, c["y"], ldy, dtype)
        assert np.isfinite(c["F"]).all()
        c["lo"], c["hi"] = c["F"].min(0), c["F"].max(0)
        for v in c.values():
            v.setflags(write=False)
        _CASES[key] = c
    return _CASES[key]


def launch(c, y, ldy, dtype, K, lo, hi, counts=None, count_before=0):
    """one call of the hook on the members y [b, T, C] -> counts [K + 2, T, C] int32.  counts: the state to add to (None: zeros)."""
    import torch
    lib = E.load_library()
    b, T, Cn = y.shape
    d = device_inputs(c, y, ldy, dtype)
    bufs = canary_buffers({"lo": T * Cn, "hi": T * Cn, "counts": (K + 2) * T * Cn}, integer=("counts",))
    for name, a in (("lo", lo), ("hi", hi)):
        bufs[name][1].copy_(torch.from_numpy(np.array(a, np.float32).reshape(-1)).cuda())
    bufs["counts"][1].copy_(torch.from_numpy(np.ascontiguousarray(np.zeros((K + 2, T, Cn), np.int32) if counts is None else counts).reshape(-1)).cuda())
    before = {n: bufs[n][1].clone() for n in ("lo", "hi")}
    st = E.DistributionState(lo=bufs["lo"][1].data_ptr(), hi=bufs["hi"][1].data_ptr(), counts=bufs["counts"][1].data_ptr(), bins=K)
    rc = lib.sgv_test_recon_distribution(dtype, *hook_inputs(d, ldy), count_before, C.byref(st), b, T, Cn, None)
    assert rc == 0, lib.sgv_last_error().decode()
    assert margins_intact(bufs), "a margin around a buffer was written"
    assert padding_intact(d, Cn), "the padding columns of y were written"
    for n in before:
        assert bool((bufs[n][1].view(torch.int32) == before[n].view(torch.int32)).all()), f"{n} was written"
    return bufs["counts"][1].cpu().numpy().reshape(K + 2, T, Cn)


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
    F = field(c, y, ldy, dtype)
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
    lib = E.load_library()
    B, T, Cn, ldy, dtype, K = 3, 5, 40, 40, 0, 7
    c = case(B, T, Cn, ldy, dtype)
    d = device_inputs(c, c["y"], ldy, dtype)
    bufs = canary_buffers({"lo": T * Cn, "hi": T * Cn, "counts": (K + 2) * T * Cn}, integer=("counts",))
    bufs["lo"][1].copy_(torch.from_numpy(np.array(c["lo"]).reshape(-1)).cuda())
    bufs["hi"][1].copy_(torch.from_numpy(np.array(c["hi"]).reshape(-1)).cuda())
    bufs["counts"][1].zero_()
    keep = {n: b.clone() for n, (b, _) in bufs.items()}
    ptr = {n: v.data_ptr() for n, (_, v) in bufs.items()}
    good = dict(dtype=dtype, y=d["y"].data_ptr(), ldy=ldy, sums=d["sums"].data_ptr(), gamma=d["gamma"].data_ptr(), beta=d["beta"].data_ptr(),
                scale=d["scale"].data_ptr(), mn=d["mn"].data_ptr(), count_before=0, B=B, T=T, Cn=Cn, st=True, bins=K, **ptr)

    def call(**over):
        a = dict(good, **over)
        st = E.DistributionState(lo=a["lo"], hi=a["hi"], counts=a["counts"], bins=a["bins"])
        return lib.sgv_test_recon_distribution(a["dtype"], a["y"], a["ldy"], a["sums"], a["gamma"], a["beta"], a["scale"], a["mn"], a["count_before"],
                                               C.byref(st) if a["st"] else None, a["B"], a["T"], a["Cn"], None)

    bad = [(dict([(k, None)]), "null argument") for k in ("y", "sums", "gamma", "beta", "scale", "mn")]
    bad += [(dict(st=False), "null argument"), (dict(dtype=2), "dtype must be")]
    bad += [(dict([(k, None)]), "lo, hi and counts are all required") for k in ptr]
    bad += [(dict(bins=v), "is outside [2, 64]") for v in (-1, 0, 1, 65, 1 << 20)]
    bad += [(dict(B=0), "B, T >= 1"), (dict(T=0), "B, T >= 1"), (dict(Cn=0), "C % 8 == 0"), (dict(Cn=4), "C % 8 == 0"), (dict(Cn=36), "C % 8 == 0")]
    bad += [(dict(ldy=32), "row stride"), (dict(ldy=44), "row stride")]
    bad += [(dict(y=good["y"] + 4), "misaligned")] + [(dict([(k, ptr[k] + 4)]), "misaligned") for k in ptr]
    bad += [(dict(count_before=-1), "outside [0, 2^24]"), (dict(count_before=(1 << 24) - B + 1), "outside [0, 2^24]"), (dict(count_before=1 << 40), "outside [0, 2^24]")]
    for kw, msg in bad:
        assert call(**kw) == -1, kw          # SGV_ERR_ARG
        assert msg in lib.sgv_last_error().decode(), (kw, lib.sgv_last_error().decode())
    torch.cuda.synchronize()
    for n, (b, _) in bufs.items():
        assert bool((b.view(torch.int32) == keep[n].view(torch.int32)).all()), f"{n} was written by a rejected call"
    assert int(bufs["counts"][0][0]) == ICANARY
    assert call() == 0, lib.sgv_last_error().decode()
    assert np.array_equal(bufs["counts"][1].cpu().numpy().reshape(K + 2, T, Cn), run_once(B, T, Cn, ldy, dtype, K))
