"""The host side of the surrogate's exceedance durations (simulgen-vae_amd/predict.py: exceedance_levels, ExceedanceResult; engine.py:
the bindings of sgv_exceedance and sgv_test_recon_exceedance) and the numpy restatement of the exceedance pass
(tests/exceedance_reference.py).  No GPU.

The emulation is held to an independent brute force (itertools.groupby over Python lists) bit for bit, and its excess to float64
within the a-priori bound (T + 1) 2^-24 sum_t |d[t]| (exceedance_reference.worst_ratio)."""
import os
import re
import sys

import numpy as np
import pytest
import torch

import simulgen_vae_amd  # noqa: F401
from simulgen_vae_amd import engine as E
from simulgen_vae_amd.predict import ExceedanceResult, Surrogate, exceedance_levels

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exceedance_reference as XR  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["sgv_exceedance", "sgv_test_recon_exceedance"]
SIDES = pytest.mark.parametrize("side", ["above", "below"])


# ---- the emulation against the brute force ----
PATTERNS = {"all off": "0000000", "all on": "1111111", "a single step at 0": "1000000", "a single step at T - 1": "0000001",
            "mixed": "0110111001", "alternating from 0": "0101010", "alternating from 1": "1010101", "T = 1 off": "0", "T = 1 on": "1"}
EXPECTED = {"all off": (0, -1, -1, 0, 0), "all on": (7, 0, 6, 7, 1), "a single step at 0": (1, 0, 0, 1, 1),
            "a single step at T - 1": (1, 6, 6, 1, 1), "mixed": (6, 1, 9, 3, 3), "alternating from 0": (3, 1, 5, 1, 3),
            "alternating from 1": (4, 0, 6, 1, 4), "T = 1 off": (0, -1, -1, 0, 0), "T = 1 on": (1, 0, 0, 1, 1)}


def _field_of(pattern, side):
    """a one-channel field whose steps exceed the level 1.0 exactly where the pattern has a 1 (the others sit ON the level or
    beyond it on the other side), padded to 8 channels with copies"""
    bitsn = np.array([int(ch) for ch in pattern])
    off = np.where(np.arange(len(pattern)) % 2 == 0, 1.0, 0.25 if side == "above" else 1.75)          # a tie, or the other side
    on = 1.5 if side == "above" else 0.5
    return np.repeat(np.where(bitsn == 1, on, off).astype(np.float32)[:, None], 8, axis=1)


@SIDES
@pytest.mark.parametrize("name", list(PATTERNS))
def test_handwritten_patterns(name, side):
    F = _field_of(PATTERNS[name], side)
    levels = np.ones((1, 8), np.float32)
    stats, excess = XR.emulate(F, levels, side)
    assert stats.dtype == np.int32 and stats.shape == (5, 1, 8) and excess.dtype == np.float32 and excess.shape == (1, 8)
    assert tuple(int(v) for v in stats[:, 0, 0]) == EXPECTED[name] == XR.brute([c == "1" for c in PATTERNS[name]])
    assert np.array_equal(stats, XR.brute_stats(XR.exceeds(F, levels, side)))
    assert np.array_equal(excess, np.full((1, 8), 0.5 * EXPECTED[name][0], np.float32))          # 0.5 per step, exact in fp32
    assert not np.signbit(excess).any()


def _random_case(T, C, L, rows=(2,), seed=0):
    """a field with per-channel magnitudes over many decades and levels inside its range, some of them stored elements"""
    rng = np.random.default_rng(seed + 100 * T + C)
    F = (rng.standard_normal(rows + (T, C)) * np.exp(rng.uniform(-6, 6, C))).astype(np.float32)
    flat = F.reshape(-1, C)
    levels = np.stack([flat[rng.integers(0, flat.shape[0], C), np.arange(C)] for _ in range(L)]).astype(np.float32)          # stored elements: ties
    levels[::2] *= np.float32(0.5)
    return F, levels


@SIDES
@pytest.mark.parametrize("T,C,L", [(1, 8, 1), (2, 72, 3), (5, 16, 4), (33, 24, 3), (200, 8, 4)])
def test_emulation_equals_the_brute_force_on_random_data(T, C, L, side):
    F, levels = _random_case(T, C, L)
    stats, excess = XR.emulate(F, levels, side)
    assert stats.shape == (2, 5, L, C) and excess.shape == (2, L, C)
    assert np.array_equal(stats, XR.brute_stats(XR.exceeds(F, levels, side)))
    ratio = XR.worst_ratio(excess, F, levels, side)
    print(f"  T = {T}, C = {C}, L = {L}, {side}: worst err / bound {ratio:.4f}")
    assert ratio <= 1.0
    assert XR.BLOCK_COLS == 4 * XR.WAVE_COLS and XR.WAVE_COLS == 64 * 8


@SIDES
def test_identities(side):
    T = 33
    F, levels = _random_case(T, 72, 4, rows=(3,), seed=4)
    levels[3] = np.float32(1e30 if side == "above" else -1e30)          # a level nothing exceeds
    stats, excess = XR.emulate(F, levels, side)
    count, first, last, longest, runs = (stats[:, k] for k in range(5))
    assert np.all(count >= longest) and np.all(longest >= (count > 0)) and np.all(runs <= count) and np.all(runs >= (count > 0))
    span = last - first + 1
    assert np.all(span[count > 0] >= count[count > 0])
    assert np.array_equal((span == count) & (count > 0), runs == 1)
    none = count == 0
    assert none[:, 3].all() and none.any() and (~none).any()
    assert np.array_equal(none, first == -1) and np.array_equal(none, last == -1) and np.array_equal(none, (first == -1) & (last == -1))
    assert np.array_equal(none, excess.view(np.int32) == 0)          # +0.0 bit for bit, and only there
    assert np.all(excess[~none] > 0)
    assert (runs > 1).any() and (longest > 1).any()
    # above + below + ties = T
    other = XR.emulate(F, levels, "below" if side == "above" else "above")[0][:, 0]
    ties = (F[:, :, None, :] == levels).sum(axis=1)
    assert ties.any() and np.array_equal(count + other + ties, np.full_like(count, T))


@SIDES
def test_a_level_equal_to_an_element_is_not_exceeded_by_it(side):
    F, _ = _random_case(5, 8, 1, rows=())
    levels = F[2:3].copy()          # step 2 of every channel sits on its level
    stats, excess = XR.emulate(F, levels, side)
    e = XR.exceeds(F, levels, side)
    assert not e[2].any() and np.array_equal(stats[0, 0], e.sum(axis=0)[0]) and np.all(stats[0, 0] <= 4)
    only = np.where(np.arange(5)[:, None] == 2, F, levels)          # every step ON the level: nothing exceeds, on either side
    stats, excess = XR.emulate(only.astype(np.float32), levels, side)
    assert not stats[0].any() and np.all(stats[1:3] == -1) and not stats[3:].any() and np.array_equal(excess.view(np.int32), np.zeros((1, 8), np.int32))


def test_emulation_does_not_depend_on_the_cut_into_batches_or_on_the_other_levels():
    F, levels = _random_case(33, 72, 4, rows=(5,))
    whole = XR.emulate(F, levels)
    for cut in (1, 2, 3):
        parts = [XR.emulate(F[lo:lo + cut], levels) for lo in range(0, 5, cut)]
        assert np.array_equal(whole[0], np.concatenate([p[0] for p in parts]))
        assert np.array_equal(whole[1].view(np.int32), np.concatenate([p[1] for p in parts]).view(np.int32))
    for sel in ([0], [3], [1, 2], [3, 0, 2, 1]):
        st, ex = XR.emulate(F, levels[sel])
        assert np.array_equal(st, whole[0][:, :, sel]) and np.array_equal(ex.view(np.int32), whole[1][:, sel].view(np.int32))


def test_a_nan_exceeds_nothing_and_is_exceeded_by_nothing():
    F = np.ones((3, 8), np.float32)
    F[1] = np.nan
    for side in ("above", "below"):
        stats, excess = XR.emulate(F, np.full((1, 8), 0.5 if side == "above" else 1.5, np.float32), side)
        assert tuple(int(v) for v in stats[:, 0, 0]) == (2, 0, 2, 1, 2) and np.array_equal(excess, np.ones((1, 8), np.float32))
        stats, excess = XR.emulate(F, np.full((1, 8), np.nan, np.float32), side)
        assert tuple(int(v) for v in stats[:, 0, 0]) == (0, -1, -1, 0, 0) and np.array_equal(excess.view(np.int32), np.zeros((1, 8), np.int32))


def test_kernel_levels_are_what_they_say():
    F, _ = _random_case(33, 72, 1, rows=(3,))
    lv = XR.kernel_levels(F)
    assert lv.dtype == np.float32 and lv.shape == (4, 72)
    stats, _ = XR.emulate(F, lv)
    count, first, last, longest, runs = (stats[:, k] for k in range(5))
    assert (runs[:, 0] > 3).any()                                   # the median: many runs
    assert np.all((F[0, 16] == lv[1]))                              # a stored element: the strict tie
    assert not count[:, 2].any()                                    # the maximum: never exceeded
    assert np.all(count[:, 3] == 33) and np.all(longest[:, 3] == 33) and np.all(runs[:, 3] == 1) and not first[:, 3].any() and np.all(last[:, 3] == 32)


# ---- exceedance_levels ----
def test_exceedance_levels_accepts_a_scalar_a_vector_and_rows():
    N = 12
    one = exceedance_levels(2.5, N)
    assert isinstance(one, np.ndarray) and one.dtype == np.float32 and one.shape == (1, N) and one.flags["C_CONTIGUOUS"] and np.all(one == 2.5)
    one[0, 0] = 1.0          # a copy of its own, not a read-only broadcast view
    vec = exceedance_levels([1.0, -2.0, 3.5], N)
    assert vec.shape == (3, N) and vec.flags["C_CONTIGUOUS"] and np.array_equal(vec, np.repeat(np.float32([1.0, -2.0, 3.5])[:, None], N, 1))
    rows = np.random.default_rng(0).standard_normal((E.MAX_LEVELS, N))
    for a in (rows, rows.astype(np.float32), rows.tolist(), np.asfortranarray(rows), torch.from_numpy(rows)):
        got = exceedance_levels(a, N)
        assert isinstance(got, np.ndarray) and got.dtype == np.float32 and got.shape == (4, N) and got.flags["C_CONTIGUOUS"]
        assert np.array_equal(got, rows.astype(np.float32))
    assert exceedance_levels(np.zeros((1, N)), N).shape == (1, N) and exceedance_levels(np.int32(3), N).dtype == np.float32
    assert E.MAX_LEVELS == 4 and XR.MAX_LEVELS == 4


def test_exceedance_levels_names_what_is_wrong():
    N = 12
    with pytest.raises(ValueError, match=r"levels: a scalar, an \[L\] vector or an \[L, N\] array is required, got shape \(2, 3, 12\)"):
        exceedance_levels(np.zeros((2, 3, N)), N)
    with pytest.raises(ValueError, match=r"levels: the last dimension is 11, expected N = 12 \(shape \(3, 11\)\)"):
        exceedance_levels(np.zeros((3, 11)), N)
    with pytest.raises(ValueError, match=r"levels: L = 5 levels, between 1 and 4 are required"):
        exceedance_levels(np.zeros((5, N)), N)
    with pytest.raises(ValueError, match=r"levels: L = 0 levels, between 1 and 4 are required"):
        exceedance_levels(np.zeros((0, N)), N)
    with pytest.raises(ValueError, match=r"levels: L = 12 levels, between 1 and 4 are required .*one level per node is \[1, N\] = \[1, 12\]"):
        exceedance_levels(np.zeros(N), N)
    with pytest.raises(ValueError, match=r"levels = nan is not finite as float32"):
        exceedance_levels(float("nan"), N)
    with pytest.raises(ValueError, match=r"levels\[1\] = inf is not finite as float32"):
        exceedance_levels([1.0, np.inf, np.nan], N)
    lv = np.zeros((3, N))
    lv[2, 5] = np.inf
    lv[1, 7] = np.nan          # the first in row-major order is named
    with pytest.raises(ValueError, match=r"levels\[1, 7\] = nan is not finite as float32"):
        exceedance_levels(lv, N)
    lv = np.zeros((3, N))
    lv[2, 5] = 1e39
    with pytest.raises(ValueError, match=r"levels\[2, 5\] = 1e\+39 is not finite as float32"):
        exceedance_levels(lv, N)
    assert "NOT read back" in exceedance_levels.__doc__


# ---- ExceedanceResult ----
def _result(side="above", T=10, seed=3, **kw):
    F, levels = _random_case(T, 16, 3, rows=(4,), seed=seed)
    stats, excess = XR.emulate(F, levels, side)
    r = dict(stats=torch.from_numpy(stats), excess=torch.from_numpy(excess), levels=torch.from_numpy(levels), side=side, T=T)
    r.update(kw)
    return ExceedanceResult(**r), stats, excess


def test_exceedance_result_views_and_derived_quantities():
    assert ExceedanceResult.FIELDS == ("stats", "excess", "levels", "side", "T")
    res, stats, excess = _result()
    for k, name in enumerate(E.EXCEEDANCE_STATS):
        v = getattr(res, name)
        assert v.dtype == torch.int32 and v.shape == (4, 3, 16) and np.array_equal(v.numpy(), stats[:, k]), name
        assert v.data_ptr() == res.stats[:, k].data_ptr()          # a view of stats, not a copy
    assert E.EXCEEDANCE_STATS == XR.STATS == ("count", "first", "last", "longest", "runs")
    count, first, longest = stats[:, 0], stats[:, 1], stats[:, 3]
    assert (count == 0).any() and (count > 0).any()
    assert res.ever().dtype == torch.bool and np.array_equal(res.ever().numpy(), count > 0)
    assert res.fraction().dtype == torch.float32 and np.array_equal(res.fraction().numpy(), count.astype(np.float32) / np.float32(10))
    assert np.array_equal(res.duration().numpy(), count.astype(np.float32))
    assert np.array_equal(res.duration(0.25).numpy(), count.astype(np.float32) * np.float32(0.25))
    assert np.array_equal(res.longest_duration(0.25).numpy(), longest.astype(np.float32) * np.float32(0.25))
    ft = res.first_time(0.5).numpy()
    assert np.array_equal(np.isnan(ft), count == 0) and np.array_equal(ft[count > 0], first[count > 0].astype(np.float32) * np.float32(0.5))
    assert np.array_equal(res.excess_integral(0.125).numpy(), excess * np.float32(0.125))
    me = res.mean_excess().numpy()
    assert not me[count == 0].any() and np.array_equal(me[count > 0], excess[count > 0] / count[count > 0].astype(np.float32))
    assert np.isfinite(me).all()


def test_worst_takes_the_smallest_node_on_a_tie():
    res, stats, _ = _result()
    stats[0, 0, 0, :] = 0
    stats[0, 0, 0, [5, 9]] = 7          # a tie: node 5
    stats[1, 0, 1, :] = 3               # every node ties: node 0
    stats[2, 0, 2, :] = 0               # nothing exceeds anywhere: node 0, count 0
    stats[3, 0, 0, :] = np.arange(16)   # the last node
    res = ExceedanceResult(stats=torch.from_numpy(stats), excess=None, levels=res.levels, side="above", T=10)
    node, steps = res.worst()
    assert node.dtype == torch.int64 and node.shape == (4, 3) and steps.dtype == torch.int32 and steps.shape == (4, 3)
    assert np.array_equal(node.numpy(), stats[:, 0].argmax(axis=2))          # numpy: the first occurrence
    assert np.array_equal(steps.numpy(), stats[:, 0].max(axis=2))
    assert (int(node[0, 0]), int(steps[0, 0])) == (5, 7) and (int(node[1, 1]), int(steps[1, 1])) == (0, 3)
    assert (int(node[2, 2]), int(steps[2, 2])) == (0, 0) and (int(node[3, 0]), int(steps[3, 0])) == (15, 15)


def test_an_output_that_was_not_asked_for_is_named():
    res, _, _ = _result(excess=None)
    for fn in (res.excess_integral, res.mean_excess):
        with pytest.raises(ValueError, match="the excess was not asked for"):
            fn()
    assert res.ever().shape == (4, 3, 16)
    res, _, _ = _result(stats=None)
    for fn in (res.ever, res.fraction, res.duration, res.longest_duration, res.first_time, res.mean_excess, res.worst):
        with pytest.raises(ValueError, match="the step statistics were not asked for"):
            fn()
    with pytest.raises(ValueError, match="the step statistics were not asked for"):
        res.count
    assert res.excess_integral(2.0).shape == (4, 3, 16)
    with pytest.raises(KeyError):
        ExceedanceResult()
    assert hasattr(Surrogate, "exceedance")


def test_bindings():
    hdr = open(os.path.join(ROOT, "include", "sgvae.h")).read()
    for s in NEW_SYMBOLS:
        assert re.search(rf"\bint {s}\s*\(", hdr), s
        assert s in E.ABI_SYMBOLS
    lib = E.load_library()
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s), s
    assert len(lib.sgv_exceedance.argtypes) == 12 and len(lib.sgv_test_recon_exceedance.argtypes) == 17
    assert E.MAX_LEVELS == 4 and E.EXCEEDANCE_SIDES == {"above": 0, "below": 1} and E.EXCEEDANCE_MAX_T == 65535
    assert re.search(r"SGV_SIDE_ABOVE = 0, SGV_SIDE_BELOW = 1", hdr)
    # without an engine the call is an argument error that says who complains
    assert lib.sgv_exceedance(None, None, None, 1, 1, None, None, None, 1, 0, None, None) == -1 and "sgv_exceedance" in lib.sgv_last_error().decode()
    assert lib.sgv_test_recon_exceedance(0, None, 8, None, None, None, None, None, None, 1, 0, None, None, 1, 1, 8, None) == -1
    assert "sgv_test_recon_exceedance" in lib.sgv_last_error().decode()
    # the noise follows sgv_set_draw_row, and the header says so
    assert hasattr(E.Engine, "exceedance") and "sgv_exceedance" in hdr[hdr.index("Noise of a study"):hdr.index("int sgv_set_draw_row")]
