"""The host side of the surrogate's load cycles and rates (simulgen-vae_amd/predict.py: cycles_gate, CyclesResult; engine.py: the
bindings of sgv_cycles and sgv_test_recon_cycles) and the numpy restatement of the cycles pass (tests/cycles_reference.py).  No GPU.

The vectorised emulation is held bit for bit to two independent walks over Python lists -- brute0 at gate 0 (runs collapsed with
itertools.groupby, turning points = the first element and the strict interior extrema) and turns_list at gates > 0 (a scalar walk of
the state machine) -- and its path, range_sum and damage to float64 within the a-priori bounds (cycles_reference.ratios)."""
import os
import re
import sys

import numpy as np
import pytest
import torch

import simulgen_vae_amd  # noqa: F401
from simulgen_vae_amd import engine as E
from simulgen_vae_amd.predict import CyclesResult, Surrogate, cycles_gate

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cycles_reference as CR  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["sgv_cycles", "sgv_test_recon_cycles"]
f32 = np.float32
HAND = [0, 1, 0.5, 2, -1, -0.5, -3, 4]


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _histories(T, C=24, rows=(2,), seed=0):
    """random histories with per-channel magnitudes over many decades; channel 0 is constant, and from T = 3 on one step is
    duplicated in every channel (a plateau)"""
    rng = np.random.default_rng(seed + 100 * T + C)
    F = (rng.standard_normal(rows + (T, C)) * np.exp(rng.uniform(-6, 6, C))).astype(f32)
    F[..., 0] = f32(1.25)
    if T >= 3:
        F[..., T // 2, :] = F[..., T // 2 - 1, :]
    return F


def _check_against_lists(F, gate, m, walk):
    out = CR.emulate(F, gate, m)
    lead, C = F.shape[:-2], F.shape[-1]
    for idx in np.ndindex(*lead):
        for c in range(C):
            h = F[idx + (slice(None), c)].tolist()
            rev, ranges, rsum, rmax, dmg, opn = walk(h, c)
            got = out["ranges"][idx + (slice(None), c)]
            assert int(out["reversals"][idx + (c,)]) == rev == (len(ranges) + 1 if rev else 0), (idx, c)
            assert [bits(f32(v)).item() for v in (rsum, rmax, dmg, opn)] == [bits(v).item() for v in got], (idx, c)
            rise, fall, rw, fw, path = CR.rates_list(h)
            assert [bits(f32(v)).item() for v in (rise, fall, path)] == [bits(v).item() for v in out["rates"][idx + (slice(None), c)]], (idx, c)
            assert (rw, fw) == tuple(int(v) for v in out["rate_when"][idx + (slice(None), c)]), (idx, c)
    return out


# ---- the emulation against the two list walks ----
@pytest.mark.parametrize("m", [1, 3, 8])
@pytest.mark.parametrize("T", [1, 2, 3, 5, 33])
def test_emulation_equals_the_brute_force_at_gate_0(T, m):
    F = _histories(T)
    out = _check_against_lists(F, np.zeros(24, f32), m, lambda h, c: CR.brute0(h, m))
    assert out["reversals"].dtype == np.int32 and out["reversals"].shape == (2, 24) and out["ranges"].shape == (2, 4, 24)
    assert out["rate_when"].dtype == np.int32 and out["rate_when"].shape == (2, 2, 24) and out["rates"].shape == (2, 3, 24)
    # the constant history: nothing turns, everything +0.0
    assert not out["reversals"][:, 0].any() and not bits(out["ranges"][:, :, 0]).any() and not bits(out["rates"][:, :, 0]).any()
    if T >= 5:
        assert (out["reversals"] > 2).any()


@pytest.mark.parametrize("m", [1, 3, 8])
@pytest.mark.parametrize("T", [2, 3, 5, 33, 200])
def test_emulation_equals_the_scalar_walk_at_gates_above_0(T, m):
    F = _histories(T, seed=1)
    p2p = (F.max(axis=(0, 1)) - F.min(axis=(0, 1))).astype(f32)
    for share in (0.05, 0.25, 0.6, 2.0):
        gate = (p2p * f32(share)).astype(f32)
        out = _check_against_lists(F, gate, m, lambda h, c: CR.turns_list(h, gate[c], m))
        if share == 2.0:
            assert not out["reversals"].any()
    if T >= 33:
        gate = (p2p * f32(0.25)).astype(f32)
        rev = CR.emulate(F, gate, m)["reversals"]
        assert (rev > 3).any() and (rev < CR.emulate(F, np.zeros_like(gate), m)["reversals"]).any()          # the gate filters


def test_the_two_list_walks_agree_at_gate_0():
    F = _histories(33, seed=2)
    for c in range(24):
        h = F[0, :, c].tolist()
        a, b = CR.brute0(h, 3), CR.turns_list(h, 0.0, 3)
        assert a[0] == b[0] and [bits(f32(v)).item() for v in a[1] + list(a[2:])] == [bits(f32(v)).item() for v in b[1] + list(b[2:])]


def _hand(gate, m=3):
    F = np.repeat(np.array(HAND, f32)[:, None], 8, axis=1)
    out = CR.emulate(F, np.full(8, gate, f32), m)
    return int(out["reversals"][0]), [float(v) for v in out["ranges"][:, 0]], [float(v) for v in out["rates"][:, 0]], [int(v) for v in out["rate_when"][:, 0]]


def test_hand_pattern():
    rev, ranges, rates, when = _hand(0.0)
    assert (rev, ranges) == (7, [9.0, 3.0, 47.25, 7.0])
    assert rates == [7.0, -3.0, 16.0] and when == [7, 4]
    for gate in (0.6, 1.6):
        rev, ranges, rates, when = _hand(gate)
        assert (rev, ranges) == (3, [7.0, 5.0, 133.0, 7.0]), gate
        assert rates == [7.0, -3.0, 16.0] and when == [7, 4]
    assert CR.brute0(HAND, 3)[0] == 7 and [float(v) for v in CR.brute0(HAND, 3)[2:]] == [9.0, 3.0, 47.25, 7.0]
    assert CR.turns_list(HAND, 0.6, 3)[0] == 3 and [float(v) for v in CR.turns_list(HAND, 1.6, 3)[2:]] == [7.0, 5.0, 133.0, 7.0]
    # mirrored: the same ranges, rise and fall exchanged
    F = -np.repeat(np.array(HAND, f32)[:, None], 8, axis=1)
    out = CR.emulate(F, np.zeros(8, f32), 3)
    assert int(out["reversals"][0]) == 7 and [float(v) for v in out["ranges"][:, 0]] == [9.0, 3.0, 47.25, 7.0]
    assert [float(v) for v in out["rates"][:, 0]] == [3.0, -7.0, 16.0] and [int(v) for v in out["rate_when"][:, 0]] == [4, 7]


def test_a_gate_above_the_peak_to_peak_leaves_the_open_excursion_alone():
    F = _histories(33, rows=(3,), seed=3)
    p2p = (F.max(axis=1) - F.min(axis=1)).astype(f32)          # per sample and node
    out = CR.emulate(F, (p2p.max(axis=0) * f32(2)).astype(f32), 3)
    assert not out["reversals"].any() and not bits(out["ranges"][:, :3]).any()
    assert np.array_equal(bits(out["ranges"][:, 3]), bits(p2p))
    # and exactly the peak-to-peak does not trigger either: the comparison is strict
    one = F[:1]
    out = CR.emulate(one, p2p[0], 3)
    assert not out["reversals"].any() and np.array_equal(bits(out["ranges"][:, 3]), bits(p2p[:1]))


def test_a_gate_equal_to_the_first_difference_does_not_trigger():
    F = _histories(5, seed=4)[0]
    first = np.abs((F[1] - F[0]).astype(f32))
    held = np.where(np.arange(5)[:, None] < 2, F, F[1])          # the history stays where step 1 put it
    out = CR.emulate(held.astype(f32), first, 3)
    assert not out["reversals"].any() and np.array_equal(bits(out["ranges"][3]), bits(first))
    lower = np.nextafter(first, f32(-1))
    out = CR.emulate(held.astype(f32), np.maximum(lower, 0).astype(f32), 3)
    assert np.array_equal(out["reversals"], (first > 0).astype(np.int32))


def test_a_single_time_step():
    F = _histories(1, rows=(3,))
    out = CR.emulate(F, np.zeros(24, f32), 3)
    assert not out["reversals"].any() and not bits(out["ranges"]).any() and not bits(out["rates"]).any()
    assert np.all(out["rate_when"] == -1)
    assert CR.rates_list([1.0]) == (0, 0, -1, -1, 0) and CR.brute0([1.0])[0] == 0 and CR.turns_list([1.0], 0.0)[0] == 0


def test_ties_of_the_rates_go_to_the_smallest_step():
    h = np.array([0, 2, 1, 3, 2, 4, 4, 4], f32)          # rise 2 at steps 1, 3, 5; fall -1 at steps 2, 4; a plateau at the end
    out = CR.emulate(np.repeat(h[:, None], 8, axis=1), np.zeros(8, f32), 1)
    assert [int(v) for v in out["rate_when"][:, 0]] == [1, 2] and [float(v) for v in out["rates"][:, 0]] == [2.0, -1.0, 8.0]
    h = np.array([5, 5, 5], f32)          # all differences 0: both at step 1
    out = CR.emulate(np.repeat(h[:, None], 8, axis=1), np.zeros(8, f32), 1)
    assert [int(v) for v in out["rate_when"][:, 0]] == [1, 1] and not bits(out["rates"]).any()
    h = np.array([0, -1, -3], f32)         # only falls: rise is the least negative, at its first step
    out = CR.emulate(np.repeat(h[:, None], 8, axis=1), np.zeros(8, f32), 1)
    assert [float(v) for v in out["rates"][:, 0]] == [-1.0, -2.0, 3.0] and [int(v) for v in out["rate_when"][:, 0]] == [1, 2]


def test_emulation_does_not_depend_on_the_cut_into_batches():
    F = _histories(33, C=72, rows=(5,), seed=5)
    gate = ((F.max(axis=(0, 1)) - F.min(axis=(0, 1))) * f32(0.25)).astype(f32)
    whole = CR.emulate(F, gate, 3)
    for cut in (1, 2, 3):
        parts = [CR.emulate(F[lo:lo + cut], gate, 3) for lo in range(0, 5, cut)]
        for k in whole:
            assert np.array_equal(bits(whole[k]), bits(np.concatenate([p[k] for p in parts]))), (cut, k)


def test_the_exponent_changes_the_damage_alone():
    F = _histories(33, seed=6)
    gate = np.zeros(24, f32)
    base = CR.emulate(F, gate, 1)
    assert np.array_equal(bits(base["ranges"][:, 0]), bits(base["ranges"][:, 2]))          # m = 1: the damage is the range sum
    for m in (2, 3, 8):
        out = CR.emulate(F, gate, m)
        for k in ("reversals", "rate_when", "rates"):
            assert np.array_equal(bits(out[k]), bits(base[k])), (m, k)
        assert np.array_equal(bits(out["ranges"][:, [0, 1, 3]]), bits(base["ranges"][:, [0, 1, 3]]))
        assert not np.array_equal(bits(out["ranges"][:, 2]), bits(base["ranges"][:, 2]))


@pytest.mark.parametrize("scale", [1e-3, 1.0, 37.0])
@pytest.mark.parametrize("T", [2, 5, 33, 200])
def test_float64_bounds(T, scale):
    rng = np.random.default_rng(T)
    F = (np.tanh(rng.standard_normal((2, T, 40)) * 1.5) * scale).astype(f32)
    worst = {}
    for m in (1, 3, 8):
        for g in (0.0, 0.25, 1.0):
            r = CR.ratios(CR.emulate(F, np.full(40, g * scale, f32), m), F, np.full(40, g * scale, f32), m)
            for k, v in r.items():
                worst[k] = max(worst.get(k, 0.0), v)
    print(f"  T = {T}, scale = {scale}: worst err / bound " + ", ".join(f"{k} {v:.4f}" for k, v in sorted(worst.items())))
    assert set(worst) == {"path", "range_sum", "damage"}
    assert worst["path"] <= 1.0 and worst["range_sum"] <= 1.0 and worst["damage"] <= 1.0


def test_kernel_gates_are_what_they_say():
    F = _histories(33, C=72, rows=(3,), seed=7)
    g = CR.kernel_gates(F)
    assert g.dtype == f32 and g.shape == (4, 72) and np.all(g >= 0) and not g[0].any()
    assert (CR.emulate(F, g[1], 3)["reversals"] > 3).any()
    out = CR.emulate(F[:1, :2], g[2], 3)          # sample 0 does not trigger at t = 1
    assert not out["reversals"].any()
    out = CR.emulate(F, g[3], 3)
    assert not out["reversals"].any() and np.array_equal(bits(out["ranges"][:, 3]), bits((F.max(axis=1) - F.min(axis=1)).astype(f32)))
    assert CR.BLOCK_COLS == 4 * CR.WAVE_COLS and CR.WAVE_COLS == 64 * 8
    assert not CR.kernel_gates(F[:, :1])[2].any()          # T = 1: no first difference


# ---- cycles_gate ----
def test_cycles_gate_accepts_a_scalar_and_a_vector():
    N = 12
    one = cycles_gate(0.5, N)
    assert isinstance(one, np.ndarray) and one.dtype == f32 and one.shape == (N,) and one.flags["C_CONTIGUOUS"] and np.all(one == 0.5)
    one[0] = 1.0          # a copy of its own, not a read-only broadcast view
    vec = np.random.default_rng(0).uniform(0, 3, N)
    for a in (vec, vec.astype(f32), vec.tolist(), torch.from_numpy(vec)):
        got = cycles_gate(a, N)
        assert isinstance(got, np.ndarray) and got.dtype == f32 and got.shape == (N,) and np.array_equal(got, vec.astype(f32))
    assert not cycles_gate(0, N).any() and cycles_gate(np.int32(3), N).dtype == f32 and np.all(np.isinf(cycles_gate(np.inf, N)))


def test_cycles_gate_names_what_is_wrong():
    N = 12
    for bad in (np.zeros((1, N)), np.zeros(N - 1), np.zeros((N, 1)), np.zeros(0)):
        with pytest.raises(ValueError, match=r"gate: a scalar or an \[N\] = \[12\] vector is required, got shape"):
            cycles_gate(bad, N)
    with pytest.raises(ValueError, match=r"gate = -0.5 is not a gate: a value >= 0 is required"):
        cycles_gate(-0.5, N)
    with pytest.raises(ValueError, match=r"gate = nan is not a gate"):
        cycles_gate(float("nan"), N)
    g = np.ones(N)
    g[7] = -1e-30
    g[9] = np.nan
    with pytest.raises(ValueError, match=r"gate\[7\] = -1e-30 is not a gate"):
        cycles_gate(g, N)
    g[7] = 0.0
    with pytest.raises(ValueError, match=r"gate\[9\] = nan is not a gate"):
        cycles_gate(g, N)
    assert "NOT read back" in cycles_gate.__doc__


# ---- CyclesResult ----
def _result(F, gate, m, **kw):
    out = CR.emulate(F, gate, m)
    r = {k: torch.from_numpy(v) for k, v in out.items()}
    r.update(gate=torch.from_numpy(np.asarray(gate, f32)), exponent=m, T=F.shape[-2])
    r.update(kw)
    return CyclesResult(**r), out


def test_cycles_result_on_sampled_sinusoids():
    T, N, amp = 400, 8, f32(2.5)
    ks = np.arange(1, N + 1)
    t = np.arange(T)[:, None] / T
    # k periods in node k - 1.  Started on a crest the history has 2 k - 1 extrema inside and the start itself turns: 2 k - 1 +- 1
    crest = (amp * np.cos(2 * np.pi * ks * t)).astype(f32)[None]
    rev = CR.emulate(crest, np.zeros(N, f32), 3)["reversals"][0]
    assert np.all(np.abs(rev - (2 * ks - 1)) <= 1)
    # started in between, all 2 k extrema lie inside and the start turns as well: 2 k + 1
    F = (amp * np.sin(2 * np.pi * ks * t + 0.3)).astype(f32)[None]
    res, out = _result(F, np.zeros(N, f32), 3)
    assert CyclesResult.FIELDS == ("reversals", "ranges", "rate_when", "rates", "gate", "exponent", "T")
    rev = res.reversals.numpy()[0]
    assert np.array_equal(rev, 2 * ks + 1)
    half = res.half_cycles().numpy()[0]
    assert res.half_cycles().dtype == torch.int32 and np.array_equal(half, np.maximum(rev - 1, 0))
    full = half >= 2          # a range between two extrema of the sinusoid is twice the amplitude (to the sampling)
    assert full.any() and np.allclose(res.range_max.numpy()[0][full], 2 * amp, rtol=2e-3)
    mean = res.mean_range().numpy()[0]
    assert np.array_equal(mean[half > 0], (out["ranges"][0, 0] / np.maximum(half, 1).astype(f32))[half > 0]) and not mean[half == 0].any()
    for k, name in enumerate(("range_sum", "range_max", "damage_sum", "open")):
        v = getattr(res, name)
        assert v.shape == (1, N) and v.data_ptr() == res.ranges[:, k].data_ptr() and np.array_equal(v.numpy(), out["ranges"][:, k])
    for k, name in enumerate(("rise", "fall", "path")):
        v = getattr(res, name)
        assert v.data_ptr() == res.rates[:, k].data_ptr() and np.array_equal(v.numpy(), out["rates"][:, k])
    assert np.array_equal(res.rise_when.numpy(), out["rate_when"][:, 0]) and np.array_equal(res.fall_when.numpy(), out["rate_when"][:, 1])
    d = res.damage().numpy()
    want = f32(0.5) * (out["ranges"][:, 2] + out["ranges"][:, 3] ** 3)
    assert d.dtype == f32 and np.allclose(d, want, rtol=1e-6)
    assert np.allclose(res.damage(coefficient=4.0, include_open=False).numpy(), out["ranges"][:, 2] * f32(0.125), rtol=1e-6)
    # the steepest slope of a sin(2 pi k t / T) is 2 pi k a / T per step
    peak = res.peak_rate(0.5).numpy()[0]
    assert np.array_equal(peak, np.maximum(np.abs(out["rates"][0, 0]), np.abs(out["rates"][0, 1])) / f32(0.5))
    assert np.allclose(peak * 0.5, 2 * np.pi * ks * amp / T, rtol=2e-2)
    assert np.array_equal(res.rise_time(0.25).numpy(), out["rate_when"][:, 0].astype(f32) * f32(0.25))
    assert np.array_equal(res.fall_time(0.25).numpy(), out["rate_when"][:, 1].astype(f32) * f32(0.25))
    assert np.allclose(res.path_length().numpy()[0], 4 * amp * ks, rtol=5e-3)          # the total variation of k periods
    node, top = res.worst()
    assert node.dtype == torch.int64 and node.shape == (1,) and int(node[0]) == int(np.argmax(d[0])) == N - 1 and float(top[0]) == d[0].max()


def test_cycles_result_at_one_time_step_and_on_a_tie():
    F = _histories(1, rows=(2,))
    res, _ = _result(F, np.zeros(24, f32), 3)
    assert np.isnan(res.rise_time().numpy()).all() and np.isnan(res.fall_time(2.0).numpy()).all()
    assert not res.half_cycles().numpy().any() and not res.mean_range().numpy().any() and not res.damage().numpy().any()
    node, top = res.worst()          # every node ties at 0: node 0
    assert node.tolist() == [0, 0] and top.tolist() == [0.0, 0.0]
    ranges = np.zeros((2, 4, 24), f32)
    ranges[0, 2, [5, 9]] = 7.0
    ranges[1, 2] = np.arange(24)
    res = CyclesResult(reversals=torch.zeros(2, 24, dtype=torch.int32), ranges=torch.from_numpy(ranges), rate_when=None, rates=None,
                       gate=None, exponent=3, T=1)
    node, top = res.worst(include_open=False)
    assert node.tolist() == [5, 23] and top.tolist() == [3.5, 11.5]


def test_a_group_that_was_not_asked_for_is_named():
    F = _histories(5)
    res, _ = _result(F, np.zeros(24, f32), 3, rate_when=None, rates=None)
    for fn in (res.peak_rate, res.rise_time, res.fall_time, res.path_length):
        with pytest.raises(ValueError, match="the rates were not asked for"):
            fn()
    with pytest.raises(ValueError, match="the rates were not asked for"):
        res.rise
    assert res.half_cycles().shape == (2, 24)
    res, _ = _result(F, np.zeros(24, f32), 3, reversals=None, ranges=None)
    for fn in (res.half_cycles, res.mean_range, res.damage, res.worst):
        with pytest.raises(ValueError, match="the turns were not asked for"):
            fn()
    with pytest.raises(ValueError, match="the turns were not asked for"):
        res.open
    assert res.peak_rate().shape == (2, 24)
    with pytest.raises(KeyError):
        CyclesResult()
    assert hasattr(Surrogate, "cycles")


def test_bindings():
    hdr = open(os.path.join(ROOT, "include", "sgvae.h")).read()
    for s in NEW_SYMBOLS:
        assert re.search(rf"\bint {s}\s*\(", hdr), s
        assert s in E.ABI_SYMBOLS
    lib = E.load_library()
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s), s
    assert len(lib.sgv_cycles.argtypes) == 10 and len(lib.sgv_test_recon_cycles.argtypes) == 15
    assert E.MAX_CYCLES_EXPONENT == CR.MAX_EXPONENT == 8 and E.CYCLES_MAX_T == CR.MAX_T == 65535
    assert E.CYCLES_RANGES == CR.RANGES == ("range_sum", "range_max", "damage", "open") and E.CYCLES_RATES == CR.RATES == ("rise", "fall", "path")
    assert [f for f, _ in E.CyclesOut._fields_] == re.findall(r"(\w+);", hdr[hdr.index("typedef struct {\n    int32_t* reversals;"):hdr.index("} sgv_cycles_out;")])
    # without an engine the call is an argument error that says who complains
    assert lib.sgv_cycles(None, None, None, 1, 1, None, None, None, 3, None) == -1 and "sgv_cycles" in lib.sgv_last_error().decode()
    assert lib.sgv_test_recon_cycles(0, None, 8, None, None, None, None, None, None, 3, None, 1, 1, 8, None) == -1
    assert "sgv_test_recon_cycles" in lib.sgv_last_error().decode()
    # the noise follows sgv_set_draw_row, and the header says so
    assert hasattr(E.Engine, "cycles") and "sgv_cycles" in hdr[hdr.index("Noise of a study"):hdr.index("int sgv_set_draw_row")]
