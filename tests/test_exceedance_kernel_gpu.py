"""The exceedance pass alone (csrc/recon_out.hip: recon_exceed_kernel; include/sgvae.h: sgv_test_recon_exceedance): the level-crossing
statistics over time of val = (tanh(GroupNorm(y)) - min_n) / scale_n, never stored, against L levels per channel.  Inputs,
canary-framed buffers and the stored field F -- what the output pass (sgv_test_recon_physical, layout [B][T][N]) writes for the same
inputs -- come from tests/recon_kernel_common.py; a quarter of the scales are negative.

All six outputs are held to the numpy emulation on F (tests/exceedance_reference.py) bit for bit, for both sides and both dtypes; the
excess also to float64 within the a-priori bound (T + 1) 2^-24 sum_t |d[t]|.  No other tolerance anywhere.

Shapes (B, T, C, ldy, L).  T = 1, 2, 5; T = 33: longer than the ring of loads in flight (4 steps in bf16, 2 in fp32).  C = 8: a single
octet, one thread; C = 72: G = 8 groups of 9 channels, octets straddle groups; C = 504, 512, 520: one octet below, at and past a wave's
512-channel share; C = 2040, 2048, 2056: the same around a block's 2048-channel share.  ldy = C and C + 24 with canary padding columns;
B = 1 and 3; L = 1, 3 and 4.

Levels (exceedance_reference.kernel_levels, from F): the per-node median (many runs), a stored element itself (the strict tie), the
node's maximum (never exceeded above) and nextafter(the node's minimum, -inf) (always exceeded above).  L = 1 takes the first, L = 3
the last three."""
import os
import sys

import numpy as np
import pytest

import simulgen_vae_amd  # noqa: F401
from simulgen_vae_amd import engine as E

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exceedance_reference as XR  # noqa: E402
from recon_kernel_common import _bf16, base_inputs, bits, canary_buffers, device_inputs, field, hook_inputs, margins_intact, padding_intact  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = [(1, 1, 8, 8, 1), (3, 2, 8, 32, 4), (3, 5, 72, 72, 3), (3, 33, 72, 96, 4), (1, 5, 504, 504, 4), (3, 33, 512, 536, 3),
         (1, 2, 520, 520, 1), (3, 1, 520, 544, 4), (1, 33, 2040, 2040, 3), (3, 5, 2048, 2072, 4), (1, 1, 2056, 2056, 4),
         (3, 33, 2056, 2080, 3), (1, 2, 2056, 2056, 1)]          # (B, T, C, ldy, L)
DTYPES = pytest.mark.parametrize("dtype", [0, 1], ids=["f32", "bf16"])
SIDES = pytest.mark.parametrize("side", ["above", "below"])
SGV_ERR_ARG = -1
UNWRITTEN = -999          # no statistic is below -1

_CASES = {}


def case(B, T, Cn, ldy, dtype):
    """inputs, the stored field F and the four levels of one (shape, dtype), computed once and left alone"""
    import torch
    key = (B, T, Cn, ldy, dtype)
    if key not in _CASES:
        c = base_inputs(B, T, Cn, dtype)
        if dtype == 1:
            c["y"] = _bf16(torch, c["y"])
        c["F"] = field(c, c["y"], ldy, dtype)
        c["levels"] = XR.kernel_levels(c["F"])
        for v in c.values():
            v.setflags(write=False)
        _CASES[key] = c
    return _CASES[key]


def pick(levels, L):
    return {1: levels[:1], 3: levels[1:], 4: levels}[L]


def launch(c, y, levels, ldy, dtype, side, want=("stats", "excess")):
    """one call of the hook on the samples y [b, T, C] against levels [L, C] -> (stats [b, 5, L, C] or None, excess [b, L, C] or None);
    the outputs start as -999 / NaN, so every element must have been written, and nothing around them"""
    import torch
    lib = E.load_library()
    b, T, Cn = y.shape
    L = levels.shape[0]
    lv = np.array(levels, np.float32).reshape(-1)          # a writable copy
    d = device_inputs(c, y, ldy, dtype)
    bufs = canary_buffers({"levels": L * Cn, "stats": b * 5 * L * Cn, "excess": b * L * Cn}, integer=("stats",))
    bufs["levels"][1].copy_(torch.from_numpy(lv).cuda())
    bufs["stats"][1].fill_(UNWRITTEN)
    bufs["excess"][1].fill_(float("nan"))
    rc = lib.sgv_test_recon_exceedance(dtype, *hook_inputs(d, ldy), bufs["levels"][1].data_ptr(), L, E.EXCEEDANCE_SIDES[side],
                                       bufs["stats"][1].data_ptr() if "stats" in want else None,
                                       bufs["excess"][1].data_ptr() if "excess" in want else None, b, T, Cn, None)
    assert rc == 0, lib.sgv_last_error().decode()
    assert margins_intact(bufs), "a margin around a buffer was written"
    assert padding_intact(d, Cn), "the padding columns of y were written"
    assert np.array_equal(bits(bufs["levels"][1].cpu().numpy()), bits(lv)), "the levels were written"
    stats = bufs["stats"][1].cpu().numpy().reshape(b, 5, L, Cn)
    excess = bufs["excess"][1].cpu().numpy().reshape(b, L, Cn)
    if "stats" in want:
        assert (stats != UNWRITTEN).all(), "an element of stats was not written"
    else:
        assert (stats == UNWRITTEN).all(), "stats was written although it was not asked for"
    if "excess" in want:
        assert np.isfinite(excess).all(), "an element of excess was not written"
    else:
        assert np.isnan(excess).all(), "excess was written although it was not asked for"
    return (stats if "stats" in want else None), (excess if "excess" in want else None)


def same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1]))


@SIDES
@DTYPES
@pytest.mark.parametrize("B,T,Cn,ldy,L", CASES)
def test_exceedance_equals_the_emulation_on_the_stored_field(B, T, Cn, ldy, L, dtype, side):
    c = case(B, T, Cn, ldy, dtype)
    levels = pick(c["levels"], L)
    stats, excess = launch(c, c["y"], levels, ldy, dtype, side)
    assert stats.dtype == np.int32 and stats.shape == (B, 5, L, Cn) and excess.dtype == np.float32 and excess.shape == (B, L, Cn)
    want_stats, want_excess = XR.emulate(c["F"], levels, side)
    for k, name in enumerate(XR.STATS):
        assert np.array_equal(stats[:, k], want_stats[:, k]), name
    assert np.array_equal(bits(excess), bits(want_excess)), "excess"
    ratio = XR.worst_ratio(excess, c["F"], levels, side)
    print(f"  B {B} T {T} C {Cn} ldy {ldy} L {L} {'bf16' if dtype else 'f32'} {side}: worst excess err / bound {ratio:.4f}")
    assert ratio <= 1.0
    # what the levels were chosen for
    count, first, last, longest, runs = (stats[:, k] for k in range(5))
    if L >= 3:
        tie, top, low = L - 3, L - 2, L - 1
        assert (c["F"][0, T // 2] == levels[tie]).all() and not XR.exceeds(c["F"], levels, side)[0, T // 2, tie].any()          # the strict tie
        if side == "above":
            assert not count[:, top].any() and (first[:, top] == -1).all() and (last[:, top] == -1).all() and not longest[:, top].any()
            assert not runs[:, top].any() and np.array_equal(bits(excess[:, top]), np.zeros((B, Cn), np.int32))          # exactly +0.0
            assert (count[:, low] == T).all() and (longest[:, low] == T).all() and (runs[:, low] == 1).all()
            assert (first[:, low] == 0).all() and (last[:, low] == T - 1).all()
        else:
            assert not count[:, low].any() and np.array_equal(bits(excess[:, low]), np.zeros((B, Cn), np.int32))
    if L != 3 and T == 33:
        assert (runs[:, 0] > 3).any(), "the median gives many runs"
    # two launches are bitwise equal
    assert same(launch(c, c["y"], levels, ldy, dtype, side), (stats, excess))


@SIDES
@DTYPES
@pytest.mark.parametrize("B,T,Cn,ldy", [(3, 5, 72, 72), (3, 33, 512, 536), (3, 1, 520, 544), (3, 33, 2056, 2080), (1, 5, 504, 504)])
def test_a_level_does_not_depend_on_the_other_levels(B, T, Cn, ldy, dtype, side):
    c = case(B, T, Cn, ldy, dtype)
    stats, excess = launch(c, c["y"], c["levels"], ldy, dtype, side)
    for sel in ([0], [1], [2], [3], [0, 1], [1, 3], [2, 0], [0, 1, 2], [3, 2, 1], [3, 1, 0, 2], [2, 3, 0, 1]):          # alone, subsets, permutations
        st, ex = launch(c, c["y"], c["levels"][sel], ldy, dtype, side)
        assert np.array_equal(st, stats[:, :, sel]) and np.array_equal(bits(ex), bits(excess[:, sel])), sel


@SIDES
@DTYPES
@pytest.mark.parametrize("T,Cn,ldy,L", [(2, 8, 32, 4), (5, 72, 72, 3), (33, 512, 536, 3), (1, 520, 544, 4), (5, 2048, 2072, 4), (33, 2056, 2080, 3)])
def test_a_sample_does_not_depend_on_its_batch(T, Cn, ldy, L, dtype, side):
    """each sample of B = 3 launched alone, and the last two together, give the bits they have in the batch"""
    c = case(3, T, Cn, ldy, dtype)
    levels = pick(c["levels"], L)
    stats, excess = launch(c, c["y"], levels, ldy, dtype, side)
    for b in range(3):
        assert same(launch(c, c["y"][b:b + 1], levels, ldy, dtype, side), (stats[b:b + 1], excess[b:b + 1])), b
    assert same(launch(c, c["y"][1:], levels, ldy, dtype, side), (stats[1:], excess[1:]))


@SIDES
@DTYPES
@pytest.mark.parametrize("B,T,Cn,ldy,L", [(3, 33, 72, 96, 4), (3, 33, 512, 536, 3), (1, 2, 520, 520, 1), (3, 5, 2048, 2072, 4), (1, 33, 2040, 2040, 3)])
def test_each_output_alone_gives_the_bits_it_gives_with_the_other(B, T, Cn, ldy, L, dtype, side):
    c = case(B, T, Cn, ldy, dtype)
    levels = pick(c["levels"], L)
    stats, excess = launch(c, c["y"], levels, ldy, dtype, side)
    st, none = launch(c, c["y"], levels, ldy, dtype, side, want=("stats",))
    assert none is None and np.array_equal(st, stats)
    none, ex = launch(c, c["y"], levels, ldy, dtype, side, want=("excess",))
    assert none is None and np.array_equal(bits(ex), bits(excess))


def test_rejected_arguments_launch_nothing():
    import torch
    lib = E.load_library()
    B, T, Cn, ldy, L = 3, 5, 72, 96, 3
    c = case(B, T, Cn, ldy, 0)
    d = device_inputs(c, c["y"], ldy, 0)
    bufs = canary_buffers({"levels": 4 * Cn + 8, "stats": B * 5 * 4 * Cn, "excess": B * 4 * Cn}, integer=("stats",))
    lv, st, ex = (bufs[k][1].data_ptr() for k in ("levels", "stats", "excess"))
    hook = list(hook_inputs(d, ldy))

    def rejected(msg, inputs=None, levels=lv, n_level=L, side=0, stats=st, excess=ex, Bn=B, Tn=T, C_=Cn):
        a = hook if inputs is None else inputs
        assert lib.sgv_test_recon_exceedance(0, *a, levels, n_level, side, stats, excess, Bn, Tn, C_, None) == SGV_ERR_ARG, msg
        assert msg in lib.sgv_last_error().decode(), lib.sgv_last_error().decode()

    for i in (0, 2, 3, 4, 5, 6):          # y, sums, gamma, beta, scale, min
        rejected("null argument", inputs=hook[:i] + [None] + hook[i + 1:])
    rejected("null argument", levels=None)
    rejected("no output", stats=None, excess=None)
    rejected("n_level = 0 is outside [1, 4]", n_level=0)
    rejected("n_level = 5 is outside [1, 4]", n_level=5)
    rejected("n_level = -1 is outside [1, 4]", n_level=-1)
    rejected("unknown side 2", side=2)
    rejected("unknown side -1", side=-1)
    rejected("T = 65536 is beyond the limit of 65535 time steps", Tn=65536)
    rejected("misaligned pointer", levels=lv + 2)
    rejected("misaligned pointer", stats=st + 4)
    rejected("misaligned pointer", stats=st + 8, excess=None)
    rejected("misaligned pointer", excess=ex + 4)
    rejected("misaligned pointer", excess=ex + 8, stats=None)
    rejected("misaligned pointer", inputs=[hook[0] + 4] + hook[1:])
    rejected("C % 8 == 0 required", C_=76)
    rejected("C % 8 == 0 required", C_=0)
    rejected("B, T >= 1", Bn=0)
    rejected("B, T >= 1", Tn=0)
    rejected("row stride", inputs=hook[:1] + [64] + hook[2:])
    rejected("row stride", inputs=hook[:1] + [ldy + 4] + hook[2:])
    assert lib.sgv_test_recon_exceedance(2, *hook, lv, L, 0, st, ex, B, T, Cn, None) == SGV_ERR_ARG          # an unknown dtype
    torch.cuda.synchronize()
    assert all(bool((buf == buf[0]).all()) for buf, _ in bufs.values()), "a rejected call wrote something"
    assert torch.isnan(d["sums"]).all(), "a rejected call computed the statistics"
    assert padding_intact(d, Cn)
    # and the levels may sit at any 4-byte boundary
    levels = pick(c["levels"], L)
    sub = bufs["levels"][1][1:1 + L * Cn]
    assert sub.data_ptr() % 16 == 4
    sub.copy_(torch.from_numpy(np.array(levels).reshape(-1)).cuda())
    s, e = bufs["stats"][1][:B * 5 * L * Cn], bufs["excess"][1][:B * L * Cn]
    assert lib.sgv_test_recon_exceedance(0, *hook, sub.data_ptr(), L, 0, s.data_ptr(), e.data_ptr(), B, T, Cn, None) == 0, lib.sgv_last_error().decode()
    want = launch(c, c["y"], levels, ldy, 0, "above")
    assert same((s.cpu().numpy().reshape(B, 5, L, Cn), e.cpu().numpy().reshape(B, L, Cn)), want)
    assert bool((bufs["stats"][1][B * 5 * L * Cn:] == -777).all()) and bool((bufs["excess"][1][B * L * Cn:] == 768.0).all()) and margins_intact(bufs)
