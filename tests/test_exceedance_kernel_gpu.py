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
import recon_kernel_common as H  # noqa: E402
from recon_kernel_common import DTYPES, bits, same  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = [(1, 1, 8, 8, 1), (3, 2, 8, 32, 4), (3, 5, 72, 72, 3), (3, 33, 72, 96, 4), (1, 5, 504, 504, 4), (3, 33, 512, 536, 3),
         (1, 2, 520, 520, 1), (3, 1, 520, 544, 4), (1, 33, 2040, 2040, 3), (3, 5, 2048, 2072, 4), (1, 1, 2056, 2056, 4),
         (3, 33, 2056, 2080, 3), (1, 2, 2056, 2056, 1)]          # (B, T, C, ldy, L)
SIDES = pytest.mark.parametrize("side", ["above", "below"])
PASS = H.Pass("exceedance", lambda b, T, Cn, n_level, side: {"levels": (n_level, Cn), "stats": (b, 5, n_level, Cn), "excess": (b, n_level, Cn)},
              ("stats", "excess"), lambda a: (a["levels"], a["n_level"], a["side"], a["stats"], a["excess"]), integer=("stats",))


def case(B, T, Cn, ldy, dtype):
    """inputs, the stored field F and the four levels of one (shape, dtype), computed once and left alone"""
    return H.case(__name__, B, T, Cn, ldy, dtype, extras=lambda c: {"levels": XR.kernel_levels(c["F"])})


def pick(levels, L):
    return {1: levels[:1], 3: levels[1:], 4: levels}[L]


def launch(c, y, levels, ldy, dtype, side, want=("stats", "excess")):
    """one call of the hook on the samples y [b, T, C] against levels [L, C] -> {stats [b, 5, L, C], excess [b, L, C]}, those in `want`"""
    res = H.launch(PASS, c, y, ldy, dtype, {"levels": levels}, want=want, n_level=levels.shape[0], side=E.EXCEEDANCE_SIDES[side])
    return {k: res[k] for k in want}


@SIDES
@DTYPES
@pytest.mark.parametrize("B,T,Cn,ldy,L", CASES)
def test_exceedance_equals_the_emulation_on_the_stored_field(B, T, Cn, ldy, L, dtype, side):
    c = case(B, T, Cn, ldy, dtype)
    levels = pick(c["levels"], L)
    got = launch(c, c["y"], levels, ldy, dtype, side)
    stats, excess = got["stats"], got["excess"]
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
    assert not same(launch(c, c["y"], levels, ldy, dtype, side), got)


@SIDES
@DTYPES
@pytest.mark.parametrize("B,T,Cn,ldy", [(3, 5, 72, 72), (3, 33, 512, 536), (3, 1, 520, 544), (3, 33, 2056, 2080), (1, 5, 504, 504)])
def test_a_level_does_not_depend_on_the_other_levels(B, T, Cn, ldy, dtype, side):
    c = case(B, T, Cn, ldy, dtype)
    full = launch(c, c["y"], c["levels"], ldy, dtype, side)
    for sel in ([0], [1], [2], [3], [0, 1], [1, 3], [2, 0], [0, 1, 2], [3, 2, 1], [3, 1, 0, 2], [2, 3, 0, 1]):          # alone, subsets, permutations
        got = launch(c, c["y"], c["levels"][sel], ldy, dtype, side)
        assert not same(got, {"stats": full["stats"][:, :, sel], "excess": full["excess"][:, sel]}), sel


@SIDES
@DTYPES
@pytest.mark.parametrize("T,Cn,ldy,L", [(2, 8, 32, 4), (5, 72, 72, 3), (33, 512, 536, 3), (1, 520, 544, 4), (5, 2048, 2072, 4), (33, 2056, 2080, 3)])
def test_a_sample_does_not_depend_on_its_batch(T, Cn, ldy, L, dtype, side):
    """each sample of B = 3 launched alone, and the last two together, give the bits they have in the batch"""
    c = case(3, T, Cn, ldy, dtype)
    levels = pick(c["levels"], L)
    H.assert_batch_independent(lambda y: launch(c, y, levels, ldy, dtype, side), c["y"])


@SIDES
@DTYPES
@pytest.mark.parametrize("B,T,Cn,ldy,L", [(3, 33, 72, 96, 4), (3, 33, 512, 536, 3), (1, 2, 520, 520, 1), (3, 5, 2048, 2072, 4), (1, 33, 2040, 2040, 3)])
def test_each_output_alone_gives_the_bits_it_gives_with_the_other(B, T, Cn, ldy, L, dtype, side):
    c = case(B, T, Cn, ldy, dtype)
    levels = pick(c["levels"], L)
    both = launch(c, c["y"], levels, ldy, dtype, side)
    for name in PASS.outputs:          # H.launch checks that the other's buffer stays blank
        alone = launch(c, c["y"], levels, ldy, dtype, side, want=(name,))
        assert tuple(alone) == (name,) and not same(alone, {name: both[name]})


def test_rejected_arguments_launch_nothing():
    import torch
    B, T, Cn, ldy, L = 3, 5, 72, 96, 3
    c = case(B, T, Cn, ldy, 0)
    d = H.device_inputs(c, c["y"], ldy, 0)
    bufs = H.canary_buffers(dict(H.sizes(PASS, B, T, Cn, n_level=4, side=0), levels=4 * Cn + 8), integer=PASS.integer)
    levels = pick(c["levels"], L)
    sub = bufs["levels"][1][1:1 + L * Cn]          # the levels may sit at any 4-byte boundary: the good call has them there
    assert sub.data_ptr() % 16 == 4
    sub.copy_(torch.from_numpy(np.array(levels).reshape(-1)).cuda())
    good = dict(H.hook_args(d, bufs, ldy, 0, B, T, Cn, n_level=L, side=0), levels=sub.data_ptr())
    st, ex = good["stats"], good["excess"]
    bad = H.common_rejections(good)
    bad += [(dict(levels=None), "null argument"), (dict(stats=None, excess=None), "no output")]
    bad += [(dict(n_level=v), f"n_level = {v} is outside [1, 4]") for v in (0, 5, -1)]
    bad += [(dict(side=2), "unknown side 2"), (dict(side=-1), "unknown side -1"), (dict(T=65536), "T = 65536 is beyond the limit of 65535 time steps")]
    bad += [(over, "misaligned pointer") for over in (dict(levels=good["levels"] + 2), dict(stats=st + 4), dict(stats=st + 8, excess=None),
                                                      dict(excess=ex + 4), dict(excess=ex + 8, stats=None))]
    H.reject_all(PASS, d, bufs, good, bad)
    assert not same(H.outputs_of(PASS, bufs, B, T, Cn, n_level=L, side=0), launch(c, c["y"], levels, ldy, 0, "above"))
    assert bool((bufs["stats"][1][B * 5 * L * Cn:] == -777).all()) and bool((bufs["excess"][1][B * L * Cn:] == 768.0).all()) and H.margins_intact(bufs)
