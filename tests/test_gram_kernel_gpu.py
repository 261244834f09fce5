"""The Gram pass alone (csrc/recon_out.hip: recon_gram_kernel + recon_gram_finish_kernel; include/sgvae.h: sgv_test_recon_gram):
out[b, t, t'] = sum_n w[n] (val[b, t, n] - m[n]) (val[b, t', n] - m[n]) with val = (tanh(GroupNorm(y)) - min_n) / scale_n never
stored.  Inputs, canary-framed buffers and the stored field F -- what the output pass (sgv_test_recon_physical, layout [B][T][N])
writes for the same inputs -- come from tests/recon_kernel_common.py; a quarter of the scales are negative.

Against float64 on F the pass is held to the a-priori bound of an fp32 summation in any order,
|G - G64| <= (C + 3) 2^-24 sum_n |w d_t d_t'| with d the fp32 difference F - m (tests/gram_reference.py); everything else is bit for
bit or exact.

Shapes (B, T, C, ldy).  T = 1, 2: one tile, one pair, three waves without a pair; T = 5: odd; T = 31, 32, 33: a tile edge (33: three
pairs); T = 65: three tiles, six pairs, the pair (0, 2) not adjacent, two waves with two pairs; T = 200: the flagship's 7 tiles and 28
pairs, 7 per wave; T = 256: the limit, 8 tiles, 36 pairs, the 9-accumulator instantiation; T = 257 is refused.  C = 8: half a step,
every upper half past C; C = 72: G = 8 groups of 9 channels, octets straddle groups, a ragged last step; C = 6136, 6144, 6152: one
octet below, at and past a block's 6144-channel share (6152: two shares, the float64 combine runs, the second share is half a step);
the waves of a block split the tile pairs, not the channels, so the step and the block's share are the only edges.  ldy = C and
C + 24 with canary padding columns; B = 1 and 3."""
import os
import sys

import numpy as np
import pytest

import simulgen_vae_amd  # noqa: F401

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gram_reference as GR  # noqa: E402
import recon_kernel_common as H  # noqa: E402
from recon_kernel_common import DTYPES, bits  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = [(1, 1, 8, 8), (3, 2, 8, 32), (3, 5, 72, 72), (1, 31, 72, 96), (3, 32, 8, 8), (3, 33, 72, 96), (1, 65, 72, 72), (3, 65, 8, 32),
         (1, 200, 8, 8), (3, 200, 72, 96), (1, 256, 8, 32), (1, 5, 6136, 6136), (3, 2, 6144, 6168), (1, 33, 6152, 6152),
         (3, 5, 6152, 6176)]          # (B, T, C, ldy)
SMALL = [(1, 1, 8, 8), (3, 5, 72, 72), (3, 33, 72, 96), (3, 65, 8, 32), (3, 200, 72, 96), (1, 256, 8, 32), (3, 2, 6144, 6168), (3, 5, 6152, 6176)]
PASS = H.Pass("gram", lambda b, T, Cn: {"w": (Cn,), "m": (Cn,), "out": (b, T, T)}, ("out",), lambda a: (a["w"], a["m"], a["out"]))


def case(B, T, Cn, ldy, dtype):
    """inputs, the stored field F, weights and an offset of one (shape, dtype), computed once and left alone"""
    return H.case(__name__, B, T, Cn, ldy, dtype, extras=lambda c: {"w": GR.mixed_weights(Cn), "m": GR.mixed_offset(c["F"])})


def launch(c, y, w, m, ldy, dtype):
    """one call of the hook on the samples y [b, T, C] with weights w and offset m ([C] or None) -> out [b, T, T]"""
    return H.launch(PASS, c, y, ldy, dtype, {"w": w, "m": m})["out"]


@DTYPES
@pytest.mark.parametrize("B,T,Cn,ldy", CASES)
def test_gram_is_within_the_bound_of_float64_on_the_stored_field(B, T, Cn, ldy, dtype):
    c = case(B, T, Cn, ldy, dtype)
    first = None
    for name, w, m in (("neither", None, None), ("w", c["w"], None), ("m", None, c["m"]), ("both", c["w"], c["m"])):
        g = launch(c, c["y"], w, m, ldy, dtype)
        assert g.dtype == np.float32 and g.shape == (B, T, T)
        ratio = GR.worst_ratio(g, c["F"], w, m)
        print(f"  B {B} T {T} C {Cn} ldy {ldy} {'bf16' if dtype else 'f32'} {name}: worst err / bound {ratio:.4f}")
        assert ratio <= 1.0
        assert np.array_equal(bits(g), bits(np.swapaxes(g, 1, 2))), "out is bitwise symmetric"
        assert (np.diagonal(g, axis1=1, axis2=2) >= 0).all(), "the diagonal is >= 0 for w >= 0"
        first = first if first is not None else g
    # two launches are bitwise equal
    assert np.array_equal(bits(launch(c, c["y"], None, None, ldy, dtype)), bits(first))


@DTYPES
@pytest.mark.parametrize("B,T,Cn,ldy", SMALL)
def test_one_hot_weights_give_the_single_product_and_zero_weights_give_zero(B, T, Cn, ldy, dtype):
    c = case(B, T, Cn, ldy, dtype)
    F = c["F"]
    for n in sorted({0, Cn - 1, Cn // 2, min(Cn - 1, 9)}):          # the first, the last (a ragged step's lower half), one between, an upper half
        w = np.zeros(Cn, np.float32)
        w[n] = 1.0
        g = launch(c, c["y"], w, None, ldy, dtype)
        want = F[:, :, None, n] * F[:, None, :, n]          # fl(F[t, n] * F[t', n]): one product, one rounding
        assert np.array_equal(bits(g + 0.0), bits(want + 0.0)), n          # + 0.0: a zero of either sign
    assert not launch(c, c["y"], np.zeros(Cn, np.float32), c["m"], ldy, dtype).any(), "w = 0 gives exactly 0"


@DTYPES
@pytest.mark.parametrize("B,T,Cn,ldy", SMALL)
def test_ones_and_zeros_are_the_null_pointers(B, T, Cn, ldy, dtype):
    c = case(B, T, Cn, ldy, dtype)
    one, zero = np.ones(Cn, np.float32), np.zeros(Cn, np.float32)
    assert np.array_equal(bits(launch(c, c["y"], one, zero, ldy, dtype)), bits(launch(c, c["y"], None, None, ldy, dtype)))
    assert np.array_equal(bits(launch(c, c["y"], one, c["m"], ldy, dtype)), bits(launch(c, c["y"], None, c["m"], ldy, dtype)))
    assert np.array_equal(bits(launch(c, c["y"], c["w"], zero, ldy, dtype)), bits(launch(c, c["y"], c["w"], None, ldy, dtype)))


@DTYPES
@pytest.mark.parametrize("T,Cn,ldy", [(2, 8, 32), (5, 72, 72), (33, 72, 96), (65, 8, 32), (200, 72, 96), (2, 6144, 6168), (5, 6152, 6176)])
def test_a_sample_does_not_depend_on_its_batch(T, Cn, ldy, dtype):
    """each sample of B = 3 launched alone, and the last two together, give the bits they have in the batch"""
    c = case(3, T, Cn, ldy, dtype)
    H.assert_batch_independent(lambda y: {"out": launch(c, y, c["w"], c["m"], ldy, dtype)}, c["y"])


def test_the_weight_rides_on_the_smaller_time_index():
    """an asymmetric check of the operand roles: with w that is not a power of two, fl(fl(w d_t) d_t') differs from
    fl(fl(w d_t') d_t) somewhere, and the kept element is the first for t <= t'"""
    Cn = 8
    c = case(3, 32, Cn, 8, 0)
    F = c["F"][:1]
    w = np.zeros(Cn, np.float32)
    w[3] = np.float32(1.0 / 3.0)
    g = launch(c, c["y"][:1], w, None, 8, 0)
    a = (w[3] * F[:, :, 3]).astype(np.float32)
    want = a[:, :, None] * F[:, None, :, 3]
    up = np.triu(np.ones((32, 32), bool))
    want = np.where(up, want, np.swapaxes(want, 1, 2))
    assert np.array_equal(bits(g + 0.0), bits(want + 0.0))
    assert not np.array_equal(bits(want), bits(a[:, None, :] * F[:, :, None, 3])), "the check tells the two roles apart"


def test_rejected_arguments_launch_nothing():
    B, T, Cn, ldy = 3, 5, 72, 96
    c = case(B, T, Cn, ldy, 0)
    d = H.device_inputs(c, c["y"], ldy, 0)
    bufs = H.canary_buffers({"w": Cn + 8, "m": Cn + 8, "out": B * 257 * 257})
    ptr = H.hook_args(d, bufs, ldy, 0, B, T, Cn)
    sub = bufs["out"][1][1:1 + B * T * T]          # out may sit at any 4-byte boundary: the good call has it there, and no w or m
    assert sub.data_ptr() % 16 == 4
    good = dict(ptr, w=None, m=None, out=sub.data_ptr())
    bad = H.common_rejections(good)
    bad += [(dict(out=None), "null argument"), (dict(T=257), "T = 257 is beyond the limit of 256")]
    bad += [(over, "misaligned pointer") for over in (dict(w=ptr["w"] + 4), dict(m=ptr["m"] + 8), dict(out=ptr["out"] + 2))]
    H.reject_all(PASS, d, bufs, good, bad)
    assert np.array_equal(bits(sub.cpu().numpy().reshape(B, T, T)), bits(launch(c, c["y"], None, None, ldy, 0)))
    assert bool((bufs["out"][1][1 + B * T * T:] == 768.0).all()) and float(bufs["out"][1][0]) == 768.0 and H.margins_intact(bufs)
