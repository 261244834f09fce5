"""The temporal pass alone (csrc/recon_out.hip: recon_temporal_weights_kernel + recon_temporal_kernel; include/sgvae.h:
sgv_test_recon_temporal): out[b, r, n] = sum_t W[r, t] val[b, t, n] with val = (tanh(GroupNorm(y)) - min_n) / scale_n never stored.
Inputs, canary-framed buffers and the stored field F -- what the output pass (sgv_test_recon_physical, layout [B][T][N]) writes for the
same inputs -- come from tests/recon_kernel_common.py; a quarter of the scales are negative.

Against float64 on F the pass is held to the a-priori bound of an fp32 summation in any order,
|q - q64| <= (T + 2) 2^-24 sum_t |W[r, t] F[t, n]| (tests/temporal_reference.py); everything else is bit for bit or exact.

Shapes (B, T, C, ldy, R).  T = 1: the upper half of the only MFMA step is past T; T = 2: one full step; T = 5: odd, a ragged last
step; T = 33: odd, 17 steps, more than are kept in flight (8 in bf16, 4 in fp32).  C = 8: a single octet, every other lane past C;
C = 72: G = 8 groups of 9 channels, octets straddle groups; C = 248, 256, 264: one octet below, at and past a wave's 256-channel
share; C = 1016, 1024, 1032: the same around a block's 1024-channel share.  ldy = C and C + 24 with canary padding columns; B = 1
and 3; R = 1, 3 and 32."""
import os
import sys

import numpy as np
import pytest

import simulgen_vae_amd  # noqa: F401

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import temporal_reference as TR  # noqa: E402
import recon_kernel_common as H  # noqa: E402
from recon_kernel_common import DTYPES, bits  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = [(1, 1, 8, 8, 1), (3, 2, 8, 32, 32), (3, 5, 72, 72, 3), (3, 33, 72, 96, 32), (1, 5, 248, 248, 32), (3, 33, 256, 280, 3),
         (1, 2, 264, 264, 1), (3, 1, 264, 288, 32), (1, 33, 1016, 1016, 3), (3, 5, 1024, 1048, 32), (1, 1, 1032, 1032, 32),
         (3, 33, 1032, 1056, 3), (1, 2, 1032, 1032, 1)]          # (B, T, C, ldy, R)
PASS = H.Pass("temporal", lambda b, T, Cn, n_func: {"w": (n_func, T), "out": (b, n_func, Cn)}, ("out",), lambda a: (a["w"], a["n_func"], a["out"]))


def case(B, T, Cn, ldy, dtype):
    """inputs and the stored field F of one (shape, dtype), computed once and left alone"""
    return H.case(__name__, B, T, Cn, ldy, dtype)


def launch(c, y, W, ldy, dtype):
    """one call of the hook on the samples y [b, T, C] with weight rows W [R, T] -> out [b, R, C]"""
    return H.launch(PASS, c, y, ldy, dtype, {"w": W}, n_func=W.shape[0])["out"]


@DTYPES
@pytest.mark.parametrize("B,T,Cn,ldy,R", CASES)
def test_temporal_is_within_the_bound_of_float64_on_the_stored_field(B, T, Cn, ldy, R, dtype):
    c = case(B, T, Cn, ldy, dtype)
    W = TR.mixed_weights(R, T)
    q = launch(c, c["y"], W, ldy, dtype)
    assert q.dtype == np.float32 and q.shape == (B, R, Cn)
    ratio = TR.worst_ratio(q, c["F"], W)
    print(f"  B {B} T {T} C {Cn} ldy {ldy} R {R} {'bf16' if dtype else 'f32'}: worst err / bound {ratio:.4f}")
    assert ratio <= 1.0
    # two launches are bitwise equal
    assert np.array_equal(bits(launch(c, c["y"], W, ldy, dtype)), bits(q))


@DTYPES
@pytest.mark.parametrize("B,T,Cn,ldy", [(1, 1, 8, 8), (3, 5, 72, 72), (3, 33, 256, 280), (3, 1, 264, 288), (1, 33, 1016, 1016), (3, 33, 1032, 1056),
                                        (1, 2, 1032, 1032)])
def test_one_hot_rows_pick_their_time_step_and_zero_rows_give_zero(B, T, Cn, ldy, dtype):
    c = case(B, T, Cn, ldy, dtype)
    steps = [0, T - 1, T // 2]          # the first, the last (odd T: the lower half of the ragged step), one between
    W = np.zeros((32, T), np.float32)
    for k, t in enumerate(steps):
        W[k, t] = 1.0
    W[31, T // 3] = -2.0
    q = launch(c, c["y"], W, ldy, dtype)
    for k, t in enumerate(steps):
        assert np.array_equal(bits(q[:, k] + 0.0), bits(c["F"][:, t] + 0.0)), (k, t)          # + 0.0: a zero of either sign
    assert np.array_equal(q[:, 31], -2.0 * c["F"][:, T // 3])
    assert not q[:, 3:31].any(), "an all-zero row is exactly 0"
    # a single all-zero row
    assert not launch(c, c["y"], np.zeros((1, T), np.float32), ldy, dtype).any()


@DTYPES
@pytest.mark.parametrize("B,T,Cn,ldy", [(3, 5, 72, 72), (3, 33, 256, 280), (3, 1, 264, 288), (3, 33, 1032, 1056), (1, 5, 248, 248)])
def test_a_row_does_not_depend_on_the_other_rows(B, T, Cn, ldy, dtype):
    c = case(B, T, Cn, ldy, dtype)
    W = TR.mixed_weights(32, T)
    q = launch(c, c["y"], W, ldy, dtype)
    for r in (0, 17, 31):          # alone, R = 1
        assert np.array_equal(bits(launch(c, c["y"], W[r:r + 1], ldy, dtype)[:, 0]), bits(q[:, r])), r
    assert np.array_equal(bits(launch(c, c["y"], W[5:8], ldy, dtype)), bits(q[:, 5:8]))          # R = 3
    perm = np.random.default_rng(2).permutation(32)
    assert np.array_equal(bits(launch(c, c["y"], W[perm], ldy, dtype)), bits(q[:, perm]))


@DTYPES
@pytest.mark.parametrize("T,Cn,ldy,R", [(2, 8, 32, 32), (5, 72, 72, 3), (33, 256, 280, 3), (1, 264, 288, 32), (5, 1024, 1048, 32), (33, 1032, 1056, 3)])
def test_a_sample_does_not_depend_on_its_batch(T, Cn, ldy, R, dtype):
    """each sample of B = 3 launched alone, and the last two together, give the bits they have in the batch"""
    c = case(3, T, Cn, ldy, dtype)
    W = TR.mixed_weights(R, T)
    H.assert_batch_independent(lambda y: {"out": launch(c, y, W, ldy, dtype)}, c["y"])


def test_rejected_arguments_launch_nothing():
    import torch
    B, T, Cn, ldy, R = 3, 5, 72, 96, 3
    c = case(B, T, Cn, ldy, 0)
    d = H.device_inputs(c, c["y"], ldy, 0)
    bufs = H.canary_buffers({"w": 32 * T + 8, "out": B * 32 * Cn})
    W = TR.mixed_weights(R, T)
    sub = bufs["w"][1][1:1 + R * T]          # the weights may sit at any 4-byte boundary: the good call has them there
    assert sub.data_ptr() % 16 == 4
    sub.copy_(torch.from_numpy(W.reshape(-1)).cuda())
    good = dict(H.hook_args(d, bufs, ldy, 0, B, T, Cn, n_func=R), w=sub.data_ptr())
    bad = H.common_rejections(good)
    bad += [(dict(w=None), "null argument"), (dict(out=None), "null argument")]
    bad += [(dict(n_func=v), f"n_func = {v} is outside [1, 32]") for v in (0, 33, -1)]
    bad += [(over, "misaligned pointer") for over in (dict(w=good["w"] + 2), dict(out=good["out"] + 4), dict(out=good["out"] + 8))]
    H.reject_all(PASS, d, bufs, good, bad)
    assert np.array_equal(bits(H.outputs_of(PASS, bufs, B, T, Cn, n_func=R)["out"]), bits(launch(c, c["y"], W, ldy, 0)))
    assert bool((bufs["out"][1][B * R * Cn:] == 768.0).all()) and H.margins_intact(bufs)
