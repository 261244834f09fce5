"""The project pass alone (csrc/recon_out.hip: recon_project_kernel + recon_project_finish_kernel; include/sgvae.h:
sgv_test_recon_project): out[b, t, r] = sum_n W[r, n] val[b, t, n] with val = (tanh(GroupNorm(y)) - min_n) / scale_n never stored.
Inputs, canary-framed buffers and the stored field F -- what the output pass (sgv_test_recon_physical, layout [B][T][N]) writes for the
same inputs -- come from tests/recon_kernel_common.py; a quarter of the scales are negative.

Against float64 on F the pass is held to the a-priori bound of an fp32 summation in any order,
|q - q64| <= (C + 2) 2^-24 sum_n |W[r, n] F[n]| (tests/project_reference.py); everything else is bit for bit or exact.

Shapes (B, T, C, ldy, R).  C = 8: a single octet, the upper half of the only MFMA step past C; C = 72: G = 8 groups of 9 channels, octets
straddle groups; C = 520 and C = 1032: past the 512-node column blocks of the other tails, 1032 also past a wave's 1024-channel share
with a ragged last step; C = 4104: past a block's 4096-channel share, so two partials meet in the float64 combine.  B = 3, T = 5: one
32-row tile spans all three samples; T = 33: a one-row tail in the second tile (B = 1) and a second block of rows (B = 3: 99 rows).
ldy = C and C + 24 with canary padding columns; R = 1, 3 and 32."""
import os
import sys

import numpy as np
import pytest

import simulgen_vae_amd  # noqa: F401

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import project_reference as PR  # noqa: E402
import recon_kernel_common as H  # noqa: E402
from recon_kernel_common import DTYPES, bits  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = [(1, 1, 8, 8, 1), (3, 33, 8, 32, 32), (3, 5, 72, 72, 3), (3, 5, 72, 96, 32), (1, 33, 520, 520, 32), (3, 33, 520, 544, 3),
         (1, 5, 1032, 1032, 32), (3, 1, 1032, 1056, 1), (3, 5, 1032, 1032, 3), (1, 1, 4104, 4104, 3)]          # (B, T, C, ldy, R)
PASS = H.Pass("project", lambda b, T, Cn, n_func: {"w": (n_func, Cn), "out": (b, T, n_func)}, ("out",), lambda a: (a["w"], a["n_func"], a["out"]))


def case(B, T, Cn, ldy, dtype):
    """inputs and the stored field F of one (shape, dtype), computed once and left alone"""
    return H.case(__name__, B, T, Cn, ldy, dtype)


def launch(c, y, W, ldy, dtype):
    """one call of the hook on the samples y [b, T, C] with weight rows W [R, C] -> out [b, T, R]"""
    return H.launch(PASS, c, y, ldy, dtype, {"w": W}, n_func=W.shape[0])["out"]


@DTYPES
@pytest.mark.parametrize("B,T,Cn,ldy,R", CASES)
def test_project_is_within_the_bound_of_float64_on_the_stored_field(B, T, Cn, ldy, R, dtype):
    c = case(B, T, Cn, ldy, dtype)
    W = PR.mixed_weights(R, Cn)
    q = launch(c, c["y"], W, ldy, dtype)
    assert q.dtype == np.float32 and q.shape == (B, T, R)
    ratio = PR.worst_ratio(q, c["F"], W)
    print(f"  B {B} T {T} C {Cn} ldy {ldy} R {R} {'bf16' if dtype else 'f32'}: worst err / bound {ratio:.4f}")
    assert ratio <= 1.0
    # two launches are bitwise equal
    assert np.array_equal(bits(launch(c, c["y"], W, ldy, dtype)), bits(q))


@DTYPES
@pytest.mark.parametrize("B,T,Cn,ldy", [(3, 5, 72, 96), (3, 33, 520, 544), (1, 5, 1032, 1032), (1, 1, 4104, 4104), (1, 1, 8, 8)])
def test_one_hot_rows_pick_their_node_and_zero_rows_give_zero(B, T, Cn, ldy, dtype):
    c = case(B, T, Cn, ldy, dtype)
    nodes = [0, Cn - 1, Cn - 5]          # the first, the last, and one more of the ragged last block (C = 8: node 3)
    W = np.zeros((32, Cn), np.float32)
    for k, n in enumerate(nodes):
        W[k, n] = 1.0
    W[31, Cn // 2] = -2.0
    q = launch(c, c["y"], W, ldy, dtype)
    for k, n in enumerate(nodes):
        assert np.array_equal(q[:, :, k], c["F"][:, :, n]), (k, n)
    assert np.array_equal(q[:, :, 31], -2.0 * c["F"][:, :, Cn // 2])
    assert not q[:, :, 3:31].any(), "an all-zero row is exactly 0"
    # a single all-zero row
    assert not launch(c, c["y"], np.zeros((1, Cn), np.float32), ldy, dtype).any()


@DTYPES
@pytest.mark.parametrize("B,T,Cn,ldy", [(3, 5, 72, 96), (3, 33, 520, 544), (3, 5, 1032, 1032), (1, 1, 4104, 4104)])
def test_a_row_does_not_depend_on_the_other_rows(B, T, Cn, ldy, dtype):
    c = case(B, T, Cn, ldy, dtype)
    W = PR.mixed_weights(32, Cn)
    q = launch(c, c["y"], W, ldy, dtype)
    for r in (0, 17, 31):          # alone, R = 1
        assert np.array_equal(bits(launch(c, c["y"], W[r:r + 1], ldy, dtype)[:, :, 0]), bits(q[:, :, r])), r
    assert np.array_equal(bits(launch(c, c["y"], W[5:8], ldy, dtype)), bits(q[:, :, 5:8]))          # R = 3
    perm = np.random.default_rng(2).permutation(32)
    assert np.array_equal(bits(launch(c, c["y"], W[perm], ldy, dtype)), bits(q[:, :, perm]))


@DTYPES
@pytest.mark.parametrize("T,Cn,ldy,R", [(5, 72, 96, 32), (33, 520, 544, 3), (1, 1032, 1056, 1), (5, 1032, 1032, 3), (33, 8, 32, 32)])
def test_a_sample_does_not_depend_on_its_batch(T, Cn, ldy, R, dtype):
    """B = 3: row tiles span samples (T = 5: all three in one tile); each sample launched alone gives the bits of its rows"""
    c = case(3, T, Cn, ldy, dtype)
    W = PR.mixed_weights(R, Cn)
    H.assert_batch_independent(lambda y: {"out": launch(c, y, W, ldy, dtype)}, c["y"])


def test_rejected_arguments_launch_nothing():
    import torch
    B, T, Cn, ldy, R = 3, 5, 72, 96, 3
    c = case(B, T, Cn, ldy, 0)
    d = H.device_inputs(c, c["y"], ldy, 0)
    bufs = H.canary_buffers({"w": 32 * Cn, "out": B * T * 32})
    W = PR.mixed_weights(R, Cn)
    bufs["w"][1][:R * Cn].copy_(torch.from_numpy(W.reshape(-1)).cuda())
    sub = bufs["out"][1][1:1 + B * T * R]          # out may sit at any 4-byte boundary: the good call has it there
    assert sub.data_ptr() % 16 == 4
    ptr = H.hook_args(d, bufs, ldy, 0, B, T, Cn, n_func=R)
    good = dict(ptr, out=sub.data_ptr())
    bad = H.common_rejections(good)
    bad += [(dict(w=None), "null argument"), (dict(out=None), "null argument")]
    bad += [(dict(n_func=v), f"n_func = {v} is outside [1, 32]") for v in (0, 33, -1)]
    bad += [(over, "misaligned pointer") for over in (dict(w=ptr["w"] + 4), dict(w=ptr["w"] + 8), dict(out=ptr["out"] + 2))]
    H.reject_all(PASS, d, bufs, good, bad)
    assert np.array_equal(bits(sub.cpu().numpy().reshape(B, T, R)), bits(launch(c, c["y"], W, ldy, 0)))
    assert float(bufs["out"][1][0]) == 768.0 and bool((bufs["out"][1][1 + B * T * R:] == 768.0).all()) and H.margins_intact(bufs)
