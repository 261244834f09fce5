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
from simulgen_vae_amd import engine as E

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import project_reference as PR  # noqa: E402
from recon_kernel_common import _bf16, base_inputs, bits, canary_buffers, device_inputs, field, hook_inputs, margins_intact, padding_intact  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = [(1, 1, 8, 8, 1), (3, 33, 8, 32, 32), (3, 5, 72, 72, 3), (3, 5, 72, 96, 32), (1, 33, 520, 520, 32), (3, 33, 520, 544, 3),
         (1, 5, 1032, 1032, 32), (3, 1, 1032, 1056, 1), (3, 5, 1032, 1032, 3), (1, 1, 4104, 4104, 3)]          # (B, T, C, ldy, R)
DTYPES = pytest.mark.parametrize("dtype", [0, 1], ids=["f32", "bf16"])
SGV_ERR_ARG = -1

_CASES = {}


def case(B, T, Cn, ldy, dtype):
    """inputs and the stored field F of one (shape, dtype), computed once and left alone"""
    import torch
    key = (B, T, Cn, ldy, dtype)
    if key not in _CASES:
        c = base_inputs(B, T, Cn, dtype)
        if dtype == 1:
            c["y"] = _bf16(torch, c["y"])
        c["F"] = field(c, c["y"], ldy, dtype)
        for v in c.values():
            v.setflags(write=False)
        _CASES[key] = c
    return _CASES[key]


def launch(c, y, W, ldy, dtype):
    """one call of the hook on the samples y [b, T, C] with weight rows W [R, C] -> out [b, T, R]; `out` starts as NaN, so every
    element must have been written, and nothing around it"""
    import torch
    lib = E.load_library()
    b, T, Cn = y.shape
    R = W.shape[0]
    d = device_inputs(c, y, ldy, dtype)
    bufs = canary_buffers({"w": R * Cn, "out": b * T * R})
    bufs["w"][1].copy_(torch.from_numpy(np.ascontiguousarray(W, np.float32).reshape(-1)).cuda())
    bufs["out"][1].fill_(float("nan"))
    rc = lib.sgv_test_recon_project(dtype, *hook_inputs(d, ldy), bufs["w"][1].data_ptr(), R, bufs["out"][1].data_ptr(), b, T, Cn, None)
    assert rc == 0, lib.sgv_last_error().decode()
    assert margins_intact(bufs), "a margin around a buffer was written"
    assert padding_intact(d, Cn), "the padding columns of y were written"
    assert np.array_equal(bits(bufs["w"][1].cpu().numpy()), bits(np.ascontiguousarray(W, np.float32).reshape(-1))), "the weights were written"
    out = bufs["out"][1].cpu().numpy().reshape(b, T, R)
    assert np.isfinite(out).all(), "an element of out was not written"
    return out


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
    q = launch(c, c["y"], W, ldy, dtype)
    for b in range(3):
        assert np.array_equal(bits(launch(c, c["y"][b:b + 1], W, ldy, dtype)), bits(q[b:b + 1])), b
    assert np.array_equal(bits(launch(c, c["y"][1:], W, ldy, dtype)), bits(q[1:]))


def test_rejected_arguments_launch_nothing():
    import torch
    lib = E.load_library()
    B, T, Cn, ldy, R = 3, 5, 72, 96, 3
    c = case(B, T, Cn, ldy, 0)
    d = device_inputs(c, c["y"], ldy, 0)
    bufs = canary_buffers({"w": 32 * Cn, "out": B * T * 32})
    w, out = bufs["w"][1].data_ptr(), bufs["out"][1].data_ptr()
    hook = list(hook_inputs(d, ldy))

    def rejected(msg, inputs=None, weights=w, n_func=R, o=out, Bn=B, Tn=T, C_=Cn):
        a = hook if inputs is None else inputs
        assert lib.sgv_test_recon_project(0, *a, weights, n_func, o, Bn, Tn, C_, None) == SGV_ERR_ARG, msg
        assert msg in lib.sgv_last_error().decode(), lib.sgv_last_error().decode()

    for i in (0, 2, 3, 4, 5, 6):          # y, sums, gamma, beta, scale, min
        rejected("null argument", inputs=hook[:i] + [None] + hook[i + 1:])
    rejected("null argument", weights=None)
    rejected("null argument", o=None)
    rejected("n_func = 0 is outside [1, 32]", n_func=0)
    rejected("n_func = 33 is outside [1, 32]", n_func=33)
    rejected("n_func = -1 is outside [1, 32]", n_func=-1)
    rejected("misaligned pointer", weights=w + 4)
    rejected("misaligned pointer", weights=w + 8)
    rejected("misaligned pointer", o=out + 2)
    rejected("misaligned pointer", inputs=[hook[0] + 4] + hook[1:])
    rejected("C % 8 == 0 required", C_=76)
    rejected("C % 8 == 0 required", C_=0)
    rejected("B, T >= 1", Bn=0)
    rejected("B, T >= 1", Tn=0)
    rejected("row stride", inputs=hook[:1] + [64] + hook[2:])
    rejected("row stride", inputs=hook[:1] + [ldy + 4] + hook[2:])
    assert lib.sgv_test_recon_project(2, *hook, w, R, out, B, T, Cn, None) == SGV_ERR_ARG          # an unknown dtype
    torch.cuda.synchronize()
    assert all(bool((buf == buf[0]).all()) for buf, _ in bufs.values()), "a rejected call wrote something"
    assert torch.isnan(d["sums"]).all(), "a rejected call computed the statistics"
    assert padding_intact(d, Cn)
    # and out may sit at any 4-byte boundary
    sub = bufs["out"][1][1:1 + B * T * R]
    assert sub.data_ptr() % 16 == 4
    W = PR.mixed_weights(R, Cn)
    bufs["w"][1][:R * Cn].copy_(torch.from_numpy(W.reshape(-1)).cuda())
    assert lib.sgv_test_recon_project(0, *hook, w, R, sub.data_ptr(), B, T, Cn, None) == 0, lib.sgv_last_error().decode()
    assert np.array_equal(bits(sub.cpu().numpy().reshape(B, T, R)), bits(launch(c, c["y"], W, ldy, 0)))
    assert float(bufs["out"][1][0]) == 768.0 and bool((bufs["out"][1][1 + B * T * R:] == 768.0).all()) and margins_intact(bufs)
