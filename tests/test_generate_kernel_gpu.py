"""The output pass of surrogate prediction alone (csrc/recon_out.hip: recon_phys_*; include/sgvae.h: sgv_test_recon_physical) against
float64:  out[b, t, n] = (tanh(GroupNorm(y)[b, t, n]) - min_n) / scale_n,  layouts [B][T][N] and [B][N][T], fp32 out.

x_hat_ref comes from tests/ew_reference.py (GroupNorm + tanh in float64, as tests/test_ew_kernels_gpu.py uses it); the descale is
restated here in float64.  Groups follow the model's rule G = min(8, max(1, C // 4)).

Bound (derived, not fitted): the element bound tests/test_ew_kernels_gpu.py puts on x_hat stored in fp32 (ELT32 * max|x_hat_ref|),
carried through the division, plus four fp32 roundings (subtraction, reciprocal, product, and one to spare) of the terms of the
subtraction; no bf16 term for either dtype, the output is fp32 and nothing is rounded to the compute dtype on the way:
    tol[b, t, n] = (ELT32 * max|x_hat_ref| + 4 * 2^-24 * (|x_hat_ref| + |min_n|)) / |scale_n|
Measured on an MI355X over all cases: worst err / tol 0.30, at (2, 200, 2080).

Shapes: the five of the issue.  (1, 1, 8) is one row; under the model's rule it has G = 2, Cg = 4.  (3, 5, 40): Cg = 5, a group
boundary inside every 8-channel vector, 5 column vectors on 8 lanes.  (2, 33, 72): Cg = 9, T one past the [B][N][T] kernel's 32-row
tile and C 8 past its 64-channel tile.  (2, 10, 72) with ldy = 80: padded rows.  (2, 200, 2080): the other ew tests' width, several
blocks per sample in both kernels."""
import os
import sys

import numpy as np
import pytest

import simulgen_vae_amd  # noqa: F401
from simulgen_vae_amd import engine as E

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ew_reference as R  # noqa: E402
from recon_kernel_common import CANARY, ELT32, MARGIN, _bf16, _groups, base_inputs, device_inputs, hook_inputs, padding_intact  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 8, 8), (3, 5, 40, 40), (2, 33, 72, 72), (2, 10, 72, 80), (2, 200, 2080, 2080)]     # (B, T, C, ldy)


_CASES = {}


def case(B, T, Cn, dtype):
    """inputs and the float64 reference of one (shape, dtype), computed once"""
    key = (B, T, Cn, dtype)
    if key not in _CASES:
        import torch
        c = base_inputs(B, T, Cn, dtype, signed=False)
        y, gamma, beta, scale, mn = (c[k] for k in ("y", "gamma", "beta", "scale", "mn"))
        if dtype == 1:
            y = _bf16(torch, y)
        xhat = R.gn_forward(y, _groups(Cn), gamma, beta, 2)["out"]
        assert np.abs(xhat).max() > 0.99, "the inputs do not reach tanh's saturation"
        ref = (xhat - mn.astype(np.float64)) / scale.astype(np.float64)
        tol = (ELT32 * np.abs(xhat).max() + 4 * 2.0 ** -24 * (np.abs(xhat) + np.abs(mn.astype(np.float64)))) / np.abs(scale.astype(np.float64))
        _CASES[key] = dict(y=y, gamma=gamma, beta=beta, scale=scale, mn=mn, ref=ref, tol=tol)
    return _CASES[key]


def run(c, B, T, Cn, ldy, dtype, layout):
    """-> (out [B, T, C] float64 in the reference's axis order, raw buffer) after one call of the hook"""
    import torch
    lib = E.load_library()
    d = device_inputs(c, c["y"], ldy, dtype)
    n = B * T * Cn
    buf = torch.full((n + 2 * MARGIN,), CANARY, dtype=torch.float32, device="cuda")
    buf[MARGIN:MARGIN + n] = float("nan")
    out = buf[MARGIN:MARGIN + n]
    assert out.data_ptr() % 16 == 0
    rc = lib.sgv_test_recon_physical(dtype, *hook_inputs(d, ldy), layout, out.data_ptr(), B, T, Cn, None)
    assert rc == 0, lib.sgv_last_error().decode()
    assert bool((buf[:MARGIN] == CANARY).all()) and bool((buf[MARGIN + n:] == CANARY).all()), "the margin around the output was written"
    assert padding_intact(d, Cn), "the padding columns of y were written"
    got = out.double().cpu().numpy()
    got = got.reshape(B, T, Cn) if layout == 0 else got.reshape(B, Cn, T).transpose(0, 2, 1)
    return got, buf.clone()


@pytest.mark.parametrize("layout", [0, 1], ids=["TN", "NT"])
@pytest.mark.parametrize("dtype", [0, 1], ids=["f32", "bf16"])
@pytest.mark.parametrize("B,T,Cn,ldy", SHAPES)
def test_recon_physical_matches_float64(B, T, Cn, ldy, dtype, layout):
    c = case(B, T, Cn, dtype)
    got, raw = run(c, B, T, Cn, ldy, dtype, layout)
    assert np.isfinite(got).all(), "an element of the output was not written"
    err = np.abs(got - c["ref"])
    ratio = err / c["tol"]
    print(f"  (B, T, C, ldy) = {(B, T, Cn, ldy)} dtype {dtype} layout {layout}: max err {err.max():.3e}, max|ref| {np.abs(c['ref']).max():.3e}, "
          f"worst err/tol {ratio.max():.3f}")
    assert np.all(err <= c["tol"]), f"{int((err > c['tol']).sum())} elements off, worst err/tol {ratio.max():.3f} at {np.unravel_index(np.argmax(ratio), err.shape)}"
    # a second launch on the same inputs: bitwise equal (no atomics, no workspace)
    _, raw2 = run(c, B, T, Cn, ldy, dtype, layout)
    import torch
    assert bool((raw.view(torch.int32) == raw2.view(torch.int32)).all()), "two launches differ"


def test_layouts_agree_bitwise():
    """the two layouts are the same numbers in another order"""
    B, T, Cn, ldy = SHAPES[2]
    for dtype in (0, 1):
        c = case(B, T, Cn, dtype)
        a, _ = run(c, B, T, Cn, ldy, dtype, 0)
        b, _ = run(c, B, T, Cn, ldy, dtype, 1)
        assert np.array_equal(a, b)


def test_argument_errors_launch_nothing():
    import torch
    lib = E.load_library()
    B, T, Cn = 2, 3, 16
    y = torch.zeros((B * T, Cn), dtype=torch.float32, device="cuda")
    v = torch.ones(Cn, dtype=torch.float32, device="cuda")
    sums = torch.zeros(B * 4 * 2, dtype=torch.float64, device="cuda")
    out = torch.full((B * T * Cn,), CANARY, dtype=torch.float32, device="cuda")
    good = dict(y=y.data_ptr(), sums=sums.data_ptr(), gamma=v.data_ptr(), beta=v.data_ptr(), scale=v.data_ptr(), mn=v.data_ptr(), out=out.data_ptr())

    def call(layout=0, **kw):
        a = dict(good, **kw)
        return lib.sgv_test_recon_physical(0, a["y"], Cn, a["sums"], a["gamma"], a["beta"], a["scale"], a["mn"], layout, a["out"], B, T, Cn, None)

    for name in good:
        assert call(**{name: None}) == -1, name
        assert "null argument" in lib.sgv_last_error().decode()
    for layout in (2, -1):
        assert call(layout=layout) == -1
        assert "unknown layout" in lib.sgv_last_error().decode()
    assert lib.sgv_test_recon_physical(0, good["y"], Cn, good["sums"], good["gamma"], good["beta"], good["scale"], good["mn"], 0, good["out"] + 4,
                                       B, T, Cn, None) == -1                     # misaligned output
    torch.cuda.synchronize()
    assert bool((out == CANARY).all()), "a rejected call wrote the output"
    assert call() == 0
    assert not bool((out == CANARY).any())
