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
blocks per sample in both kernels.

The pass is the harness's own FIELD (tests/recon_kernel_common.py), the reference of the other eleven files; here it has no stored
field to lean on, so the cases carry none (ldy None) and positive scales."""
import os
import sys

import numpy as np
import pytest

import simulgen_vae_amd  # noqa: F401

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ew_reference as R  # noqa: E402
import recon_kernel_common as H  # noqa: E402
from recon_kernel_common import CANARY, DTYPES, ELT32, _groups, bits  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 8, 8), (3, 5, 40, 40), (2, 33, 72, 72), (2, 10, 72, 80), (2, 200, 2080, 2080)]     # (B, T, C, ldy)


def reference(c):
    xhat = R.gn_forward(c["y"], _groups(c["y"].shape[2]), c["gamma"], c["beta"], 2)["out"]
    assert np.abs(xhat).max() > 0.99, "the inputs do not reach tanh's saturation"
    mn64, sc64 = c["mn"].astype(np.float64), c["scale"].astype(np.float64)
    return {"ref": (xhat - mn64) / sc64, "tol": (ELT32 * np.abs(xhat).max() + 4 * 2.0 ** -24 * (np.abs(xhat) + np.abs(mn64))) / np.abs(sc64)}


def case(B, T, Cn, dtype):
    """inputs and the float64 reference of one (shape, dtype), computed once"""
    return H.case(__name__, B, T, Cn, None, dtype, extras=reference, signed=False)


def run(c, ldy, dtype, layout):
    """-> out [B, T, C] fp32 in the reference's axis order after one call of the hook"""
    out = H.launch(H.FIELD, c, c["y"], ldy, dtype, layout=layout)["out"]
    return out if layout == 0 else out.transpose(0, 2, 1)


@pytest.mark.parametrize("layout", [0, 1], ids=["TN", "NT"])
@DTYPES
@pytest.mark.parametrize("B,T,Cn,ldy", SHAPES)
def test_recon_physical_matches_float64(B, T, Cn, ldy, dtype, layout):
    c = case(B, T, Cn, dtype)
    got = run(c, ldy, dtype, layout)
    assert np.isfinite(got).all(), "an element of the output was not written"
    err = np.abs(got - c["ref"])
    ratio = err / c["tol"]
    print(f"  (B, T, C, ldy) = {(B, T, Cn, ldy)} dtype {dtype} layout {layout}: max err {err.max():.3e}, max|ref| {np.abs(c['ref']).max():.3e}, "
          f"worst err/tol {ratio.max():.3f}")
    assert np.all(err <= c["tol"]), f"{int((err > c['tol']).sum())} elements off, worst err/tol {ratio.max():.3f} at {np.unravel_index(np.argmax(ratio), err.shape)}"
    # a second launch on the same inputs: bitwise equal (no atomics, no workspace)
    assert np.array_equal(bits(run(c, ldy, dtype, layout)), bits(got)), "two launches differ"


def test_layouts_agree_bitwise():
    """the two layouts are the same numbers in another order"""
    B, T, Cn, ldy = SHAPES[2]
    for dtype in (0, 1):
        c = case(B, T, Cn, dtype)
        assert np.array_equal(run(c, ldy, dtype, 0), run(c, ldy, dtype, 1))


def test_argument_errors_launch_nothing():
    B, T, Cn = 2, 3, 16
    c = H.inputs(B, T, Cn, 0, signed=False)
    d = H.device_inputs(c, c["y"], Cn, 0)
    bufs = H.canary_buffers(H.sizes(H.FIELD, B, T, Cn, layout=0))
    good = H.hook_args(d, bufs, Cn, 0, B, T, Cn, layout=0)
    bad = H.common_rejections(good) + [(dict(out=None), "null argument"), (dict(layout=2), "unknown layout"), (dict(layout=-1), "unknown layout")]
    bad += [(dict(out=good["out"] + 4), "out must be 16-byte aligned")]
    H.reject_all(H.FIELD, d, bufs, good, bad)
    assert not bool((bufs["out"][1] == CANARY).any()) and H.margins_intact(bufs)
