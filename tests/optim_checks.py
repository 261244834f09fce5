"""Shared input generators, comparison helpers and derived error bounds of the float64 kernel tests of the optimizer kernels:
tests/test_optim_kernels_gpu.py (csrc/optim.hip through the sgv_test_optset_* hook) and tests/test_lc_param_ops_gpu.py (the
parameter side of include/sgvae_ops.h).  The derivations are in the module docstring of tests/test_optim_kernels_gpu.py; each
bound is one function here, so both tests assert exactly the same thing.  No GPU is touched."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ew_reference as R  # noqa: E402
import optim_reference as O  # noqa: E402

U = 2.0 ** -24          # the largest relative error of one correctly rounded fp32 operation
FLOOR = 2.0 ** -22
TINY = 1e-300
B1, B2, EPS = float(np.float32(0.9)), float(np.float32(0.999)), float(np.float32(1e-8))
LR = float(np.float32(1e-3))


def mags(rng, shape, scale=1.0):
    """random signs, magnitudes in [0.25, 1] x scale, fp32"""
    return (rng.choice([-1.0, 1.0], shape) * rng.uniform(0.25, 1.0, shape) * scale).astype(np.float32)


def same(a, b):
    import torch
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def red_tol(measured):
    return max(4.0 * measured, FLOOR)


def check_abs(got, ref, tol, what):
    ref = np.asarray(ref, np.float64)
    got = np.asarray(got, np.float64).reshape(ref.shape)
    tol = np.broadcast_to(np.asarray(tol, np.float64), ref.shape)
    assert np.isfinite(got).all(), f"{what}: non-finite output (an element was not written?)"
    err = np.abs(got - ref)
    worst = np.max(err / np.maximum(tol, TINY)) if err.size else 0.0
    print(f"  {what}: max err {err.max():.3e}, max|ref| {np.abs(ref).max():.3e}, worst err/tol {worst:.3f}")
    assert np.all(err <= tol), f"{what}: {int((err > tol).sum())} elements off, worst err/tol {worst:.3g} at {np.unravel_index(np.argmax(err - tol), ref.shape)}"


def check_red(got, ref, mag, measured, what, extra=0.0):
    tol = red_tol(measured)
    print(f"  {what}: tolerance {tol:.3e} of the sum of magnitudes (float32 re-summation {measured:.3e})")
    check_abs(got, ref, tol * np.asarray(mag, np.float64) + extra, what)


def norm_bound(x_ref, dx, tol_n, eps=O.SN_EPS):
    """bound of x / max(|x|, eps) given the elementwise bound dx of x and the reduction tolerance of the squared norm"""
    N = max(float(np.linalg.norm(x_ref)), eps)
    return dx / N + np.abs(x_ref) / N * (tol_n + float(np.linalg.norm(dx)) / N + 4 * U)


def sigma_bound(s_ref, ds, tol_n):
    return (1.5 * (tol_n + 2.0 * float(np.linalg.norm(ds)) / max(float(np.linalg.norm(s_ref)), TINY)) + 3 * U)


def sq_err(x):
    return R.f32_sum_error(np.asarray(x, np.float64) ** 2)[0]


def coef(step):
    """the bias corrections of csrc/sgv_ew.h's adam_coef: formed in double from the exact betas, rounded to fp32"""
    return float(np.float32(1.0 - 0.9 ** step)), float(np.float32(np.sqrt(1.0 - 0.999 ** step)))


def sn_grad_bound(go, u, v, cdot, inv_sigma, shape):
    """e_g of g = (G - (u cdot) v) / sigma: 2 U (|g| + |u cdot v / sigma|)"""
    uv = np.abs(O.f64(u)[None, :, None] * O.f64(v).reshape(shape[0], 1, shape[2]) * float(cdot) * float(inv_sigma))
    return 2 * U * (np.abs(go) + uv)


def check_update(tag, shape, g_ref, e_g, got, old, lr, wd, step, gscale, bc=None, inc_extra=0.0, old_err=None):
    """got / old: dicts of p, m, v.  The bounds are derived in the module docstring of tests/test_optim_kernels_gpu.py, one term per
    line here.  bc: the launch's own (bc1, bc2sqrt) where it does not form them as coef(step) does; inc_extra: a further term of
    the increment's bound, per element (a caller whose kernel rounds once more states which rounding); old_err: the bounds of
    the incoming moments (dict of m, v) where old holds float64 reference moments, not the kernel's own (a set that keeps its
    moments to itself): they enter m and v scaled by b1 and b2.  got without m / v: only the increment is compared.  The
    result carries the bounds as e_m, e_v, e_inc."""
    bc1, bc2s = coef(step) if bc is None else bc
    sh = shape
    p0, m0, v0 = (O.f64(old[k]).reshape(sh) for k in ("p", "m", "v"))
    r = O.adamw(p0, g_ref, m0, v0, lr, step, wd, eps=EPS, b1=B1, b2=B2, gscale=gscale, bc1=bc1, bc2sqrt=bc2s)
    g = r["g"]
    if gscale is not None:
        e_g = e_g * abs(gscale) + U * np.abs(g)                                 # g * gscale
    e_m = (3 * U * (np.abs(m0) * B1 + (1 - B1) * np.abs(g))                    # m b1, (1 - b1) g, their sum
           + (1 - B1) * e_g                                                     # the gradient's own error
           + (B1 * old_err["m"] if old_err else 0.0))
    e_v = (3 * U * r["v"]                                                       # (1 - b2) g, * g, v b2 / the sum (positive terms)
           + (1 - B2) * (2 * np.abs(g) * e_g + e_g * e_g)                       # the gradient's own error
           + (B2 * old_err["v"] if old_err else 0.0))
    rel_v = np.where(r["v"] > 0, e_v / np.maximum(2 * r["v"], TINY), 0.0)       # sqrt halves the relative error
    e_u = ((lr / bc1) * e_m / r["denom"]                                        # the numerator's error
           + np.abs(r["update"]) * (rel_v + 9 * U))                             # sqrt 2, / bc2sqrt 2, + eps 1, quotient 2, lr / bc1 1, product 1
    e_inc = (e_u
             + (np.abs(p0) * 2.0 ** -25 + U * np.abs(p0 * r["decay"]) if r["decay"] != 1.0 else 0.0)   # decay rounded next to 1; p * decay
             + U * np.abs(r["p"])                                               # the final subtraction
             + inc_extra)
    if "m" in got:
        check_abs(got["m"], r["m"], e_m + TINY, f"{tag} m")
        check_abs(got["v"], r["v"], e_v + TINY, f"{tag} v")
    check_abs(O.f64(got["p"]).reshape(sh) - p0, r["p"] - p0, e_inc + TINY, f"{tag} p_new - p_old")
    r.update(e_m=e_m, e_v=e_v, e_inc=e_inc + TINY)
    return r
