"""tests/ew_reference.py (PyTorch float64 + autograd) pinned to the numpy oracle the golden vectors tie to the reference
project (oracle/vae_oracle.py): losses, both KL terms, the reparameterisations and GroupNorm / GELU, forward and backward, with
log-variances on both sides of the clamps and exactly on them.  The oracle returns float32, hence the 2e-6 relative bound.
Also: the float32 re-summation that the GPU tests derive their reduction tolerances from stays under the figures of their TOL
table."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ew_reference as R  # noqa: E402
from oracle import vae_oracle as vo  # noqa: E402

RTOL = 2e-6       # float32 results of the oracle: a few ulps of 6e-8


def _close(a, b, scale=None):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    s = np.abs(b).max() if scale is None else scale
    assert np.all(np.abs(a - b) <= RTOL * s), (np.abs(a - b).max(), s)      # max-norm: the oracle's intermediates are float32 too


def _clamp_inputs(seed, shape):
    """ordinary values with the clamp set planted in the first positions"""
    rng = np.random.default_rng(seed)
    lv = rng.standard_normal(shape).astype(np.float32)
    flat = lv.reshape(-1)
    flat[:len(R.LV_CLAMP_SET)] = np.array(R.LV_CLAMP_SET, np.float32)
    return rng, lv


@pytest.mark.parametrize("kind", range(4))
def test_losses_match_oracle(kind):
    rng = np.random.default_rng(kind)
    B, T, C, G = 3, 10, 72, 8
    y = rng.standard_normal((B, T, C)).astype(np.float32) * 2 + 0.5
    x = rng.uniform(-2, 2, (B, T, C)).astype(np.float32)
    gamma = (1 + 0.2 * rng.standard_normal(C)).astype(np.float32)
    beta = (0.2 * rng.standard_normal(C)).astype(np.float32)
    r = R.recon_loss(y, x, G, gamma, beta, kind, True)
    share = np.mean(np.abs(r["diff"]) > 1)
    assert 0.2 < share < 0.8
    n = y.size
    sel, mse, g = vo.recon_losses(r["xhat"], x.astype(np.float64), R.LOSSES[kind])
    assert abs(r["loss"] / n - sel) <= RTOL * abs(sel) and abs(r["sq"] / n - mse) <= RTOL * mse
    # the loss gradient wrt xhat, element by element: autograd's dz = g * (1 - xhat^2)
    yt = np.transpose(y, (0, 2, 1))
    zo, cache = vo.gn_fwd(yt, G, gamma, beta)
    dz = g.astype(np.float64) * n * (1 - r["xhat"] ** 2)
    dx, dgam, dbet = vo.gn_bwd(cache, gamma, np.transpose(dz, (0, 2, 1)).astype(np.float32))
    _close(np.transpose(r["dy"], (0, 2, 1)), dx)
    _close(r["dgamma"], dgam)
    _close(r["dbeta"], dbet)


@pytest.mark.parametrize("act", [0, 1])
def test_groupnorm_gelu_match_oracle(act):
    rng = np.random.default_rng(10 + act)
    B, T, C, G = 2, 13, 64, 8
    y = rng.standard_normal((B, T, C)).astype(np.float32)
    dout = rng.standard_normal((B, T, C)).astype(np.float32)
    gamma = (1 + 0.2 * rng.standard_normal(C)).astype(np.float32)
    beta = (0.2 * rng.standard_normal(C)).astype(np.float32)
    f = R.gn_forward(y, G, gamma, beta, act)
    b = R.gn_backward(y, dout, G, gamma, beta, act)
    zo, cache = vo.gn_fwd(np.transpose(y, (0, 2, 1)), G, gamma, beta)
    out = vo.gelu_fwd(zo) if act else zo
    _close(np.transpose(f["out"], (0, 2, 1)), out)
    dzo = np.transpose(dout, (0, 2, 1))
    if act:
        dzo = vo.gelu_bwd(zo, dzo)
    dx, dgam, dbet = vo.gn_bwd(cache, gamma, dzo)
    _close(np.transpose(b["dy"], (0, 2, 1)), dx)
    _close(b["dgamma"], dgam, np.abs(b["dgamma_mag"]).max())
    _close(b["dbeta"], dbet, np.abs(b["dbeta_mag"]).max())
    # the definitions of the extra reductions agree with the closed form (m1, m2 of GroupNorm's backward)
    xh = cache[0].astype(np.float64)
    gd = (dzo.astype(np.float64) * gamma[None, :, None]).reshape(B, G, -1)
    _close(b["sums2"][..., 0], gd.sum(2), np.abs(b["sums2_mag"]).max())
    _close(b["sums2"][..., 1], (gd * xh.reshape(B, G, -1)).sum(2), np.abs(b["sums2_mag"]).max())


def test_latent_matches_oracle_beyond_the_clamps():
    B, Z = 5, 7
    rng, lv = _clamp_inputs(3, (B, Z))
    mu = rng.standard_normal((B, Z)).astype(np.float32)
    eps = rng.standard_normal((B, Z)).astype(np.float32)
    dz = rng.standard_normal((B, Z)).astype(np.float32)
    beta_w = 0.37
    r = R.latent(np.concatenate([mu, lv], 1), eps, dz, beta_w / B)
    _close(r["z"], vo.reparam_fwd(mu, lv, eps))
    assert abs(r["kl"] - vo.kl_fwd(mu, lv)) <= RTOL * abs(r["kl"])
    kmu, klv = vo.kl_bwd(mu.astype(np.float64), lv.astype(np.float64), beta_w)
    rmu, rlv = vo.reparam_bwd(lv, eps, dz)
    ref = np.concatenate([rmu + kmu, rlv.astype(np.float64) + klv.astype(np.float64)], 1)
    assert np.all(np.abs(r["dlast"] - ref) <= RTOL * r["dlast_mag"] + 1e-12)
    # both masks on and off at the planted positions
    g_lv = r["dlast"][:, Z:].reshape(-1)[:len(R.LV_CLAMP_SET)]
    assert g_lv[0] == 0 and g_lv[7] == 0 and g_lv[1] != 0 and g_lv[6] != 0


@pytest.mark.parametrize("std_scale", [1.0, 0.5])
def test_stage_matches_oracle_beyond_the_clamps(std_scale):
    M, C = 6, 9
    rng, lv = _clamp_inputs(4, (M, C))
    _, dlv = _clamp_inputs(5, (M, C))
    dlv = np.roll(dlv.reshape(-1), 16).reshape(M, C)          # lv planted at 0..7 (dlv ordinary), dlv at 16..23 (lv ordinary)
    half = (np.array(R.LV_CLAMP_SET, np.float32) / 2)
    lv.reshape(-1)[32:40] = half
    dlv.reshape(-1)[32:40] = half                             # lv + dlv planted at 32..39
    mu, dmu, eps, dzs, dec = (rng.standard_normal((M, C)).astype(np.float32) for _ in range(5))
    beta_w = 0.21
    B = 3
    r = R.stage(np.concatenate([mu, lv], 1), np.concatenate([dmu, dlv], 1), eps, dec, std_scale, 1.0 / B, dzs, beta_w / B)
    _close(r["z"], vo.reparam_fwd(mu + dmu, lv + dlv, eps, std_scale))
    ko = vo.kl2_fwd(dmu.reshape(B, -1, C), dlv.reshape(B, -1, C), mu.reshape(B, -1, C), lv.reshape(B, -1, C))
    assert abs(r["kl"] - ko) <= RTOL * r["kl_mag"]
    g_dmu, g_dlv, g_mu, g_lv = (a.astype(np.float64) for a in vo.kl2_bwd(dmu.reshape(B, -1, C), dlv.reshape(B, -1, C), mu.reshape(B, -1, C),
                                                                          lv.reshape(B, -1, C), beta_w))
    _, rlv = vo.reparam_bwd(lv + dlv, eps, dzs)
    ref_p = np.concatenate([dzs + g_mu.reshape(M, C), rlv + g_lv.reshape(M, C)], 1)
    ref_q = np.concatenate([dzs + g_dmu.reshape(M, C), rlv + g_dlv.reshape(M, C)], 1)
    assert np.all(np.abs(r["g_p"] - ref_p) <= RTOL * r["g_p_mag"] + 1e-12)
    assert np.all(np.abs(r["g_q"] - ref_q) <= RTOL * r["g_q_mag"] + 1e-12)


def test_f32_resummation_stays_under_the_tol_table():
    """The GPU tests allow a reduction max(4 x measured, 2^-22) where `measured` is this float32 re-summation on the test's own inputs;
    the orientation figures of their TOL table are upper bounds of it at the mid-size recon shape."""
    import test_ew_kernels_gpu as K
    rng = np.random.default_rng(0)
    B, T, C, G = 2, 200, 2080, 8
    y = (rng.standard_normal((B, T, C)) * 2 + 0.5).astype(np.float32)
    x = rng.uniform(-2, 2, (B, T, C)).astype(np.float32)
    r = R.recon_loss(y, x, G, np.ones(C, np.float32), np.zeros(C, np.float32), 0, False)
    d = r["diff"]
    assert R.f32_sum_error(d * d)[0] <= K.TOL["loss"][0]
    assert R.f32_sum_error((d * d).reshape(B * T, C), axis=0)[0] <= K.TOL["column"][0]
    assert R.f32_sum_error(y.astype(np.float64).reshape(B, T, G, C // G), axis=(1, 3))[0] <= K.TOL["group"][0]
    for k, (measured, floor) in K.TOL.items():
        assert floor == 2.0 ** -22 and measured < 1e-6, k
