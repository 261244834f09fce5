"""tests/optim_reference.py (the float64 reference of tests/test_optim_kernels_gpu.py) against three independent statements of the
same operations: oracle/vae_oracle.py (the numpy oracle of the engine goldens, fp32), torch.optim.AdamW in float64 and
torch.nn.utils.spectral_norm on a float64 Conv1d.  CPU only."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import optim_reference as O  # noqa: E402
from oracle import vae_oracle as vo  # noqa: E402

F32_TOL = 2e-6     # float32 oracle vs float64: a handful of roundings of 2^-24 = 6e-8 relative to the largest element


def _close(a, b, tol, what):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    err = np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)
    print(f"{what}: {err:.3e} (tolerance {tol:.1e})")
    assert err <= tol, (what, err)


def _conv_case(seed, cout, cin, k):
    rng = np.random.default_rng(seed)
    W = rng.standard_normal((cout, cin, k)).astype(np.float32)
    u = rng.standard_normal(cout).astype(np.float32)
    v = rng.standard_normal(cin * k).astype(np.float32)
    G = rng.standard_normal((cout, cin, k)).astype(np.float32)
    return W, u / np.linalg.norm(u), v / np.linalg.norm(v), G


def test_layout_round_trip():
    W, _, v, _ = _conv_case(0, 5, 3, 4)
    Wi = O.weight_to_internal(W)
    assert Wi.shape == (4, 5, 3) and Wi[2, 1, 0] == W[1, 0, 2]
    assert np.array_equal(O.weight_from_internal(Wi), W)
    vi = O.v_to_internal(v, 3, 4)
    assert vi[2 * 3 + 1] == v[1 * 4 + 2]
    assert np.array_equal(O.v_from_internal(vi, 3, 4), v)
    # the matrix spectral norm sees: W.reshape(Cout, Cin*K) v == sum over (tap, col) of the internal layout
    assert np.allclose(W.reshape(5, -1).astype(np.float64) @ v, O.w_v(Wi, vi)[0], rtol=1e-13, atol=1e-13)
    lin = np.arange(6, dtype=np.float32).reshape(2, 3)
    assert O.weight_to_internal(lin).shape == (1, 2, 3)


def test_wct_copy_definition():
    p = np.random.default_rng(1).standard_normal((3, 4, 5))
    t = O.wct_copy(p)
    assert t.shape == (3, 5, 4)
    for tap in range(3):
        for r in range(4):
            for c in range(5):
                assert t[3 - 1 - tap, c, r] == p[tap, r, c]


def test_bf16_round_is_nearest_even():
    x = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20, -3.1415927], np.float32)
    r = O.bf16_round(x)
    assert r[0] == 1.0 and r[1] == 1.0 and r[2] == 1.0 + 2.0 ** -6 and r[3] == 1.0 + 2.0 ** -7
    assert abs(r[4] - x[4]) <= 2.0 ** -8 * abs(x[4])
    bits = O.bf16_bits(x)
    assert np.array_equal((bits.astype(np.uint32) << 16).view(np.float32), r)


def test_power_iteration_matches_oracle():
    for seed, (cout, cin, k) in enumerate([(6, 4, 3), (9, 8, 1), (70, 12, 5)]):
        W, u, v, _ = _conv_case(seed, cout, cin, k)
        for train in (True, False):
            _, sigma, uo, vo_ = vo.sn_forward(W, u, v, "conv", train)
            r = O.power_iteration(O.weight_to_internal(W), u, O.v_to_internal(v, cin, k), train)
            _close(r["sigma"], sigma, F32_TOL, f"sigma train={train}")
            _close(r["u"], uo, F32_TOL, "u")
            _close(O.v_from_internal(r["v"], cin, k), vo_, F32_TOL, "v")
            if not train:
                assert np.array_equal(r["u"], u.astype(np.float64)) and np.array_equal(O.v_from_internal(r["v"], cin, k), v.astype(np.float64))


def test_chain_rule_matches_oracle_and_autograd():
    for seed, (cout, cin, k) in enumerate([(6, 4, 3), (9, 8, 1)]):
        W, u, v, G = _conv_case(10 + seed, cout, cin, k)
        Wi, vi = O.weight_to_internal(W), O.v_to_internal(v, cin, k)
        sigma = O.power_iteration(Wi, u, vi, False)["sigma"]
        got = O.weight_from_internal(O.sn_backward(O.weight_to_internal(G), Wi, sigma, u, vi))
        _close(got, vo.sn_backward(G, W, np.float32(sigma), u, v, "conv"), F32_TOL, "sn_backward vs oracle")
        # autograd: L = <G, W / (u^T W v)> with u, v constants
        Wt = torch.from_numpy(W.astype(np.float64)).requires_grad_(True)
        s = torch.from_numpy(u.astype(np.float64)) @ (Wt.reshape(cout, -1) @ torch.from_numpy(v.astype(np.float64)))
        (torch.from_numpy(G.astype(np.float64)) * (Wt / s)).sum().backward()
        _close(got, Wt.grad.numpy(), 1e-12, "sn_backward vs autograd")


def test_adamw_matches_oracle_step():
    rng = np.random.default_rng(3)
    n, lr = 257, 1e-3
    for step, wd in ((1, 0.01), (2, 0.01), (10, 0.0), (1000, 0.01)):
        p, g = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
        m, v = (0.1 * rng.standard_normal(n)).astype(np.float32), (0.1 * rng.random(n) + 1e-3).astype(np.float32)
        if step == 1:
            m[:], v[:] = 0, 0
        ns = SimpleNamespace(adam={"w": [m.copy(), v.copy()]}, t=step - 1, grads={"w": g.copy(), "none": None}, P={"w": p.copy()})
        vo.OracleVAE.adamw_step(ns, lr, wd=wd)
        r = O.adamw(p, g, m, v, lr, step, wd)
        _close(r["m"], ns.adam["w"][0], F32_TOL, f"m step {step}")
        _close(r["v"], ns.adam["w"][1], F32_TOL, f"v step {step}")
        _close(r["p"] - p, ns.P["w"].astype(np.float64) - p, 2e-4, f"increment step {step}")      # the oracle's p is fp32: the increment carries its rounding
        _close(r["p"], ns.P["w"], F32_TOL, f"p step {step}")


def test_adamw_matches_torch_float64_over_five_steps():
    rng = np.random.default_rng(4)
    n, lr, wd = 301, 1e-3, 0.01
    p0 = rng.standard_normal(n)
    pt = torch.from_numpy(p0.copy()).requires_grad_(True)
    opt = torch.optim.AdamW([pt], lr=lr, weight_decay=wd)          # betas (0.9, 0.999), eps 1e-8
    p, m, v = p0.copy(), np.zeros(n), np.zeros(n)
    for step in range(1, 6):
        g = rng.standard_normal(n) * 10.0 ** rng.integers(-3, 2, n)
        pt.grad = torch.from_numpy(g.copy())
        opt.step()
        r = O.adamw(p, g, m, v, lr, step, wd)
        p, m, v = r["p"], r["m"], r["v"]
        st = opt.state[pt]
        _close(p - p0, pt.detach().numpy() - p0, 1e-12, f"p - p0 after step {step}")
        _close(m, st["exp_avg"].numpy(), 1e-12, "exp_avg")
        _close(v, st["exp_avg_sq"].numpy(), 1e-12, "exp_avg_sq")
    assert abs(r["gnorm_sq"] - float((g * g).sum())) <= 1e-12 * r["gnorm_sq"]


def test_adamw_gscale_scales_the_gradient_after_the_norm():
    rng = np.random.default_rng(5)
    p, g, m, v = rng.standard_normal(8), rng.standard_normal(8), rng.standard_normal(8), rng.random(8)
    a = O.adamw(p, g, m, v, 1e-3, 7, 0.01, gscale=0.25)
    b = O.adamw(p, 0.25 * g, m, v, 1e-3, 7, 0.01)
    assert np.array_equal(a["p"], b["p"]) and np.array_equal(a["v"], b["v"])
    assert a["gnorm_sq"] == float((g * g).sum())


def test_power_iteration_matches_torch_spectral_norm():
    torch.manual_seed(6)
    for cout, cin, k in ((7, 4, 3), (5, 8, 1)):
        conv = torch.nn.utils.spectral_norm(torch.nn.Conv1d(cin, cout, k).double())
        W = conv.weight_orig.detach().numpy().copy()
        u0, v0 = conv.weight_u.detach().numpy().copy(), conv.weight_v.detach().numpy().copy()
        conv.train()
        conv(torch.zeros(1, cin, 8, dtype=torch.float64))
        r = O.power_iteration(O.weight_to_internal(W), u0, O.v_to_internal(v0, cin, k), True)
        sigma_t = float(np.linalg.norm(W) / np.linalg.norm(conv.weight.detach().numpy()))      # weight = weight_orig / sigma
        _close(r["u"], conv.weight_u.detach().numpy(), 1e-12, "u")
        _close(O.v_from_internal(r["v"], cin, k), conv.weight_v.detach().numpy(), 1e-12, "v")
        _close(r["sigma"], sigma_t, 1e-12, "sigma")


def test_clamp_of_both_normalisations():
    W = np.full((1, 2, 4), 1e-15)
    r = O.power_iteration(W, np.ones(2), np.zeros(4), True)
    assert np.allclose(r["v"], 2e-15 / 1e-12, rtol=1e-14) and np.allclose(r["u"], r["s"] / 1e-12, rtol=1e-14)
    z = O.power_iteration(np.zeros((1, 2, 4)), np.ones(2), np.ones(4), True)
    assert not z["u"].any() and not z["v"].any() and z["sigma"] == 0.0
