"""The float64 references of tests/test_lc_param_ops_gpu.py (tests/optim_reference.py used on a plain [rows][cols] matrix, its
conv-weight packing and its clip coefficient) against torch in float64 on the CPU: torch.nn.utils.spectral_norm (the legacy hook
the reference conditioner uses: one power iteration, eps 1e-12) on an nn.Linear and an nn.Conv2d with KH != KW, the permute +
reshape statement of the packed layout, and torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW over three steps.  CPU only."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import optim_reference as O  # noqa: E402

TOL = 1e-12     # float64 against float64: a few hundred roundings of 2^-53 = 1.1e-16 relative to the largest element


def _close(a, b, tol, what):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)
    print(f"{what}: {err:.3e} (tolerance {tol:.1e})")
    assert err <= tol, (what, err)


def _sn_modules():
    torch.manual_seed(11)
    return [("linear", torch.nn.Linear(12, 7).double(), torch.randn(3, 12, dtype=torch.float64)),
            ("conv2d 5x3", torch.nn.Conv2d(4, 6, (5, 3), padding=(2, 1)).double(), torch.randn(2, 4, 6, 5, dtype=torch.float64))]


@pytest.mark.parametrize("which", [0, 1], ids=["linear", "conv2d_kh_ne_kw"])
def test_power_iteration_and_sn_backward_match_torch_spectral_norm(which):
    name, mod, x = _sn_modules()[which]
    mod = torch.nn.utils.spectral_norm(mod)          # n_power_iterations 1, eps 1e-12
    W = mod.weight_orig.detach().numpy().copy()
    rows = W.shape[0]
    Wm = W.reshape(rows, -1)                         # the matrix the hook sees
    u0, v0 = mod.weight_u.detach().numpy().copy(), mod.weight_v.detach().numpy().copy()
    mod.train()
    y = mod(x)
    r = O.power_iteration(O.as_taps(Wm), u0, v0, True)
    _close(r["u"], mod.weight_u.detach().numpy(), TOL, f"{name} u")
    _close(r["v"], mod.weight_v.detach().numpy(), TOL, f"{name} v")
    assert not np.allclose(r["u"], u0) and not np.allclose(r["v"], v0), "the power iteration moved nothing"
    W_eff = mod.weight.detach().numpy()
    _close(Wm / r["sigma"], W_eff.reshape(rows, -1), TOL, f"{name} W / sigma")
    # the gradient: autograd wrt weight_orig against sn_backward applied to the gradient wrt W / sigma
    mod.weight.retain_grad()
    dy = torch.randn(y.shape, dtype=torch.float64, generator=torch.Generator().manual_seed(5))
    y.backward(dy)
    G = mod.weight.grad.numpy().reshape(rows, -1)
    got = O.sn_backward(O.as_taps(G), O.as_taps(Wm), r["sigma"], r["u"], r["v"])
    _close(got.reshape(W.shape), mod.weight_orig.grad.numpy(), TOL, f"{name} gradient wrt weight_orig")
    assert np.abs(got.reshape(rows, -1) - G / r["sigma"]).max() > 1e-3 * np.abs(G).max(), "the u v^T term does not show in this case"
    # eval: sigma from the stored vectors, nothing moves
    e = O.power_iteration(O.as_taps(Wm), r["u"], r["v"], False)
    assert np.array_equal(e["u"], r["u"]) and np.array_equal(e["v"], r["v"])
    mod.eval()
    mod(x)
    _close(Wm / e["sigma"], mod.weight.detach().numpy().reshape(rows, -1), TOL, f"{name} W / sigma (eval)")


PACK_SHAPES = [(3, 1, 7, 7), (5, 3, 3, 3), (16, 8, 3, 3), (4, 2, 1, 1), (2, 5, 5, 3), (2, 3, 1, 4)]


@pytest.mark.parametrize("shape", PACK_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_pack_and_unpack_are_the_permutation(shape):
    cout, cin, kh, kw = shape
    w = torch.arange(cout * cin * kh * kw, dtype=torch.float32).reshape(shape) + 1.0      # every element distinct and non-zero
    k = kh * kw * cin
    packed = O.conv_weight_pack(w.numpy())
    assert packed.shape == (cout, (k + 7) // 8 * 8) and packed.dtype == np.float32
    assert np.array_equal(packed[:, :k], w.permute(0, 2, 3, 1).reshape(cout, -1).numpy())
    assert not packed[:, k:].any(), "pad columns must be zero"
    assert np.array_equal(O.conv_weight_unpack(packed, shape), w.numpy())
    dirty = packed.copy()
    dirty[:, k:] = np.nan
    assert np.array_equal(O.conv_weight_unpack(dirty, shape), w.numpy()), "unpack read a pad column"
    if kh != kw and min(kh, kw) > 1:        # the transposed window is a different matrix: a KH / KW swap cannot pass
        swapped = w.permute(0, 1, 3, 2).contiguous().permute(0, 2, 3, 1).reshape(cout, -1).numpy()
        assert not np.array_equal(packed[:, :k], swapped)


def test_clip_coef_definition():
    assert O.clip_coef(3.0, 10.0) == 1.0
    assert O.clip_coef(20.0, 10.0) == 10.0 / (20.0 + 1e-6)
    assert O.clip_coef(10.0, 10.0) == 10.0 / (10.0 + 1e-6)      # torch clamps to 1 but does not skip the 1e-6
    assert O.clip_coef(5.0, 0.0) == 0.0                         # the formula itself: max_norm 0 zeroes the gradient


def test_clip_and_adamw_match_torch_over_three_steps():
    rng = np.random.default_rng(8)
    shapes, lr, wd = [(9, 5), (33,)], 1e-3, 0.1
    p0 = [rng.standard_normal(s) for s in shapes]
    pt = [torch.from_numpy(p.copy()).requires_grad_(True) for p in p0]
    opt = torch.optim.AdamW(pt, lr=lr, weight_decay=wd)          # betas (0.9, 0.999), eps 1e-8
    p = [a.copy() for a in p0]
    m, v = [np.zeros(s) for s in shapes], [np.zeros(s) for s in shapes]
    max_norm, clipped = 12.0, []
    for step, gs in enumerate((1.0, 3.0, 0.5), start=1):         # |g| about sqrt(78) gs = 8.8, 26, 4.4
        g = [rng.standard_normal(s) * gs for s in shapes]
        for t, a in zip(pt, g):
            t.grad = torch.from_numpy(a.copy())
        total_t = float(torch.nn.utils.clip_grad_norm_(pt, max_norm))
        opt.step()
        total = float(np.sqrt(sum(O.adamw(p[k], g[k], m[k], v[k], lr, step, wd)["gnorm_sq"] for k in range(2))))
        c = O.clip_coef(total, max_norm)
        clipped.append(c < 1.0)
        _close(total, total_t, TOL, f"total norm, step {step}")
        for k in range(2):
            r = O.adamw(p[k], g[k], m[k], v[k], lr, step, wd, gscale=c)
            _close(r["g"], pt[k].grad.numpy(), TOL, f"clipped gradient {k}, step {step}")
            p[k], m[k], v[k] = r["p"], r["m"], r["v"]
            _close(p[k] - p0[k], pt[k].detach().numpy() - p0[k], 1e-11, f"p - p0 of tensor {k} after step {step}")
            _close(m[k], opt.state[pt[k]]["exp_avg"].numpy(), TOL, "exp_avg")
            _close(v[k], opt.state[pt[k]]["exp_avg_sq"].numpy(), TOL, "exp_avg_sq")
    assert clipped == [False, True, False], clipped
    # decay is visible: three steps of 1 - lr wd move p by 3e-4 relative, far above the tolerance
    no_wd = O.adamw(p0[0], np.ones(shapes[0]), np.zeros(shapes[0]), np.zeros(shapes[0]), lr, 1, 0.0)["p"]
    with_wd = O.adamw(p0[0], np.ones(shapes[0]), np.zeros(shapes[0]), np.zeros(shapes[0]), lr, 1, wd)["p"]
    _close(no_wd - with_wd, lr * wd * p0[0], 1e-10, "the decay term")
