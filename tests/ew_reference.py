"""Plain float64 statements of the operations csrc/ew.hip implements, written with PyTorch on the CPU and autograd (no
hand-derived backward formulas).  Maps are channels-last [B, T, C] like the kernels'; group g owns channels g*Cg .. (g+1)*Cg.
Inputs are numpy arrays already rounded to the compute dtype, so the reference sees the numbers the kernel sees.  Every function
returns a dict of float64 numpy arrays.  The extra reductions the kernels emit are defined from autograd's gradient wrt the
normalised-and-affine value z (retain_grad):
    sums2 = (sum gamma dz, sum gamma dz xhat) per (sample, group),  dbias = sum over rows of dY,  cdot = sum dY * (y - cbias).
Reductions come with `<name>_mag`, the sum of the magnitudes of their terms (the scale their tolerance refers to).
No GPU is touched at import or in any function."""
import numpy as np
import torch
import torch.nn.functional as F

GN_EPS = 1e-5
LOSSES = ("MSE", "MAE", "smoothL1", "Huber")      # SGV_LOSS_* order
LV_CLAMP_SET = (-40.0, -30.0, -29.9, 0.0, 4.7, 29.9, 30.0, 40.0)


def _t(a, grad=False):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(torch.float64)
    return t.requires_grad_(True) if grad else t


def _n(t):
    return t.detach().numpy()


def act_apply(act, z):
    """act: 0 none, 1 GELU (exact erf), 2 tanh, 3 ReLU."""
    return z if act == 0 else F.gelu(z) if act == 1 else torch.tanh(z) if act == 2 else F.relu(z)


def _gn(y, G, gamma=None, beta=None):
    return F.group_norm(y.permute(0, 2, 1), G, gamma, beta, eps=GN_EPS).permute(0, 2, 1)


def _group_sum(a, G):
    B, T, C = a.shape
    return a.reshape(B, T, G, C // G).sum(dim=(1, 3))


def gn_stats(y, G):
    y = _t(y)
    return {"sums": _n(torch.stack((_group_sum(y, G), _group_sum(y * y, G)), dim=-1)),
            "sums_mag": _n(torch.stack((_group_sum(y.abs(), G), _group_sum(y * y, G)), dim=-1))}


def gn_forward(y, G, gamma, beta, act, res=None, rscale=1.0):
    """out = [res + rscale *] act(GroupNorm(y)); also the statistics and z (to find elements next to a kink)."""
    yt = _t(y)
    z = _gn(yt, G, _t(gamma), _t(beta))
    out = act_apply(act, z)
    if res is not None:
        out = _t(res) + rscale * out
    r = gn_stats(y, G)
    r.update(out=_n(out), z=_n(z))
    return r


def _bwd_extras(r, yt, z, xhat, gamma_t, G, gscale, cbias):
    dz = z.grad
    gdz = gamma_t.detach() * dz
    r["sums2"] = _n(torch.stack((_group_sum(gdz, G), _group_sum(gdz * xhat, G)), dim=-1))
    r["sums2_mag"] = _n(torch.stack((_group_sum(gdz.abs(), G), _group_sum((gdz * xhat).abs(), G)), dim=-1))
    r["dgamma"] = _n(gamma_t.grad)
    r["dgamma_mag"] = _n((dz * xhat).abs().sum(dim=(0, 1)))
    dy = gscale * yt.grad
    r["dy"] = _n(dy)
    r["dbias"] = _n(dy.sum(dim=(0, 1)))
    # The kernels do not add dY up: they form the column sum in closed form per sample,
    #   gscale * rstd * (gamma_c * sum_t dz - T * m1 - m2 * sum_t xhat),   m1, m2 = sums2 / (T * Cg),
    # so its rounding error scales with the magnitudes of THESE terms (which cancel), not with sum |dY|: that is the scale.
    B, T, Cn = dz.shape
    n = T * (Cn // G)
    yd = yt.detach()
    var = _group_sum(yd * yd, G) / n - (_group_sum(yd, G) / n) ** 2
    rstd = (1.0 / torch.sqrt(var + GN_EPS)).repeat_interleave(Cn // G, dim=1)                      # [B, C]
    m1 = (_group_sum(gdz, G) / n).abs().repeat_interleave(Cn // G, dim=1)
    m2 = (_group_sum(gdz * xhat, G) / n).abs().repeat_interleave(Cn // G, dim=1)
    closed = abs(gscale) * rstd * (gamma_t.detach().abs() * dz.abs().sum(dim=1) + T * m1 + m2 * xhat.abs().sum(dim=1))
    r["dbias_mag"] = _n(torch.maximum(closed.sum(dim=0), dy.abs().sum(dim=(0, 1))))
    w = dy * (yt.detach() - (_t(cbias) if cbias is not None else 0.0))
    r["cdot"] = float(w.sum())
    r["cdot_mag"] = float(w.abs().sum())
    r["z"] = _n(z)
    r["dz"] = _n(dz)
    r["xnorm"] = _n(xhat)
    return r


def gn_backward(y, dout, G, gamma, beta, act, rscale=1.0, gscale=1.0, cbias=None):
    """Backward of L = sum dout * rscale * act(GroupNorm(y)): dgamma, dbeta, sums2 as autograd gives them; dy = gscale * dL/dy,
    dbias and cdot from that dy (the kernels apply the output-gradient scale to the gradient that flows on only)."""
    yt, gt, bt = _t(y, True), _t(gamma, True), _t(beta, True)
    z = _gn(yt, G, gt, bt)
    z.retain_grad()
    (_t(dout) * (rscale * act_apply(act, z))).sum().backward()
    xhat = _gn(yt.detach(), G)
    r = {"dbeta": _n(bt.grad), "dbeta_mag": _n(z.grad.abs().sum(dim=(0, 1)))}
    return _bwd_extras(r, yt, z, xhat, gt, G, gscale, cbias)


def gn_bwd_terms_f32(y, dout, G, gamma, beta, act, rscale=1.0, loss_kind=None):
    """The terms of dbeta (dz) and dgamma (dz * xhat) evaluated in float32 from the same inputs (statistics from float64, as the
    kernels take them): the float32 restatement the column-sum tolerance is measured on.  act' comes from autograd in float32.
    loss_kind given: the recon head instead, dz = gradient of the loss sum of tanh(z) against the target `dout`."""
    f32 = torch.float32
    yd = _t(y)
    B, T, Cn = yd.shape
    n = T * (Cn // G)
    mean = _group_sum(yd, G) / n
    rstd = 1.0 / torch.sqrt(_group_sum(yd * yd, G) / n - mean * mean + GN_EPS)
    mean, rstd = (a.to(f32).repeat_interleave(Cn // G, dim=1)[:, None, :] for a in (mean, rstd))
    xh = (yd.to(f32) - mean) * rstd
    z = (xh * _t(gamma).to(f32) + _t(beta).to(f32)).requires_grad_(True)
    if loss_kind is not None:
        loss_sum(loss_kind, torch.tanh(z), _t(dout).to(f32)).backward()
        dz = z.grad
    else:
        act_apply(act, z).sum().backward()
        dz = _t(dout).to(f32) * np.float32(rscale) * z.grad
    return dz.numpy(), (dz * xh.detach()).numpy()


def loss_sum(kind, xhat, x):
    """The selected reconstruction loss with reduction='sum' (the mean is folded into the weight by the caller)."""
    if kind == 0:
        return F.mse_loss(xhat, x, reduction="sum")
    if kind == 1:
        return F.l1_loss(xhat, x, reduction="sum")
    if kind == 2:
        return F.smooth_l1_loss(xhat, x, reduction="sum", beta=1.0)
    return F.huber_loss(xhat, x, reduction="sum", delta=1.0)


def recon_loss(y, x, G, gamma, beta, kind, train, gscale=1.0, cbias=None):
    """xhat = tanh(GroupNorm(y)) against x: loss sum, squared-error sum; train: the backward of the (unit-weight) loss sum with the
    unit-weight dgamma / dbeta / dbias_unit, and dy / cdot at weight gscale."""
    yt, gt, bt, xt = _t(y, train), _t(gamma, train), _t(beta, train), _t(x)
    z = _gn(yt, G, gt, bt)
    xhat = torch.tanh(z)
    L = loss_sum(kind, xhat, xt)
    d = (xhat - xt).detach()
    r = gn_stats(y, G)
    r.update(xhat=_n(xhat), loss=float(L.detach()), sq=float((d * d).sum()), diff=_n(d))
    with torch.no_grad():
        r["loss_mag"] = float(loss_sum(kind, xhat, xt).abs()) if kind != 1 else float(d.abs().sum())
    if not train:
        return r
    z.retain_grad()
    L.backward()
    nx = _gn(yt.detach(), G)
    r["dbeta"] = _n(bt.grad)
    r["dbeta_mag"] = _n(z.grad.abs().sum(dim=(0, 1)))
    _bwd_extras(r, yt, z, nx, gt, G, gscale, cbias)
    # |d(dz)/d(xhat)| per element, dz = loss'(xhat - x) * (1 - xhat^2): how far an absolute error of the kernels' fast tanh moves a term
    o = xhat.detach().requires_grad_(True)
    (g,) = torch.autograd.grad(loss_sum(kind, o, xt), o, create_graph=True)
    (sens,) = torch.autograd.grad((g * (1.0 - o * o)).sum(), o)
    r["tanh_sens"] = _n(sens.abs())
    r["dbias_unit"] = r["dbias"] / gscale
    r["dbias_unit_mag"] = r["dbias_mag"] / abs(gscale)
    return r


def act_forward(y):
    return {"out": _n(F.gelu(_t(y)))}


def act_backward(y, dout, rscale=1.0, cbias=None):
    """mode 1: out = dL/dy of L = sum dout * rscale * gelu(y); dbias = column sums of out, cdot = sum out * (y - cbias)."""
    yt = _t(y, True)
    (_t(dout) * (rscale * F.gelu(yt))).sum().backward()
    return colsum_dot(_n(yt.grad), y, cbias, out=True)


def colsum_dot(dY, yf, cbias=None, out=False):
    """mode 2: dbias = column sums of dY, cdot = sum dY * (yf - cbias)."""
    g = _t(dY)
    C = g.shape[-1]
    w = g * (_t(yf) - (_t(cbias) if cbias is not None else 0.0))
    r = {"dbias": _n(g.reshape(-1, C).sum(0)), "dbias_mag": _n(g.abs().reshape(-1, C).sum(0)), "cdot": float(w.sum()),
         "cdot_mag": float(w.abs().sum())}
    if out:
        r["out"] = _n(g)
    return r


def _reparam(mu, lv, eps, std_scale=1.0):
    std = torch.exp(0.5 * torch.clamp(lv, -30.0, 30.0)) * std_scale
    return mu + eps * torch.clamp(std, 1e-8, 10.0)


def _kl_terms(mu, lv):
    lvc = torch.clamp(lv, -30.0, 30.0)
    return 0.5 * (mu * mu + torch.exp(lvc) - lvc - 1.0)


def _kl2_terms(dmu, dlv, mu, lv):
    lvc, dlvc = torch.clamp(lv, -30.0, 30.0), torch.clamp(dlv, -30.0, 30.0)
    var = torch.exp(lvc) + 1e-8
    return 0.5 * (torch.exp(dlvc) / var + (mu - dmu) ** 2 / var - dlvc + lvc - 1.0)


def _two_part_grads(leaves, part_a, part_b):
    """gradients of part_a + part_b wrt the leaves, and the sum of the magnitudes of the two parts' gradients"""
    ga = torch.autograd.grad(part_a, leaves, retain_graph=True, allow_unused=True)
    gb = torch.autograd.grad(part_b, leaves, allow_unused=True)
    z0 = [torch.zeros_like(l) for l in leaves]
    ga = [g if g is not None else z for g, z in zip(ga, z0)]
    gb = [g if g is not None else z for g, z in zip(gb, z0)]
    return [_n(a + b) for a, b in zip(ga, gb)], [_n(a.abs() + b.abs()) for a, b in zip(ga, gb)]


def latent(last, eps, dz=None, coef=0.0):
    """last = [mu | logvar] [B, 2Z]: z, kl (batch mean of the row sums); dz given: gradient of sum dz z + coef * B * kl."""
    B, Z = eps.shape
    lt = _t(last, True)
    mu, lv = lt[:, :Z], lt[:, Z:]
    z = _reparam(mu, lv, _t(eps))
    terms = _kl_terms(mu, lv)
    r = {"z": _n(z), "kl": float(terms.detach().sum() / B), "kl_mag": float(terms.detach().abs().sum() / B)}
    if dz is not None:
        (g,), (m,) = _two_part_grads([lt], (_t(dz) * z).sum(), coef * terms.sum())
        r["dlast"], r["dlast_mag"] = g, m
    return r


def stage(pz, qz, eps, dec_out, std_scale=1.0, inv_b=1.0, dzs=None, coef=0.0):
    """pz = [mu | lv], qz = [dmu | dlv] [M, 2C]: z = (mu + dmu) + eps * clamp(exp(.5 clamp(lv + dlv)) * std_scale), zs = dec_out + z,
    kl = inv_b * sum of the KL(q || p) terms; dzs given: gradients of sum dzs z(std_scale = 1) + coef * sum of the KL terms."""
    M, C = eps.shape
    pt, qt = _t(pz, True), _t(qz, True)
    mu, lv, dmu, dlv = pt[:, :C], pt[:, C:], qt[:, :C], qt[:, C:]
    z = _reparam(mu + dmu, lv + dlv, _t(eps), std_scale)
    terms = _kl2_terms(dmu, dlv, mu, lv)
    r = {"z": _n(z), "zs": _n(_t(dec_out) + z), "kl": float(terms.detach().sum() * inv_b), "kl_mag": float(terms.detach().abs().sum() * abs(inv_b))}
    if dzs is not None:
        z1 = _reparam(mu + dmu, lv + dlv, _t(eps), 1.0)
        (gp, gq), (mp, mq) = _two_part_grads([pt, qt], (_t(dzs) * z1).sum(), coef * terms.sum())
        r.update(g_p=gp, g_q=gq, g_p_mag=mp, g_q_mag=mq)
    return r


def linear(X, W, bias=None, scale=1.0, dY=None, addend=None):
    """Y = scale * X W^T + bias; dY given: dX = dL/dX (+ addend), dW = dL/d(scale * W) (the gradient wrt the effective weight),
    db, for L = sum dY Y."""
    Xt, Wt = _t(X, True), _t(W)
    We = (scale * Wt).requires_grad_(True)
    bt = _t(bias, True) if bias is not None else None
    Y = F.linear(Xt, We, bt)
    r = {"Y": _n(Y), "Y_mag": _n(F.linear(Xt.detach().abs(), We.detach().abs(), bt.detach().abs() if bt is not None else None))}
    if dY is not None:
        g = _t(dY)
        (g * Y).sum().backward()
        r["dX"] = _n(Xt.grad) + (np.asarray(addend, np.float64) if addend is not None else 0.0)
        r["dX_mag"] = _n(g.abs() @ We.detach().abs()) + (np.abs(np.asarray(addend, np.float64)) if addend is not None else 0.0)
        r["dW"] = _n(We.grad)
        r["dW_mag"] = _n(g.abs().T @ Xt.detach().abs())
        r["db"] = _n(g.sum(0))
        r["db_mag"] = _n(g.abs().sum(0))
    return r


def _moved(t, axis):
    """[reduced, kept] view of t"""
    if axis is None:
        return t.reshape(-1, 1)
    axis = tuple(np.atleast_1d(axis))
    keep = [a for a in range(t.ndim) if a not in axis]
    return np.transpose(t, list(axis) + keep).reshape(int(np.prod([t.shape[a] for a in axis])), -1)


def f32_sum_error(terms, axis=None, terms32=None):
    """How far a float32 sum of `terms` (float64 array) lands from the float64 sum, relative to the sum of magnitudes, for two
    float32 orders that differ from each other and from the kernels': numpy's pairwise sum over the row-major terms, and up to
    256 strided lanes (term i -> lane i % lanes, at least 64 terms per lane; fewer than 128 terms: one lane) that each add
    their terms strictly one after the other, the lane totals added pairwise.  axis: reduce over these axes (None: all), the worst output is reported.  Returns (error, float64 sums)."""
    t = _moved(np.asarray(terms, np.float64), axis)
    ref = t.sum(0)
    mag = np.maximum(np.abs(t).sum(0), np.finfo(np.float64).tiny)
    t32 = t.astype(np.float32) if terms32 is None else _moved(np.asarray(terms32, np.float32), axis)
    pair = np.ascontiguousarray(t32.T).sum(1, dtype=np.float32).astype(np.float64)      # pairwise needs the contiguous axis
    n, m = t32.shape
    lanes = max(1, min(256, n // 64))           # every lane adds at least 64 terms one after the other, as a kernel's thread does
    pad = np.zeros(((n + lanes - 1) // lanes * lanes, m), np.float32)
    pad[:n] = t32
    lane = np.cumsum(pad.reshape(-1, lanes, m), axis=0, dtype=np.float32)[-1]
    seq = np.ascontiguousarray(lane.T).sum(1, dtype=np.float32).astype(np.float64)
    return float(max(np.max(np.abs(pair - ref) / mag), np.max(np.abs(seq - ref) / mag))), ref
