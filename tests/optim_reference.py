"""Plain float64 statements of the operations csrc/optim.hip implements, in the kernels' internal layout: a weight is
[taps][rows][cols] (cols contiguous), u is [rows], v is [taps*cols] in (tap, col) order.  The matrix spectral norm sees is
rows x (taps*cols): row r holds W[:, r, :] flattened in (tap, col) order.  Inputs are numpy arrays holding the numbers the
kernel reads (already rounded to fp32 / bf16 where it reads those); everything is computed in float64.  No GPU is touched.

tests/test_optim_reference_host.py pins this file to oracle/vae_oracle.py, torch.optim.AdamW and torch.nn.utils.spectral_norm;
tests/test_lc_param_reference_host.py pins the plain [rows][cols] use of it (taps = 1), the conv-weight packing and the clip
coefficient to torch in float64."""
import numpy as np
import torch

SN_EPS = 1e-12      # torch.nn.functional.normalize's clamp, as spectral_norm passes it


def f64(a):
    return np.asarray(a, np.float64)


def bf16_round(a):
    """round to nearest even to bfloat16, returned as float32 values"""
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(torch.bfloat16).to(torch.float32).numpy()


def bf16_bits(a):
    """the uint16 patterns of bf16_round(a)"""
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)


# ---- layout: reference Conv1d / Linear weight [Cout][Cin][K] (Linear: K = 1) <-> internal [K][Cout][Cin] ----
def weight_to_internal(W):
    W = np.asarray(W)
    if W.ndim == 2:
        W = W[:, :, None]
    return np.ascontiguousarray(W.transpose(2, 0, 1))


def weight_from_internal(Wi):
    return np.ascontiguousarray(np.asarray(Wi).transpose(1, 2, 0))


def v_to_internal(v, cin, k):
    """the reference's v runs over W.reshape(Cout, Cin*K), i.e. in (cin, k) order"""
    return np.ascontiguousarray(np.asarray(v).reshape(cin, k).T).ravel()


def v_from_internal(vi, cin, k):
    return np.ascontiguousarray(np.asarray(vi).reshape(k, cin).T).ravel()


# ---- spectral norm ----
def wt_u(W, u):
    """t = W^T u, [taps*cols]; also the sum of the magnitudes of each output's terms"""
    W, u = f64(W), f64(u)
    terms = W * u[None, :, None]
    return terms.sum(1).ravel(), np.abs(terms).sum(1).ravel()


def w_v(W, v):
    """s = W v, [rows]; also the sum of the magnitudes of each output's terms"""
    W = f64(W)
    terms = W * f64(v).reshape(W.shape[0], 1, W.shape[2])
    return terms.sum((0, 2)), np.abs(terms).sum((0, 2))


def normalize(x):
    x = f64(x)
    return x / max(float(np.sqrt((x * x).sum())), SN_EPS)


def power_iteration(W, u, v, train, Wv=None):
    """One legacy spectral-norm step.  train: t = W^T u, v = t / max(|t|, 1e-12), s = Wv v, u = s / max(|s|, 1e-12), sigma = u.s;
    eval: sigma = u.(Wv v), u and v untouched.  Wv: the operand of the W v pass (the master, or the bf16 copy as float values)."""
    W, u, v = f64(W), f64(u), f64(v)
    Wv = W if Wv is None else f64(Wv)
    r = {}
    if train:
        r["t"], r["t_mag"] = wt_u(W, u)
        v = normalize(r["t"])
    r["s"], r["s_mag"] = w_v(Wv, v)
    if train:
        u = normalize(r["s"])
    r.update(u=u, v=v, sigma=float((u * r["s"]).sum()))
    return r


def grad_dot(G, W):
    """<G, W> and the sum of the magnitudes of its terms"""
    p = f64(G) * f64(W)
    return float(p.sum()), float(np.abs(p).sum())


def chain_rule(G, cdot, inv_sigma, u, v):
    """Gradient wrt the original weight of L(W / sigma), sigma = u^T W v with u, v constants:
    (G - <G, W_eff> u v^T) / sigma, where G = dL/dW_eff and cdot = <G, W_eff> = <G, W> / sigma."""
    G = f64(G)
    uv = f64(u)[None, :, None] * f64(v).reshape(G.shape[0], 1, G.shape[2])
    return (G - float(cdot) * uv) * float(inv_sigma)


def sn_backward(G, W, sigma, u, v):
    return chain_rule(G, grad_dot(G, W)[0] / sigma, 1.0 / sigma, u, v)


# ---- AdamW ----
def adamw(p, g, m, v, lr, step, wd, eps=1e-8, b1=0.9, b2=0.999, gscale=None, bc1=None, bc2sqrt=None):
    """torch.optim.AdamW in the order oracle/vae_oracle.py::adamw_step applies it: decay, moments, update.  step is 1-based; m, v
    are the incoming moments.  gscale (the clip coefficient) multiplies the gradient after the norm is taken.  bc1 / bc2sqrt
    override the bias corrections (a caller that models a launch passes the float32 values the launch got).
    Returns a dict: p, m, v, update (what was subtracted from p * decay), decay, gnorm_sq (before gscale)."""
    p, g, m, v = f64(p), f64(g), f64(m), f64(v)
    gnorm_sq = float((g * g).sum())
    if gscale is not None:
        g = g * float(gscale)
    bc1 = 1.0 - b1 ** step if bc1 is None else float(bc1)
    bc2sqrt = np.sqrt(1.0 - b2 ** step) if bc2sqrt is None else float(bc2sqrt)
    decay = 1.0 - lr * wd
    pd = p * decay
    m = m * b1 + (1.0 - b1) * g
    v = v * b2 + (1.0 - b2) * g * g
    denom = np.sqrt(v) / bc2sqrt + eps
    upd = (lr / bc1) * (m / denom)
    return dict(p=pd - upd, m=m, v=v, update=upd, decay=decay, denom=denom, g=g, gnorm_sq=gnorm_sq)


# ---- compute-dtype copies ----
def wct_copy(p):
    """wct[taps-1-tap][c][r] = p[tap][r][c]"""
    p = np.asarray(p)
    return np.ascontiguousarray(p[::-1].transpose(0, 2, 1))


# ---- the latent conditioner's parameter side (include/sgvae_ops.h) ----
def as_taps(W):
    """a plain [rows][cols] matrix in the layout above (one tap)"""
    W = np.asarray(W)
    return W.reshape(1, W.shape[0], W.shape[1])


def conv_weight_pack(w, align=8):
    """reference Conv2d weight [Cout][Cin][KH][KW] -> the GEMM layout [Cout][(kh*KW + kw)*Cin + ci], rows zero-padded to a
    multiple of `align` columns; written as loops on purpose (the host test pins it to permute + reshape)"""
    w = np.asarray(w)
    cout, cin, kh_, kw_ = w.shape
    k = kh_ * kw_ * cin
    out = np.zeros((cout, (k + align - 1) // align * align), w.dtype)
    for co in range(cout):
        for ci in range(cin):
            for kh in range(kh_):
                for kw in range(kw_):
                    out[co, (kh * kw_ + kw) * cin + ci] = w[co, ci, kh, kw]
    return out


def conv_weight_unpack(packed, shape):
    """the inverse: the pad columns are not read"""
    packed = np.asarray(packed)
    cout, cin, kh_, kw_ = shape
    w = np.empty(shape, packed.dtype)
    for co in range(cout):
        for ci in range(cin):
            for kh in range(kh_):
                for kw in range(kw_):
                    w[co, ci, kh, kw] = packed[co, (kh * kw_ + kw) * cin + ci]
    return w


def clip_coef(total_norm, max_norm, eps=1e-6):
    """torch.nn.utils.clip_grad_norm_: the factor every gradient is multiplied by, min(1, max_norm / (total_norm + 1e-6))"""
    return min(1.0, float(max_norm) / (float(total_norm) + eps))
