"""The Gram pass (csrc/recon_out.hip: recon_gram_kernel + recon_gram_finish_kernel) restated in numpy: the order in which the kernel
adds, the a-priori bound of any fp32 summation against float64, and the tolerance of the Eckart-Young identity of a truncated POD.
numpy only.

Values.  d = fl(F - m) in fp32, rounded once, is both operands; a = fl(w * d), rounded once, is the weighted one.  w = None is w = 1
and m = None is m = 0; arrays of ones and zeros give the same bits since 1 * d and F - 0 are exact.

Order.  A block owns CHUNK = 6144 contiguous channels of one sample for all T rows (the share depends on C alone; the four waves of a
block split the TILE PAIRS, not the channels, so there is no share edge inside a block besides the step).  For t <= t' the element
(t, t') is ONE chain of fused multiply-adds in fp32 from 0 over the block's channels, acc = fma(a[t, n], d[t', n], acc) -- the smaller
time index carries the weight -- in steps of STEP = 16 channels at cb; inside a step the order is cb, cb + 8, cb + 1, cb + 9, ..
cb + 7, cb + 15 (the two k of MFMA e are channels cb + e and cb + 8 + e); channels past the end of the share add 0 * 0, which changes
nothing.  The blocks' partials are added in ascending order in float64 and rounded to fp32 once.  (t', t) is the copy of (t, t'): the
result is bitwise symmetric, and its diagonal is a sum of fl(w d) * d >= 0 for w >= 0.

A fused multiply-add is emulated as float32(float64(acc) + float64(a) * float64(d)): the product of two fp32 is exact in float64, the
sum is rounded to float64 and then to float32, which differs from the single rounding of the hardware only when the float64 sum lies
within 2^-53 relative of a float32 tie.  The GPU tests therefore hold the kernel to the bound, not to these bits; the host test holds
the emulation to the same bound.

Bound.  With d = fl(F - m) TAKEN AS GIVEN (the fp32 difference is the quantity whose Gram matrix is asked for), against
G64[t, t'] = sum_n w[n] d[t, n] d[t', n] in float64:
    |G - G64| <= (C + 3) * 2^-24 * sum_n |w[n] d[t, n] d[t', n]|
for ANY order of an fp32 summation: one rounding of w * d, none of the fused product, C - 1 additions and one final rounding, each
2^-24 relative, to first order in 2^-24 -- C + 1 roundings, and the float64 combine of the blocks is far below the remaining 2.

Eckart-Young.  With Y_p = d of condition p, G = sum_p Y_p W Y_p^T = V diag(lam) V^T and P_R the projector on the first R eigenvectors,
sum_p ||Y_p - P_R Y_p||_w^2 = trace((I - P_R) G) = sum_{i > R} lam_i.  What is computed differs in four ways, each bounded below with
nf = GramResult.noise_floor() >= ||G_computed - G||_F, E = trace(G) and T - R = the modes left out:
  (a) the rows are eigenvectors of the COMPUTED matrix: for any orthogonal projector P of rank R, |trace((I - P)(G_c - G))| <=
      ||I - P||_F ||G_c - G||_F = sqrt(T - R) nf;
  (b) negative computed eigenvalues are clamped to 0; G is positive semi-definite, so by Weyl each was >= -nf: (T - R) nf;
  (c) the rows are rounded to fp32, each entry by 2^-24 relative: ||rows - V_R^T||_F <= 2^-24 sqrt(R), the residual moves by at most
      2 ||dV|| ||Y|| to first order and the sum of squares by at most 2 sqrt(lhs) of that: 4 * 2^-24 * sqrt(R) * E covers it (lhs <= E);
  (d) the coefficients carry the error of the temporal pass and of the subtraction of S_r m: with D = sum_p ||rows^T dc_p||_w^2 for
      dc the a-priori bound of the coefficients (tests/temporal_reference.py: (T + 2) 2^-24 sum_t |rows[r, t] F[p, t, n]|, plus
      2^-24 (|c| + 2 |S_r m[n]|) for the product and the difference), the sum of squares moves by at most 2 sqrt(E D) + D.
eckart_young_tol adds the four."""
import numpy as np

STEP = 16
CHUNK = 6144
MAX_T = 256
U = 2.0 ** -24


def _operands(F, w, m):
    F = np.ascontiguousarray(F, np.float32)
    C = F.shape[-1]
    d = F if m is None else (F - np.asarray(m, np.float32).reshape(C)).astype(np.float32)
    a = d if w is None else (np.asarray(w, np.float32).reshape(C) * d).astype(np.float32)
    return a, d


def channel_order(c_lo, c_hi):
    """the channels of the share [c_lo, c_hi) in the order the kernel adds them"""
    order = []
    for cb in range(c_lo, c_hi, STEP):
        for e in range(8):
            for k in (0, 8):
                if cb + k + e < c_hi:
                    order.append(cb + k + e)
    return order


def emulate(F, w=None, m=None):
    """F [..., T, C] fp32, w [C] or None, m [C] or None -> [..., T, T] fp32 in the kernel's order"""
    a, d = _operands(F, w, m)
    T, C = d.shape[-2:]
    assert T <= MAX_T
    a64, d64 = a.astype(np.float64), d.astype(np.float64)
    total = np.zeros(d.shape[:-2] + (T, T), np.float64)
    for c_lo in range(0, C, CHUNK):
        acc = np.zeros(total.shape, np.float32)
        for n in channel_order(c_lo, min(C, c_lo + CHUNK)):
            acc = (acc.astype(np.float64) + a64[..., :, None, n] * d64[..., None, :, n]).astype(np.float32)
        total += acc          # ascending share order, float64
    g = total.astype(np.float32)
    up = np.triu(np.ones((T, T), bool))
    return np.where(up, g, np.swapaxes(g, -1, -2))          # (t', t) is the copy of (t, t'), t <= t'


def reference64(F, w=None, m=None):
    """G64 [..., T, T]: sum_n w d_t d_t' in float64 with d the fp32 difference"""
    _, d = _operands(F, None, m)
    d = d.astype(np.float64)
    wd = d if w is None else d * np.asarray(w, np.float64)
    return wd @ np.swapaxes(d, -1, -2)


def bound(F, w=None, m=None):
    """(C + 3) * 2^-24 * sum_n |w d_t d_t'|, [..., T, T] float64"""
    _, d = _operands(F, None, m)
    d = np.abs(d.astype(np.float64))
    wd = d if w is None else d * np.abs(np.asarray(w, np.float64))
    return (d.shape[-1] + 3) * U * (wd @ np.swapaxes(d, -1, -2))


def worst_ratio(G, F, w=None, m=None):
    """max over the outputs of |G - G64| / bound (0 where both are 0); inf if a bound of 0 is missed"""
    err, bnd = np.abs(np.asarray(G, np.float64) - reference64(F, w, m)), bound(F, w, m)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bnd > 0, err / bnd, np.where(err > 0, np.inf, 0.0))
    return float(ratio.max()) if ratio.size else 0.0


def coefficient_bound(rows, F, coeff, m=None):
    """dc [P, R, N] float64: the a-priori bound of coefficients[p, r, n] = temporal(rows)[p, r, n] - S_r m[n] in fp32, (d) above"""
    rows64, F64 = np.asarray(rows, np.float64), np.asarray(F, np.float64)
    T = rows64.shape[1]
    dc = (T + 2) * U * (np.abs(rows64) @ np.abs(F64)) + U * np.abs(np.asarray(coeff, np.float64))
    if m is not None:
        dc = dc + 2 * U * np.abs(rows64.sum(axis=1))[None, :, None] * np.abs(np.asarray(m, np.float64))[None, None, :]
    return dc


def eckart_young_tol(noise_floor, energy, T, R, rows, dc, w=None):
    """the tolerance of sum_p ||Y_p - reconstruct_R(p)||_w^2 = sum_{i > R} eigenvalues, (a) to (d) above; dc = coefficient_bound"""
    spread = np.abs(np.asarray(rows, np.float64)).T @ dc          # [P, T, N]: |rows^T| dc
    if w is not None:
        spread = spread * np.sqrt(np.asarray(w, np.float64))
    D = float((spread ** 2).sum())
    return (np.sqrt(T - R) + (T - R)) * noise_floor + 4 * U * np.sqrt(R) * energy + 2 * np.sqrt(energy * D) + D


def residual_energy(F, recon, w=None, m=None):
    """sum_p ||Y_p - (recon_p - m)||_w^2 in float64, Y = the fp32 difference F - m"""
    _, d = _operands(F, None, m)
    r = d.astype(np.float64) - (np.asarray(recon, np.float64) - (0.0 if m is None else np.asarray(m, np.float32).astype(np.float64)))
    r2 = r ** 2
    return float((r2 if w is None else r2 * np.asarray(w, np.float64)).sum())


def mixed_weights(C, seed=0):
    """w fp32 [C] >= 0: magnitudes over four decades, about an eighth of the entries exactly zero"""
    rng = np.random.default_rng(3001 * C + seed)
    w = np.exp(rng.uniform(np.log(1e-2), np.log(1e2), C))
    w[rng.random(C) < 0.125] = 0.0
    return w.astype(np.float32)


def mixed_offset(F, seed=0):
    """m fp32 [C]: the mean over everything but the channel, perturbed, so that F - m cancels"""
    F = np.asarray(F, np.float32)
    rng = np.random.default_rng(17 + seed)
    mean = F.reshape(-1, F.shape[-1]).mean(axis=0)
    return (mean * (1.0 + 0.1 * rng.standard_normal(F.shape[-1]))).astype(np.float32)
