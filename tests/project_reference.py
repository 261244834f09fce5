"""The project pass (csrc/recon_out.hip: recon_project_kernel, recon_project_finish_kernel) restated in numpy: the order in which the
kernel adds, and the a-priori bound of any fp32 summation against float64.  numpy only.

Order.  The channels are cut into shares that depend on C alone: a block owns CHUNK = 4096 channels, its four waves WAVE_COLS = 1024
contiguous ones each.  A wave runs ONE chain of fused multiply-adds per output, acc = fma(x[n], w[n], acc) in fp32, over its channels
in steps of 16: within the step at cb the order is cb, cb + 8, cb + 1, cb + 9, .. cb + 7, cb + 15 (the two k of an MFMA, then the next
MFMA); channels past C are left out (the kernel adds 0 * 0 there).  The four waves are added in wave order in fp32, the blocks in
ascending order in float64, and the sum is rounded to fp32 once.

A fused multiply-add is emulated as float32(float64(acc) + float64(x) * float64(w)): the product of two fp32 is exact in float64, the
sum is rounded to float64 and then to float32, which differs from the single rounding of the hardware only when the float64 sum lies
within 2^-53 relative of a float32 tie.  The GPU tests therefore hold the kernel to the bound, not to these bits; the host test holds
the emulation to the same bound.

Bound.  For the stored field F (fp32) and weights W, against q64 = sum_n W[r, n] F[n] in float64:
    |q - q64| <= (C + 2) * 2^-24 * sum_n |W[r, n] F[n]|
for ANY order of an fp32 summation: at most one rounding per product (none when fused), C - 1 additions, one final rounding, each
2^-24 relative, to first order in 2^-24; the float64 combine only tightens it."""
import numpy as np

WAVE_COLS = 1024
CHUNK = 4 * WAVE_COLS
U = 2.0 ** -24


def chain_order(c_lo, c_hi):
    """the channels of a wave's share [c_lo, c_hi) in the order its chain takes them"""
    order = []
    for cb in range(c_lo, c_hi, 16):
        for e in range(8):
            order += [c for c in (cb + e, cb + 8 + e) if c < c_hi]
    return order


def emulate(F, W):
    """F [..., C] fp32, W [R, C] fp32 -> [..., R] fp32 in the kernel's order"""
    F = np.ascontiguousarray(F, np.float32)
    W = np.ascontiguousarray(W, np.float32)
    C = F.shape[-1]
    assert W.ndim == 2 and W.shape[1] == C
    F64, W64 = F.astype(np.float64), W.astype(np.float64)
    total = np.zeros(F.shape[:-1] + (W.shape[0],), np.float64)
    for b_lo in range(0, C, CHUNK):
        waves = []
        for wv in range(4):
            c_lo = b_lo + wv * WAVE_COLS
            acc = np.zeros(total.shape, np.float32)
            for n in chain_order(c_lo, min(C, c_lo + WAVE_COLS)):
                acc = (acc.astype(np.float64) + F64[..., n, None] * W64[:, n]).astype(np.float32)
            waves.append(acc)
        total = total + (((waves[0] + waves[1]) + waves[2]) + waves[3]).astype(np.float64)
    return total.astype(np.float32)


def reference64(F, W):
    """q64 [..., R]: the same sums in float64"""
    return np.asarray(F, np.float64) @ np.asarray(W, np.float64).T


def bound(F, W):
    """(C + 2) * 2^-24 * sum_n |W[r, n] F[n]|, [..., R] float64"""
    C = np.shape(F)[-1]
    return (C + 2) * U * (np.abs(np.asarray(F, np.float64)) @ np.abs(np.asarray(W, np.float64)).T)


def worst_ratio(q, F, W):
    """max over the outputs of |q - q64| / bound (0 where both are 0); inf if a bound of 0 is missed"""
    err, bnd = np.abs(np.asarray(q, np.float64) - reference64(F, W)), bound(F, W)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bnd > 0, err / bnd, np.where(err > 0, np.inf, 0.0))
    return float(ratio.max()) if ratio.size else 0.0


def mixed_weights(R, C, seed=0):
    """W fp32 [R, C]: both signs, magnitudes over six decades, about an eighth of the entries exactly zero"""
    rng = np.random.default_rng(1009 * R + C + seed)
    W = rng.standard_normal((R, C)) * np.exp(rng.uniform(np.log(1e-3), np.log(1e3), (R, C)))
    W[rng.random((R, C)) < 0.125] = 0.0
    return W.astype(np.float32)
