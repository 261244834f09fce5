"""The temporal pass (csrc/recon_out.hip: recon_temporal_kernel) restated in numpy: the order in which the kernel adds, and the
a-priori bound of any fp32 summation against float64.  numpy only.

Order.  A wave owns WAVE_COLS = 256 contiguous channels of one sample, a block BLOCK_COLS = 1024, for all T time steps; the shares do
not enter the arithmetic, they only say which lanes hold an output.  Every output out[r, n] is ONE chain of fused multiply-adds in fp32
from 0, acc = fma(W[r, t], F[t, n], acc), over t = 0, 1, .. T - 1 ascending (the two k of an MFMA step are t = 2 s and 2 s + 1, in that
order); for odd T the kernel adds 0 * 0 once more, which changes nothing.  Nothing else is added: no partial sums, no combine.

A fused multiply-add is emulated as float32(float64(acc) + float64(w) * float64(x)): the product of two fp32 is exact in float64, the
sum is rounded to float64 and then to float32, which differs from the single rounding of the hardware only when the float64 sum lies
within 2^-53 relative of a float32 tie.  The GPU tests therefore hold the kernel to the bound, not to these bits; the host test holds
the emulation to the same bound.

Bound.  For the stored field F (fp32) and weights W, against q64 = sum_t W[r, t] F[t, n] in float64:
    |q - q64| <= (T + 2) * 2^-24 * sum_t |W[r, t] F[t, n]|
for ANY order of an fp32 summation: at most one rounding per product (none when fused), T - 1 additions, one final rounding, each
2^-24 relative, to first order in 2^-24."""
import numpy as np

WAVE_COLS = 256
BLOCK_COLS = 4 * WAVE_COLS
FLIGHT = {"bf16": 8, "f32": 4}          # steps (of two rows) whose loads are in flight
U = 2.0 ** -24


def emulate(F, W):
    """F [..., T, C] fp32, W [R, T] fp32 -> [..., R, C] fp32 in the kernel's order"""
    F = np.ascontiguousarray(F, np.float32)
    W = np.ascontiguousarray(W, np.float32)
    T = F.shape[-2]
    assert W.ndim == 2 and W.shape[1] == T
    F64, W64 = F.astype(np.float64), W.astype(np.float64)
    acc = np.zeros(F.shape[:-2] + (W.shape[0], F.shape[-1]), np.float32)
    for t in range(T):
        acc = (acc.astype(np.float64) + W64[:, t, None] * F64[..., t, None, :]).astype(np.float32)
    return acc


def reference64(F, W):
    """q64 [..., R, C]: the same sums in float64"""
    return np.asarray(W, np.float64) @ np.asarray(F, np.float64)


def bound(F, W):
    """(T + 2) * 2^-24 * sum_t |W[r, t] F[t, n]|, [..., R, C] float64"""
    T = np.shape(F)[-2]
    return (T + 2) * U * (np.abs(np.asarray(W, np.float64)) @ np.abs(np.asarray(F, np.float64)))


def worst_ratio(q, F, W):
    """max over the outputs of |q - q64| / bound (0 where both are 0); inf if a bound of 0 is missed"""
    err, bnd = np.abs(np.asarray(q, np.float64) - reference64(F, W)), bound(F, W)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bnd > 0, err / bnd, np.where(err > 0, np.inf, 0.0))
    return float(ratio.max()) if ratio.size else 0.0


def mixed_weights(R, T, seed=0):
    """W fp32 [R, T]: both signs, magnitudes over six decades, about an eighth of the entries exactly zero"""
    rng = np.random.default_rng(2003 * R + T + seed)
    W = rng.standard_normal((R, T)) * np.exp(rng.uniform(np.log(1e-3), np.log(1e3), (R, T)))
    W[rng.random((R, T)) < 0.125] = 0.0
    return W.astype(np.float32)
