"""The exceedance pass (csrc/recon_out.hip: recon_exceed_kernel) restated in numpy: a float32 loop over t on a stored field F, and
an independent brute force over Python lists.  numpy only.

Contract.  For a stored field F [..., T, C] fp32, levels [L, C] fp32 and a side, with e[t] = (F[t] > level) above and
(F[t] < level) below (strict; a NaN exceeds nothing), per (level, channel):
    count   = the number of t with e[t]
    first   = the smallest t with e[t], -1 if none
    last    = the largest t with e[t], -1 if none
    longest = the length of the longest run of consecutive t with e[t], 0 if none
    runs    = the number of t with e[t] and (t == 0 or not e[t - 1]), the number of maximal runs
    excess  = s after: s = +0.0; for t ascending, where e[t]: s = fl(s + d[t]), d[t] = fl(F[t] - level) above, fl(level - F[t]) below
Everything is integer apart from excess, which is one fp32 chain in a fixed order: the kernel is held to these bits.

Shares.  A thread of the kernel owns 8 channels of one sample for all T, a wave WAVE_COLS = 512 contiguous channels, a block
BLOCK_COLS = 2048; the y rows of FLIGHT steps are in flight.  None of it enters the arithmetic; the tests take their shapes from it.

Bound.  Against s64 = the sum in float64 of the exact differences F[t] - level over the exceeding steps:
    |excess - s64| <= (T + 1) * 2^-24 * sum_t |d[t]|
-- one rounding per difference and at most T - 1 additions (the first, to +0.0, is exact), each 2^-24 relative, to first order."""
import itertools

import numpy as np

WAVE_COLS = 512
BLOCK_COLS = 4 * WAVE_COLS
FLIGHT = {"bf16": 4, "f32": 2}          # steps whose loads are in flight
MAX_LEVELS = 4
STATS = ("count", "first", "last", "longest", "runs")          # the planes of stats, in this order
U = 2.0 ** -24


def exceeds(F, levels, side="above"):
    """e [..., T, L, C] bool"""
    F = np.asarray(F, np.float32)[..., :, None, :]
    lv = np.asarray(levels, np.float32)
    return F > lv if side == "above" else F < lv


def emulate(F, levels, side="above"):
    """F [..., T, C] fp32, levels [L, C] fp32 -> (stats [..., 5, L, C] int32 in the order of STATS, excess [..., L, C] fp32)"""
    assert side in ("above", "below")
    F = np.ascontiguousarray(F, np.float32)
    lv = np.ascontiguousarray(levels, np.float32)
    T, C = F.shape[-2:]
    assert lv.ndim == 2 and lv.shape[1] == C
    shape = F.shape[:-2] + lv.shape
    count, longest, runs, cur = (np.zeros(shape, np.int32) for _ in range(4))
    first, last = (np.full(shape, -1, np.int32) for _ in range(2))
    s = np.zeros(shape, np.float32)
    for t in range(T):
        x = F[..., t, None, :]
        e = x > lv if side == "above" else x < lv
        with np.errstate(invalid="ignore", over="ignore"):
            d = (x - lv if side == "above" else lv - x).astype(np.float32)          # float32 operands: rounded once
            s = np.where(e, (s + d).astype(np.float32), s)
        runs += e & (cur == 0)
        cur = np.where(e, cur + 1, 0).astype(np.int32)
        count += e
        longest = np.maximum(longest, cur)
        first = np.where(e & (first < 0), t, first).astype(np.int32)
        last = np.where(e, t, last).astype(np.int32)
    return np.stack([count, first, last, longest, runs], axis=-3).astype(np.int32), s


def brute(e):
    """(count, first, last, longest, runs) of one 0 / 1 history, by itertools.groupby over a Python list"""
    e = [bool(v) for v in e]
    on = [len(list(g)) for k, g in itertools.groupby(e) if k]
    where = [t for t, v in enumerate(e) if v]
    return (sum(on), where[0] if where else -1, where[-1] if where else -1, max(on) if on else 0, len(on))


def brute_stats(E):
    """E [..., T, L, C] bool -> stats [..., 5, L, C] int32 by brute() on every history"""
    E = np.asarray(E, bool)
    lead, (T, L, C) = E.shape[:-3], E.shape[-3:]
    out = np.empty(lead + (5, L, C), np.int32)
    for idx in np.ndindex(*lead):
        for l in range(L):
            for c in range(C):
                out[idx + (slice(None), l, c)] = brute(E[idx + (slice(None), l, c)].tolist())
    return out


def excess64(F, levels, side="above"):
    """(s64, sum_t |d[t]|) [..., L, C] float64: the exact differences over the exceeding steps, summed in float64"""
    F64 = np.asarray(F, np.float32).astype(np.float64)[..., :, None, :]
    lv = np.asarray(levels, np.float32).astype(np.float64)
    d = np.where(exceeds(F, levels, side), F64 - lv if side == "above" else lv - F64, 0.0)
    return d.sum(axis=-3), np.abs(d).sum(axis=-3)


def worst_ratio(excess, F, levels, side="above"):
    """max over the outputs of |excess - s64| / ((T + 1) 2^-24 sum |d|) (0 where both are 0); inf if a bound of 0 is missed"""
    T = np.shape(F)[-2]
    s64, mag = excess64(F, levels, side)
    err, bnd = np.abs(np.asarray(excess, np.float64) - s64), (T + 1) * U * mag
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bnd > 0, err / bnd, np.where(err > 0, np.inf, 0.0))
    return float(ratio.max()) if ratio.size else 0.0


def kernel_levels(F):
    """The four levels of the kernel tests from a stored field F [B, T, C], fp32 [4, C]: the per-node median over (sample, time)
    (many runs), a stored element itself (the strict tie: sample 0's step T // 2), the node's maximum (never exceeded above) and
    nextafter(the node's minimum, -inf) (always exceeded above)."""
    F = np.asarray(F, np.float32)
    flat = F.reshape(-1, F.shape[-1])
    med = np.sort(flat, axis=0)[flat.shape[0] // 2]          # an element of F, not an average of two
    return np.stack([med, F[0, F.shape[1] // 2], flat.max(axis=0), np.nextafter(flat.min(axis=0), np.float32(-np.inf))]).astype(np.float32)
