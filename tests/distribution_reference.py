"""numpy float32 emulation of the distribution pass (csrc/recon_out.hip: recon_hist_kernel): the contract of its
arithmetic, one np.float32 operation -- one rounding -- per operation of the kernel.

For a member's value x (an fp32 array [T, N]), K bins and bounds lo, hi (fp32 [T, N]):
    invw = hi > lo ? (float)K / (hi - lo) : 0.0f
    row  = 0 if x < lo, K + 1 if x > hi, else 1 + min((int)((x - lo) * invw), K - 1)          (truncation; the product is >= 0 there)
    counts[row][t][n] += 1                                                                    (int32 [K + 2, T, N])
So x == hi is in the last bin, with hi == lo a value equal to them is in bin 1, and every column of counts sums to the number of
members.  The pass only adds: an empty state is zeros.  NaN is not specified.

quantile() is DistributionResult.quantile's arithmetic in numpy float32: r = max(ceil(q count), 1); j the first row at which the
running sum of a column reaches r; lo for j = 0, hi for j = K + 1, else min(lo + (j - 1 + (r - sum below j) / counts[j]) (hi - lo) / K, hi).

The bound of the quantile, bound().  Take lo / hi as the members' own extrema, so that rows 0 and K + 1 are empty, and let x_r be the
r-th smallest member, j its bin, w = (hi - lo) / K and u = 2^-24.  In exact arithmetic x_r lies in [lo + (j - 1) w, lo + j w] and so
does the interpolated value, whose position (r - sum below j) / counts[j] is in (0, 1]: they are at most w apart, and exactly w where
x_r sits alone on the lower edge of its bin.  Rounding adds rho: the rule's s = (x - lo) * invw carries four roundings (x - lo,
hi - lo, the division, the product), a relative 4 u, so a member the rule puts in bin j may lie 4 u j w outside it; the
interpolation's difference, product and division add 3 u j w, its last sum half an ulp of the result:
    |quantile - x_r| <= w + rho,   rho <= 7 u (hi - lo) + ulp(max(|lo|, |hi|)) / 2.
With u m < ulp(m) for every m, rho <= 4 ulp(max(|lo|, |hi|)) is certain where hi - lo <= max(|lo|, |hi|) / 2 (a response away from
zero); for a column around zero, hi - lo up to 2 max(|lo|, |hi|), the certain figure is 14.5 ulp with every rounding at its worst at once
and on an edge.  bound() is w + 4 ulp as the project's tests assert it; the worst err / bound they see is 0.9999998, w itself.
A degenerate column, hi == lo, gives lo exactly.  numpy only."""
import numpy as np


def empty_counts(K, T, N):
    return np.zeros((K + 2, T, N), np.int32)


def rows(x, lo, hi, K):
    """the row of counts each element of x [.., T, N] falls into (int64), lo / hi [T, N], all float32"""
    x, lo, hi = np.asarray(x), np.asarray(lo), np.asarray(hi)
    assert x.dtype == np.float32 and lo.dtype == np.float32 and hi.dtype == np.float32
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        width = hi - lo
        invw = np.where(hi > lo, np.float32(K) / np.where(hi > lo, width, np.float32(1)), np.float32(0)).astype(np.float32)
        s = (x - lo) * invw
        assert s.dtype == np.float32
        inside = 1 + np.minimum(np.trunc(np.where((x < lo) | (x > hi), 0, s)).astype(np.int64), K - 1)
    return np.where(x < lo, 0, np.where(x > hi, K + 1, inside))


def update(F, lo, hi, K, counts=None):
    """Adds the members F [B, T, N] (float32) to `counts` (int32 [K + 2, T, N]; None: zeros) and returns the new counts; the argument
    is left alone."""
    F = np.asarray(F)
    assert F.dtype == np.float32 and F.ndim == 3
    B, T, N = F.shape
    c = empty_counts(K, T, N) if counts is None else np.array(counts, copy=True)
    assert c.shape == (K + 2, T, N) and c.dtype == np.int32
    tt, nn = np.meshgrid(np.arange(T), np.arange(N), indexing="ij")
    for b in range(B):
        np.add.at(c, (rows(F[b], lo, hi, K), tt, nn), 1)
    return c


def rank(q, count):
    return max(int(np.ceil(np.float64(q) * int(count))), 1)


def quantile(counts, lo, hi, q, count):
    """the q-quantile [T, N] float32 of a column's `count` members from its counts [K + 2, T, N]"""
    counts, lo, hi = np.asarray(counts), np.asarray(lo, np.float32), np.asarray(hi, np.float32)
    K = counts.shape[0] - 2
    r = rank(q, count)
    cum = counts.astype(np.int64).cumsum(0)
    j = np.minimum((cum < r).sum(0), K + 1)
    take = lambda a, i: np.take_along_axis(a, i[None], 0)[0]
    below = np.where(j > 0, take(cum, np.maximum(j - 1, 0)), 0)
    with np.errstate(invalid="ignore", divide="ignore"):
        pos = (j - 1).astype(np.float32) + (r - below).astype(np.float32) / take(counts, j).astype(np.float32)
        v = np.minimum(lo + pos * (hi - lo) / np.float32(K), hi)
    assert v.dtype == np.float32
    return np.where(j == 0, lo, np.where(j == K + 1, hi, v)).astype(np.float32)


def bound(lo, hi, K):
    """w + 4 ulp(max(|lo|, |hi|)) in float64 (see above)"""
    lo, hi = np.asarray(lo, np.float32), np.asarray(hi, np.float32)
    w = (hi.astype(np.float64) - lo.astype(np.float64)) / K
    return w + 4.0 * np.spacing(np.maximum(np.abs(lo), np.abs(hi))).astype(np.float64)


def order_statistic(F, q):
    """sort(F, axis 0)[ceil(q M) - 1]: the exact q-quantile of the M members F [M, T, N]"""
    F = np.asarray(F)
    return np.sort(F, axis=0)[rank(q, F.shape[0]) - 1]
