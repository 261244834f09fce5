"""The cycles pass (csrc/recon_out.hip: recon_cycles_kernel) restated in numpy: a vectorised float32 loop over t on a stored field F,
two independent walks over Python lists, and the float64 sums with their a-priori bounds.  numpy only.

Contract (csrc/sgv_ew.h: ReconCycles; include/sgvae.h: sgv_cycles_out).  x[t] is the stored value F[..., t, n], h = gate[n] >= 0,
m = exponent, an integer in [1, 8], fl() one fp32 rounding.  Every difference is formed from the stored value and rounded on its
own; every product of the power and every accumulation likewise; nothing is contracted into an fma.  All comparisons are strict.

Rates, for t = 1 .. T - 1, with r[t] = fl(x[t] - x[t-1]):
    rise = max r[t], fall = min r[t]; rise_when, fall_when the step t of each, the smallest on a tie (strict > / < updates starting
    from r[1]); path = s after s = +0.0; s = fl(s + |r[t]|) for t ascending.  T = 1: rise = fall = path = +0.0, both steps -1.

Turns, a machine of three states per node, dir in {0, +1, -1}, from dir = 0 and hi = lo = x[0]; for t = 1 .. T - 1, x = x[t]:
    dir = 0:  if fl(x - lo) > h, a valley is confirmed: last = lo, cand = x, dir = +1, reversals += 1;
              else if fl(hi - x) > h, a peak is confirmed: last = hi, cand = x, dir = -1, reversals += 1;
              else hi = max(hi, x) and lo = min(lo, x) (x replaces hi where x > hi, lo where x < lo).
              Both conditions cannot hold for h >= 0; the order above is the definition.  The first turning point carries no range.
    dir = +1: if x > cand, cand = x; else if fl(cand - x) > h, a peak is confirmed: R = fl(cand - last) is counted, last = cand,
              cand = x, dir = -1, reversals += 1.
    dir = -1: if x < cand, cand = x; else if fl(x - cand) > h, a valley is confirmed: R = fl(last - cand) is counted, last = cand,
              cand = x, dir = +1, reversals += 1.
    counted:  range_sum = fl(range_sum + R); range_max = R if R > range_max; damage = fl(damage + P) with P = R and then m - 1
              times P = fl(P * R).  All three start from +0.0.
    open, the unfinished excursion at the end: fl(hi - lo) at dir = 0, fl(cand - last) at +1, fl(last - cand) at -1.
With h = 0 every strict local extremum of the history with its plateaus collapsed is a turning point; a constant history has
reversals = 0 and everything +0.0; with h above the node's peak-to-peak reversals = 0 and open = fl(max - min); the counted ranges
(half cycles) number max(reversals - 1, 0).

Outputs: reversals int32 [..., C]; ranges fp32 [..., 4, C] = range_sum, range_max, damage, open; rate_when int32 [..., 2, C] =
rise_when, fall_when; rates fp32 [..., 3, C] = rise, fall, path.

Shares.  A thread of the kernel owns 8 channels of one sample for all T, a wave WAVE_COLS = 512 contiguous channels, a block
BLOCK_COLS = 2048; the y rows of FLIGHT steps are in flight.  None of it enters the arithmetic; the tests take their shapes from it.

Bounds, first order, against float64 sums of rho = the exact differences of the fp32 values taken at the decisions fp32 makes, K the
number of counted ranges:
    |path - sum |rho||     <= (T + 1) 2^-24 sum |rho|      one rounding per difference, at most T - 2 additions that round
    |range_sum - sum rho|  <= (K + 1) 2^-24 sum rho        one rounding per range, K - 1 additions
    |damage - sum rho^m|   <= (2 m + K) 2^-24 sum rho^m    m roundings per power (the range and m - 1 products) and m times the
                                                           range's own, K - 1 additions"""
import itertools

import numpy as np

WAVE_COLS = 512
BLOCK_COLS = 4 * WAVE_COLS
FLIGHT = {"bf16": 4, "f32": 2}          # steps whose loads are in flight
MAX_EXPONENT = 8
MAX_T = 65535
RANGES = ("range_sum", "range_max", "damage", "open")          # the planes of ranges, in this order
RATES = ("rise", "fall", "path")                               # the planes of rates
U = 2.0 ** -24
f32 = np.float32


def _power(R, m):
    P = R
    for _ in range(m - 1):
        P = (P * R).astype(f32)
    return P


def emulate(F, gate, exponent=3, sums64=False):
    """F [..., T, C] fp32, gate [C] fp32 -> dict(reversals, ranges, rate_when, rates) as in the module's docstring; with sums64 also
    path64, range64, damage64 [..., C] float64 (the sums of the exact differences at the decisions made here) and K = the ranges."""
    F = np.ascontiguousarray(F, f32)
    h = np.ascontiguousarray(gate, f32)
    m = int(exponent)
    T, C = F.shape[-2:]
    assert h.shape == (C,) and 1 <= m <= MAX_EXPONENT and 1 <= T <= MAX_T
    shape = F.shape[:-2] + (C,)
    zeros = lambda dt=f32: np.zeros(shape, dt)
    x0 = F[..., 0, :]
    a, b = x0.copy(), x0.copy()          # hi / cand, lo / last
    d, rev = zeros(np.int32), zeros(np.int32)
    rsum, rmax, dmg = zeros(), zeros(), zeros()
    prev = x0.copy()
    rise, fall, path = zeros(), zeros(), zeros()
    rwhen, fwhen = np.full(shape, -1, np.int32), np.full(shape, -1, np.int32)
    path64, range64, damage64 = zeros(np.float64), zeros(np.float64), zeros(np.float64)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        for t in range(1, T):
            x = F[..., t, :]
            # the rates
            r = (x - prev).astype(f32)
            up, dn = (r > rise) | (t == 1), (r < fall) | (t == 1)
            rise, fall = np.where(up, r, rise), np.where(dn, r, fall)
            rwhen, fwhen = np.where(up, t, rwhen).astype(np.int32), np.where(dn, t, fwhen).astype(np.int32)
            path = (path + np.abs(r)).astype(f32)
            path64 += np.abs(x.astype(np.float64) - prev.astype(np.float64))
            prev = x
            # the turns
            z, p, n = d == 0, d == 1, d == -1
            up0 = z & ((x - b).astype(f32) > h)
            dn0 = z & ~up0 & ((a - x).astype(f32) > h)
            ext = (p & (x > a)) | (n & (x < a))
            peak = p & ~ext & ((a - x).astype(f32) > h)
            vall = n & ~ext & ((x - a).astype(f32) > h)
            trig = peak | vall
            R = np.where(peak, (a - b).astype(f32), (b - a).astype(f32))
            rsum = np.where(trig, (rsum + R).astype(f32), rsum)
            rmax = np.where(trig & (R > rmax), R, rmax)
            dmg = np.where(trig, (dmg + _power(R, m)).astype(f32), dmg)
            R64 = np.where(trig, np.abs(a.astype(np.float64) - b.astype(np.float64)), 0.0)
            range64 += R64
            damage64 += R64 ** m
            turn = up0 | dn0 | trig
            nb = np.where(up0, b, np.where(dn0 | trig, a, np.where(z & (x < b), x, b)))
            na = np.where(turn | ext | (z & (x > a)), x, a)
            a, b = na.astype(f32), nb.astype(f32)
            d = np.where(up0 | vall, 1, np.where(dn0 | peak, -1, d)).astype(np.int32)
            rev = rev + turn
        opn = np.where(d == -1, (b - a).astype(f32), (a - b).astype(f32))
    out = dict(reversals=rev.astype(np.int32), ranges=np.stack([rsum, rmax, dmg, opn], axis=-2).astype(f32),
               rate_when=np.stack([rwhen, fwhen], axis=-2).astype(np.int32), rates=np.stack([rise, fall, path], axis=-2).astype(f32))
    if sums64:
        out.update(path64=path64, range64=range64, damage64=damage64, K=np.maximum(rev - 1, 0))
    return out


def _sums(ranges, m):
    """(range_sum, range_max, damage) of a list of fp32 ranges, accumulated in their order as the contract says"""
    rsum = rmax = dmg = f32(0)
    for R in ranges:
        P = R
        for _ in range(m - 1):
            P = f32(P * R)
        rsum, dmg = f32(rsum + R), f32(dmg + P)
        if R > rmax:
            rmax = R
    return rsum, rmax, dmg


def brute0(history, exponent=3):
    """gate = 0, independent of emulate: the runs of equal values collapsed (itertools.groupby), the turning points are the first
    element and the strict interior extrema -> (reversals, ranges, range_sum, range_max, damage, open)"""
    v = [f32(k) for k, _ in itertools.groupby(float(x) for x in history)]
    if len(v) < 2:
        return 0, [], f32(0), f32(0), f32(0), f32(0)
    tp = [v[0]] + [v[i] for i in range(1, len(v) - 1) if (v[i] > v[i - 1] and v[i] > v[i + 1]) or (v[i] < v[i - 1] and v[i] < v[i + 1])]
    ranges = [f32(max(p, q) - min(p, q)) for p, q in zip(tp, tp[1:])]
    opn = f32(max(v[-1], tp[-1]) - min(v[-1], tp[-1]))
    return (len(tp), ranges) + _sums(ranges, int(exponent)) + (opn,)


def turns_list(history, gate, exponent=3):
    """a scalar walk of the state machine over a Python list, independent of the vectorised one ->
    (reversals, ranges, range_sum, range_max, damage, open)"""
    x = [f32(v) for v in history]
    h = f32(gate)
    state, hi, lo, cand, last = 0, x[0], x[0], None, None
    reversals, ranges = 0, []
    for v in x[1:]:
        if state == 0:
            if f32(v - lo) > h:
                last, cand, state, reversals = lo, v, +1, reversals + 1
            elif f32(hi - v) > h:
                last, cand, state, reversals = hi, v, -1, reversals + 1
            else:
                hi, lo = (v if v > hi else hi), (v if v < lo else lo)
        elif state > 0:
            if v > cand:
                cand = v
            elif f32(cand - v) > h:
                ranges.append(f32(cand - last))
                last, cand, state, reversals = cand, v, -1, reversals + 1
        else:
            if v < cand:
                cand = v
            elif f32(v - cand) > h:
                ranges.append(f32(last - cand))
                last, cand, state, reversals = cand, v, +1, reversals + 1
    opn = f32(hi - lo) if state == 0 else f32(cand - last) if state > 0 else f32(last - cand)
    return (reversals, ranges) + _sums(ranges, int(exponent)) + (opn,)


def rates_list(history):
    """(rise, fall, rise_when, fall_when, path) of one history by a scalar walk"""
    x = [f32(v) for v in history]
    if len(x) < 2:
        return f32(0), f32(0), -1, -1, f32(0)
    r = [f32(q - p) for p, q in zip(x, x[1:])]
    path = f32(0)
    for v in r:
        path = f32(path + abs(v))
    return max(r), min(r), 1 + r.index(max(r)), 1 + r.index(min(r)), path


def ratios(out, F, gate, exponent=3):
    """The worst err / bound of path, range_sum and damage in `out` (emulate's or the kernel's dict; a group may be missing) against
    the float64 sums at the decisions the emulation makes on F -> dict name -> float (0 where both are 0, inf if a bound of 0 is
    missed)"""
    T = np.shape(F)[-2]
    m = int(exponent)
    ref = emulate(F, gate, m, sums64=True)
    K = ref["K"].astype(np.float64)

    def worst(got, want, factor):
        err, bnd = np.abs(np.asarray(got, np.float64) - want), factor * U * np.abs(want)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(bnd > 0, err / bnd, np.where(err > 0, np.inf, 0.0))
        return float(ratio.max()) if ratio.size else 0.0

    res = {}
    if "rates" in out and out["rates"] is not None:
        res["path"] = worst(np.asarray(out["rates"])[..., 2, :], ref["path64"], T + 1)
    if "ranges" in out and out["ranges"] is not None:
        res["range_sum"] = worst(np.asarray(out["ranges"])[..., 0, :], ref["range64"], K + 1)
        res["damage"] = worst(np.asarray(out["ranges"])[..., 2, :], ref["damage64"], 2 * m + K)
    return res


def kernel_gates(F):
    """The four gates of the kernel tests from a stored field F [B, T, C], fp32 [4, C], each >= 0: 0 (every strict extremum turns); a
    quarter of the node's peak-to-peak over (sample, time) (many reversals left, many filtered); fl(|F[0, 1] - F[0, 0]|), the strict
    tie at the first step of sample 0 (0 at T = 1); twice the peak-to-peak (nothing turns, open = fl(max - min))."""
    F = np.asarray(F, f32)
    flat = F.reshape(-1, F.shape[-1])
    p2p = (flat.max(axis=0) - flat.min(axis=0)).astype(f32)
    first = np.abs((F[0, 1] - F[0, 0]).astype(f32)) if F.shape[1] > 1 else np.zeros_like(p2p)
    return np.stack([np.zeros_like(p2p), p2p * f32(0.25), first, p2p * f32(2)]).astype(f32)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.int32), b.view(np.int32))
