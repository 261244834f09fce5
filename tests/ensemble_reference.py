"""numpy float32 emulation of the ensemble pass (csrc/recon_out.hip: recon_ensemble_kernel): the contract of its
arithmetic, one np.float32 operation -- one rounding -- per operation of the kernel, members one after the other.

For member b of a call, index m = count_before + b, value x (an fp32 array [T, N]):
    moments   k = m + 1, r = 1.0f / (float)k;  d = x - mean;  mean = mean + d * r;  m2 = m2 + d * (x - mean)
    extrema   if x > max: max = x, arg_max = m;  if x < min: min = x, arg_min = m          (strict: the earliest member keeps a tie)
    exceed    exceed += x > limit[n]                                                      (strict)
An empty state (count_before == 0) is mean = m2 = 0, max = -inf, min = +inf, indices and counts 0.  numpy only."""
import numpy as np

STATE = ("mean", "m2", "max", "min", "arg_max", "arg_min", "exceed")


def empty_state(T, N):
    f = lambda v: np.full((T, N), v, np.float32)
    i = lambda: np.zeros((T, N), np.int32)
    return dict(mean=f(0), m2=f(0), max=f(-np.inf), min=f(np.inf), arg_max=i(), arg_min=i(), exceed=i())


def update(F, state=None, count_before=0, limit=None):
    """Merges the members F [B, T, N] (float32) into `state` (a dict as empty_state's; None: empty, count_before must be 0) and
    returns the new state; the argument is left alone.  limit: [N] float32 or None (exceed then stays as it is)."""
    F = np.asarray(F)
    assert F.dtype == np.float32 and F.ndim == 3
    B, T, N = F.shape
    if state is None:
        assert count_before == 0
        state = empty_state(T, N)
    s = {k: np.array(v, copy=True) for k, v in state.items()}
    if limit is not None:
        limit = np.asarray(limit, np.float32).reshape(1, N)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        for b in range(B):
            m = count_before + b
            x = F[b]
            r = np.float32(1.0) / np.float32(m + 1)
            d = x - s["mean"]
            s["mean"] = s["mean"] + d * r
            s["m2"] = s["m2"] + d * (x - s["mean"])
            up, dn = x > s["max"], x < s["min"]
            s["max"] = np.where(up, x, s["max"]); s["arg_max"] = np.where(up, np.int32(m), s["arg_max"]).astype(np.int32)
            s["min"] = np.where(dn, x, s["min"]); s["arg_min"] = np.where(dn, np.int32(m), s["arg_min"]).astype(np.int32)
            if limit is not None:
                s["exceed"] = (s["exceed"] + (x > limit)).astype(np.int32)
    for k in ("mean", "m2", "max", "min"):
        assert s[k].dtype == np.float32
    return s


def welford_bound(k, mean, M2):
    """A-priori bound of the relative error of M2 after k Welford updates in precision u = 2^-24 (Chan, Golub and LeVeque 1983,
    "Algorithms for computing the sample variance", section on updating algorithms: relative error of order k u kappa),
    kappa = sqrt(1 + k mean^2 / M2) the condition number of the data; returned as an absolute bound on M2: k u kappa M2."""
    u = 2.0 ** -24
    kappa = np.sqrt(1.0 + k * np.square(mean) / M2)
    return k * u * kappa * M2
