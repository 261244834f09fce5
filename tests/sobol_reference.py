"""numpy float32 emulation of the Sobol pass (csrc/recon_out.hip: recon_sobol_kernel): the contract of its
arithmetic, one np.float32 operation -- one rounding -- per operation of the kernel.

A call holds nb whole blocks of d + 2 members, F [nb (d + 2), T, N]: block j is A_j, B_j, AB_1_j .. AB_d_j.  Base sample
j (counted from blocks_before) updates, per (t, n):
    moments     Welford with xA (k = 2 j + 1) and then xB (k = 2 j + 2):  r = 1.0f / (float)k;  dl = x - mean;
                mean = mean + dl * r;  m2 = m2 + dl * (x - mean)                       (tests/ensemble_reference.py, the same lines)
    first_sq[i] e = xB - xAB_i;  first_sq[i] = first_sq[i] + e * e                      (Jansen's first-order form)
    total_sq[i] e = xA - xAB_i;  total_sq[i] = total_sq[i] + e * e                      (Jansen's total form)
An empty state (blocks_before == 0) is all zeros.  numpy only."""
import numpy as np

from ensemble_reference import welford_bound  # noqa: F401  (the bound of m2: 2 n Welford updates)

STATE = ("mean", "m2", "first_sq", "total_sq")


def empty_state(d, T, N):
    z = lambda *s: np.zeros(s, np.float32)
    return dict(mean=z(T, N), m2=z(T, N), first_sq=z(d, T, N), total_sq=z(d, T, N))


def update(F, d, state=None, blocks_before=0):
    """Merges the blocks F [nb (d + 2), T, N] (float32) into `state` (a dict as empty_state's; None: empty, blocks_before must be 0)
    and returns the new state; the argument is left alone."""
    F = np.asarray(F)
    assert F.dtype == np.float32 and F.ndim == 3 and d >= 1 and F.shape[0] % (d + 2) == 0
    T, N = F.shape[1:]
    nb = F.shape[0] // (d + 2)
    if state is None:
        assert blocks_before == 0
        state = empty_state(d, T, N)
    s = {k: np.array(v, copy=True) for k, v in state.items()}
    F = F.reshape(nb, d + 2, T, N)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        for j in range(nb):
            xa, xb = F[j, 0], F[j, 1]
            for x, k in ((xa, 2 * (blocks_before + j) + 1), (xb, 2 * (blocks_before + j) + 2)):
                r = np.float32(1.0) / np.float32(k)
                dl = x - s["mean"]
                s["mean"] = s["mean"] + dl * r
                s["m2"] = s["m2"] + dl * (x - s["mean"])
            for i in range(d):
                e = xb - F[j, 2 + i]
                s["first_sq"][i] = s["first_sq"][i] + e * e
                e = xa - F[j, 2 + i]
                s["total_sq"][i] = s["total_sq"][i] + e * e
    for k in STATE:
        assert s[k].dtype == np.float32
    return s


def exact(F, d):
    """the same sums in float64 on the same fp32 values: two-pass mean and M2 over the 2 nb values of A and B, and the plain sums of
    squared differences"""
    F = np.asarray(F, np.float64)
    nb = F.shape[0] // (d + 2)
    F = F.reshape(nb, d + 2, *F.shape[1:])
    ab = F[:, :2].reshape(2 * nb, *F.shape[2:])
    mean = ab.mean(axis=0)
    return dict(mean=mean, m2=np.square(ab - mean).sum(axis=0),
                first_sq=np.square(F[:, 1:2] - F[:, 2:]).sum(axis=0), total_sq=np.square(F[:, 0:1] - F[:, 2:]).sum(axis=0))


def sumsq_bound(n, S):
    """A-priori bound of |s_n - S| for the fp32 running sum s_n of n squared fp32 differences, S = sum_j (a_j - b_j)^2 exactly:
    gamma S with gamma = (n + 2) u / (1 - (n + 2) u), u = 2^-24.

    Derivation (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., lemma 3.1 and section 4.2; fl(x op y) =
    (x op y)(1 + delta), |delta| <= u, no underflow).  One term takes three rounding factors: e = fl(a - b) = (a - b)(1 + d1), and
    q = fl(e e) = e^2 (1 + d2) = (a - b)^2 (1 + d1)^2 (1 + d2).  The sum starts from 0, so s_1 = q_1 exactly, and term j then goes
    through the n - j additions that follow it; the first term and the second take the most, n - 1.  Every term therefore carries
    at most 3 + (n - 1) = n + 2 factors (1 + delta_i)^(+-1), whose product is 1 + theta with |theta| <= gamma_(n+2) (lemma 3.1).
    All terms are non-negative, so nothing cancels: |s_n - S| <= gamma_(n+2) sum_j (a_j - b_j)^2 = gamma_(n+2) S.  Cutting the sum
    into launches changes nothing: the state is stored in fp32 as it is held, and the operations are the same ones in the same order."""
    u = 2.0 ** -24
    k = (n + 2) * u
    return k / (1.0 - k) * S
