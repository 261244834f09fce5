"""numpy float32 emulation of the regression pass (csrc/recon_out.hip: recon_regress_kernel): the contract of its
arithmetic, one np.float32 operation -- one rounding -- per operation of the kernel, members one after the other.

For member b of a call, index m = count_before + b, k = m + 1, value x (an fp32 array [T, N]) and weights W[b] (fp32 [K], the centred
covariates predict.regression_weights forms on the host):
    r = 1.0f / (float)k;  d = x - mean;  mean = mean + d * r;  m2 = m2 + d * (x - mean)      (ensemble_reference's moments)
    co[i] = co[i] + d * W[b, i]      for i = 0 .. K - 1
An empty state (count_before == 0) is zeros.

The bound of the co-moment, comoment_bound().  The reference is the same recurrence in float64 on the same fp32 field and the same
fp32 weights: c = sum_j d_j w_j, d_j = x_j - mean_(j-1).  u = 2^-24; X_j = the largest |x| over members 1 .. j.
  * The running mean.  mean_j = mean_(j-1) + d_j r_j: the error of mean_(j-1) comes back multiplied by (1 - 1/j) <= 1; the subtraction
    that forms d_j, the rounding of r_j = 1/j and the product add at most 3 u |d_j| / j <= 6 u X_j / j (|d_j| <= 2 X_j), and the sum
    adds u |mean_j| <= u X_j.  Summed over j members, with H_j <= 1 + ln j:   e_j <= (j + 6 (1 + ln j)) u X_j.   mean_0 = 0 is exact.
  * The deviation the kernel holds, fl(x_j - mean^_(j-1)), differs from d_j by the error of the mean, e_(j-1), and its own rounding,
    u |d_j|.
  * n products and n sums follow: a relative gamma_(n+1) = (n + 1) u / (1 - (n + 1) u) of sum_j |d_j w_j|.
        |c^ - c| <= sum_j |w_j| (e_(j-1) + u |d_j|) + gamma_(n+1) sum_j |d_j w_j|
Every quantity on the right is formed in float64 from the data; no constant is fitted.  With rounded_weights=True the reference may
also hold the covariates unrounded (a float64 least-squares fit): the weights the kernel sees are float32(y - ybar), a relative u each,
which adds u sum_j |d_j w_j|.  Worst err / bound seen: DESIGN.md section 22.  numpy only."""
import numpy as np

STATE = ("mean", "m2", "comoment")
U = 2.0 ** -24


def empty_state(K, T, N):
    return dict(mean=np.zeros((T, N), np.float32), m2=np.zeros((T, N), np.float32), comoment=np.zeros((K, T, N), np.float32))


def update(F, W, state=None, count_before=0):
    """Merges the members F [B, T, N] (float32) with weights W [B, K] (float32) into `state` (a dict as empty_state's; None: empty,
    count_before must be 0) and returns the new state; the arguments are left alone."""
    F, W = np.asarray(F), np.asarray(W)
    assert F.dtype == np.float32 and F.ndim == 3 and W.dtype == np.float32 and W.ndim == 2 and W.shape[0] == F.shape[0]
    B, T, N = F.shape
    K = W.shape[1]
    if state is None:
        assert count_before == 0
        state = empty_state(K, T, N)
    s = {k: np.array(v, copy=True) for k, v in state.items()}
    assert s["comoment"].shape == (K, T, N)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        for b in range(B):
            x = F[b]
            r = np.float32(1.0) / np.float32(count_before + b + 1)
            d = x - s["mean"]
            s["mean"] = s["mean"] + d * r
            s["m2"] = s["m2"] + d * (x - s["mean"])
            for i in range(K):
                s["comoment"][i] = s["comoment"][i] + d * W[b, i]
    for k in STATE:
        assert s[k].dtype == np.float32
    return s


def update64(F, W):
    """the same recurrence from empty in float64 on the same values -> (state, sum_j |d_j w_j| [K, T, N], the bound's first sum)"""
    F, W = np.asarray(F, np.float64), np.asarray(W, np.float64)
    B, T, N = F.shape
    K = W.shape[1]
    mean, m2, co = np.zeros((T, N)), np.zeros((T, N)), np.zeros((K, T, N))
    absdw, first = np.zeros((K, T, N)), np.zeros((K, T, N))
    X = np.zeros((T, N))
    e_prev = np.zeros((T, N))                  # e_0: the empty mean is exact
    for b in range(B):
        j = b + 1
        x = F[b]
        d = x - mean
        mean = mean + d / j
        m2 = m2 + d * (x - mean)
        aw = np.abs(W[b])[:, None, None]
        co = co + d * W[b][:, None, None]
        absdw += np.abs(d) * aw
        first += aw * (e_prev + U * np.abs(d))
        X = np.maximum(X, np.abs(x))
        e_prev = (j + 6.0 * (1.0 + np.log(j))) * U * X
    return dict(mean=mean, m2=m2, comoment=co), absdw, first


def comoment_bound(F, W, rounded_weights=False):
    """the a-priori bound [K, T, N] (float64) of |comoment of update(F, W) - comoment of update64(F, W)| derived above"""
    n = np.asarray(F).shape[0]
    _, absdw, first = update64(F, W)
    g = (n + 1) * U / (1.0 - (n + 1) * U)
    return first + (g + (U if rounded_weights else 0.0)) * absdw


def gamma(k):
    return k * U / (1.0 - k * U)


def mean_bound(n, X):
    """e_n above: the error of the running mean after n members of magnitude at most X"""
    return (n + 6.0 * (1.0 + np.log(max(n, 1)))) * U * X


def derived_bounds(ginv, co, co_bound, cov_mean, mean, m2, m2_bound, n, X):
    """The co-moment bound propagated to what RegressionResult derives, all float64; ginv [K, K] the inverse Gram matrix, co the
    co-moments [K, T, N], co_bound their bound, m2_bound the bound of m2 (ensemble_reference.welford_bound), X the largest |x|.
      coefficients  beta_i = sum_j ginv_ij co_j, ginv rounded to fp32 once and a K-term fp32 product:
                        |d beta_i| <= sum_j |ginv_ij| co_bound_j + gamma_(K+1) sum_j |ginv_ij| |co_j|
      intercept     mean - sum_i beta_i ybar_i, ybar rounded to fp32 once, a K-term product and one subtraction:
                        <= e_n + sum_i |d beta_i| |ybar_i| + gamma_(K+1) sum_i (|beta_i| + |d beta_i|) |ybar_i| + u |intercept|
      r2            S / m2, S = sum_i beta_i co_i (K products, K - 1 sums), one division:
                        dS <= sum_i (|d beta_i| (|co_i| + co_bound_i) + |beta_i| co_bound_i) + gamma_K sum_i |beta_i co_i|
                        <= dS / m2 + (|S| + dS) / m2 * rel / (1 - rel) + u |r2|,   rel = m2_bound / m2
    -> (d beta [K, T, N], d intercept [T, N], d r2 [T, N])"""
    K = co.shape[0]
    aginv, aco = np.abs(ginv), np.abs(co)
    beta = np.einsum("ij,jtn->itn", ginv, co)
    dbeta = np.einsum("ij,jtn->itn", aginv, co_bound) + gamma(K + 1) * np.einsum("ij,jtn->itn", aginv, aco)
    ay = np.abs(np.asarray(cov_mean, np.float64))[:, None, None]
    icpt = mean - (beta * np.asarray(cov_mean, np.float64)[:, None, None]).sum(0)
    dicpt = mean_bound(n, X) + (dbeta * ay).sum(0) + gamma(K + 1) * ((np.abs(beta) + dbeta) * ay).sum(0) + U * np.abs(icpt)
    S = (beta * co).sum(0)
    dS = (dbeta * (aco + co_bound) + np.abs(beta) * co_bound).sum(0) + gamma(K) * np.abs(beta * co).sum(0)
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = m2_bound / m2
        dr2 = dS / m2 + (np.abs(S) + dS) / m2 * rel / (1.0 - rel) + U * np.abs(S / m2)
    return dbeta, dicpt, dr2
