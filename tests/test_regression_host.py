"""Host side of the surrogate response surfaces (no GPU): predict.regression_covariates / regression_weights, RegressionResult, the
declaration / binding of the new entry points, the numpy float32 emulation of the kernel's arithmetic (tests/regression_reference.py)
-- split invariance, its moments against the ensemble emulation, exact zeros, the two-pass co-moment -- the emulation against the
same recurrence in float64 within the a-priori bound derived in tests/regression_reference.py (no constant fitted), and an analytic
case x = a + sum b_i y_i whose coefficients, intercept and R^2 come back within that bound propagated through the inverse Gram
matrix.

Worst err / bound of the emulation against float64 over all cases below (numpy IEEE arithmetic, the same on any machine): 0.28,
at n = 2."""
import os
import re
import sys

import numpy as np
import pytest

import simulgen_vae_amd  # noqa: F401
from simulgen_vae_amd import engine as E
from simulgen_vae_amd.predict import RegressionResult, Surrogate, regression_covariates, regression_weights

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ensemble_reference as ER  # noqa: E402
import regression_reference as RR  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["sgv_regress", "sgv_test_recon_regress"]
T, N = 3, 40


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


# ---- regression_covariates ----
def test_good_covariates_come_back_as_float64():
    a = regression_covariates([[1, 2], [3, 4], [5, 6]], 3)
    assert a.dtype == np.float64 and a.shape == (3, 2)
    assert regression_covariates(np.zeros((4, 32), np.float32), 4).shape == (4, 32)
    assert regression_covariates(np.zeros((0, 1)), 0).shape == (0, 1)


@pytest.mark.parametrize("cov,P,msg", [
    ([1.0, 2.0], 2, r"covariates: a \[P, K\] array is required, got shape \(2,\)"),
    (np.zeros((2, 2, 2)), 2, r"a \[P, K\] array is required"),
    (np.zeros((3, 2)), 4, r"covariates: 3 rows, expected P = 4"),
    (np.zeros((3, 0)), 3, r"covariates: K = 0 columns, between 1 and 32 are required"),
    (np.zeros((3, 33)), 3, r"covariates: K = 33 columns, between 1 and 32"),
    ([[0.0, 1.0], [np.nan, np.inf]], 2, r"covariates\[1, 0\] = nan is not finite"),
    ([[0.0, -np.inf], [0.0, 1.0]], 2, r"covariates\[0, 1\] = -inf is not finite")])
def test_bad_covariates_are_named(cov, P, msg):
    with pytest.raises(ValueError, match=msg):
        regression_covariates(cov, P)


# ---- regression_weights ----
def test_weights_do_not_depend_on_the_cut_and_the_first_is_zero():
    rng = np.random.default_rng(0)
    Y = rng.standard_normal((37, 4)) * [1.0, 1000.0, 1e-3, 5.0] + [0.0, 3e4, 0.0, -7.0]
    w, mean, gram = regression_weights(Y)
    assert w.dtype == np.float32 and w.shape == (37, 4) and mean.dtype == gram.dtype == np.float64 and gram.shape == (4, 4)
    assert not w[0].any() and not np.signbit(w[0]).any()          # y_0 - y_0: exactly +0
    for cut in (1, 5, 36):
        w1, m1, g1 = regression_weights(Y[:cut])
        w2, m2, g2 = regression_weights(Y[cut:], m1, g1, cut)
        assert np.array_equal(bits(np.concatenate([w1, w2])), bits(w))
        assert np.array_equal(m2.view(np.int64), mean.view(np.int64)) and np.array_equal(g2.view(np.int64), gram.view(np.int64))
    assert m1 is not mean and np.array_equal(regression_weights(Y[:36])[1], m1)          # the arguments are left alone
    # the Gram matrix is the centred one, the mean the mean
    Yc = Y - Y.mean(0)
    assert np.allclose(gram, Yc.T @ Yc, rtol=1e-12, atol=0) and np.allclose(mean, Y.mean(0), rtol=1e-14, atol=0)
    # w[m] is y_m minus the mean of members 0 .. m
    run = np.cumsum(Y, 0) / np.arange(1, 38)[:, None]
    assert np.allclose(w, (Y - run).astype(np.float32), rtol=1e-6, atol=1e-30)
    e = regression_weights(np.zeros((0, 4)))
    assert e[0].shape == (0, 4) and not e[1].any() and not e[2].any()
    with pytest.raises(ValueError, match="must be"):
        regression_weights(np.zeros(4))
    with pytest.raises(ValueError, match="do not fit"):
        regression_weights(Y, np.zeros(3), None, 0)


# ---- the emulation ----
def _field(n, rng, offset=0.0):
    return (offset + rng.standard_normal((n, T, N)) * (1.0 + rng.random((1, T, N)))).astype(np.float32)


def _weights(n, K, rng, big=None):
    Y = rng.standard_normal((n, K))
    if big is not None:
        Y[:, big] *= 1000.0
    return regression_weights(Y)[0], Y


def test_any_split_of_the_members_gives_the_bits_of_one_call():
    rng = np.random.default_rng(1)
    F, (W, _) = _field(19, rng, 3.0), _weights(19, 3, rng)
    whole = RR.update(F, W)
    for parts in ((1, 18), (7, 12), (18, 1), (5, 5, 9)):
        st, lo = None, 0
        for n in parts:
            st = RR.update(F[lo:lo + n], W[lo:lo + n], st, lo)
            lo += n
        assert all(np.array_equal(bits(st[k]), bits(whole[k])) for k in RR.STATE), parts
    assert RR.update(F[:0], W[:0])["comoment"].shape == (3, T, N)


def test_the_moments_are_the_ensemble_emulations():
    rng = np.random.default_rng(2)
    F, (W, _) = _field(23, rng, -10.0), _weights(23, 2, rng)
    got, want = RR.update(F, W), ER.update(F)
    assert np.array_equal(bits(got["mean"]), bits(want["mean"])) and np.array_equal(bits(got["m2"]), bits(want["m2"]))
    # and in a continuation
    got = RR.update(F[9:], W[9:], RR.update(F[:9], W[:9]), 9)
    assert np.array_equal(bits(got["mean"]), bits(want["mean"])) and np.array_equal(bits(got["m2"]), bits(want["m2"]))


def test_a_covariate_with_zero_weights_leaves_plus_zero():
    rng = np.random.default_rng(3)
    F, (W, _) = _field(12, rng), _weights(12, 3, rng)
    W[:, 1] = 0.0
    co = RR.update(F, W)["comoment"]
    assert not co[1].any() and not np.signbit(co[1]).any() and co[0].any() and co[2].any()


def test_the_comoment_is_the_two_pass_sum():
    rng = np.random.default_rng(4)
    for n, K, off in ((2, 1, 0.0), (40, 3, 5.0), (300, 2, -20.0)):
        F = _field(n, rng, off)
        W, Y = _weights(n, K, rng)
        co = RR.update(F, W)["comoment"].astype(np.float64)
        F64 = F.astype(np.float64)
        two = np.einsum("mtn,mk->ktn", F64 - F64.mean(0), Y - Y.mean(0))
        scale = np.einsum("mtn,mk->ktn", np.abs(F64 - F64.mean(0)) + np.abs(off) * 1e-3, np.abs(Y - Y.mean(0)))
        assert np.abs(co - two).max() <= 1e-4 * scale.max(), (n, K)          # the identity, not the rounding: that is the next test


CASES = [(n, K, off) for n in (1, 2, 3, 16, 64, 500, 4000) for K, off in ((1, 0.0), (3, 10.0), (6, 100.0))]


@pytest.mark.parametrize("n,K,off", CASES)
def test_the_emulation_is_within_the_a_priori_bound_of_float64(n, K, off):
    rng = np.random.default_rng(100 * n + K)
    F = _field(n, rng, off)
    W, _ = _weights(n, K, rng, big=K - 1 if K > 1 else None)          # one covariate scaled by 1000
    got = RR.update(F, W)["comoment"].astype(np.float64)
    want = RR.update64(F, W)[0]["comoment"]
    bound = RR.comoment_bound(F, W)
    err = np.abs(got - want)
    ratio = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), 0.0)))
    print(f"n = {n}, K = {K}, offset = {off}: worst err / bound = {ratio:.3f}")
    assert (err <= bound).all()
    if n == 1:
        assert not got.any()          # the first member's weights are zero and so is its deviation from the empty mean's successor
    else:
        assert (bound > 0).all()


# ---- the analytic case ----
def _analytic():
    rng = np.random.default_rng(5)
    n, K = 24, 3
    Y = rng.integers(0, 16, (n, K)) / 8.0                                       # a grid of eighths
    a = rng.integers(-8, 9, (2, 5)) / 4.0
    b = rng.integers(-8, 9, (K, 2, 5)) / 4.0
    b[1, 0, 0] = 0.0                                                            # a covariate without influence somewhere
    x = a + np.einsum("mk,ktn->mtn", Y, b)
    F = x.astype(np.float32)
    assert np.array_equal(F.astype(np.float64), x)                              # exactly representable
    return Y, a, b, F


def test_an_exactly_linear_response_is_recovered():
    import torch
    Y, a, b, F = _analytic()
    n, K = Y.shape
    w, ybar, gram = regression_weights(Y)
    st = RR.update(F, w)
    r = RegressionResult(count=n, mean=torch.from_numpy(st["mean"]), m2=torch.from_numpy(st["m2"]), comoment=torch.from_numpy(st["comoment"]),
                         cov_mean=ybar, cov_gram=gram)
    ginv = r.gram_inverse()
    assert np.allclose(ginv @ gram, np.eye(K), atol=1e-12)
    ref, _, _ = RR.update64(F, w)
    cb = RR.comoment_bound(F, w, rounded_weights=True)
    X = np.abs(F).max(0).astype(np.float64)
    m2b = ER.welford_bound(n, ref["mean"], ref["m2"])
    dbeta, dicpt, dr2 = RR.derived_bounds(ginv, ref["comoment"], cb, ybar, ref["mean"], ref["m2"], m2b, n, X)
    beta, icpt, r2 = r.coefficients(), r.intercept(), r.r2()
    assert beta.shape == (K, 2, 5) and beta.dtype == torch.float32 and icpt.shape == r2.shape == (2, 5)
    eb, ei, er = np.abs(beta.numpy() - b), np.abs(icpt.numpy() - a), np.abs(r2.numpy() - 1.0)
    print("worst err / bound: coefficients", (eb / dbeta).max(), "intercept", (ei / dicpt).max(), "r2", (er / dr2).max())
    assert (eb <= dbeta).all() and (ei <= dicpt).all() and (er <= dr2).all()
    assert dbeta.max() < 1e-4 and dicpt.max() < 1e-3 and dr2.max() < 1e-4          # and the bound means something
    # covariance and correlation
    assert torch.equal(r.covariance(), r.comoment / float(n)) and torch.equal(r.covariance(ddof=1), r.comoment / float(n - 1))
    cor = r.correlation().numpy()
    assert cor.shape == (K, 2, 5) and np.abs(cor).max() <= 1.0 + 1e-5 and cor[1, 0, 0] != 0.0          # correlated through the other inputs or not: finite
    want = np.einsum("mtn,mk->ktn", F - F.mean(0), Y - Y.mean(0)) / np.sqrt(ref["m2"][None] * np.diag(gram)[:, None, None])
    assert np.allclose(cor, want, atol=1e-5)


# ---- RegressionResult ----
def _result(n=6, K=2, seed=7):
    import torch
    rng = np.random.default_rng(seed)
    F, (W, Y) = _field(n, rng), _weights(n, K, rng)
    _, ybar, gram = regression_weights(Y)
    st = RR.update(F, W)
    return RegressionResult(count=n, mean=torch.from_numpy(st["mean"]), m2=torch.from_numpy(st["m2"]), comoment=torch.from_numpy(st["comoment"]),
                            cov_mean=ybar, cov_gram=gram)


def test_regression_result_fields_and_guards():
    import torch
    assert RegressionResult.FIELDS == ("count", "mean", "m2", "comoment", "cov_mean", "cov_gram")
    assert RegressionResult.STATE == E.REGRESS_FIELDS == ("mean", "m2", "comoment") and E.REGRESS_MAX_COVARIATES == 32
    with pytest.raises(KeyError):
        RegressionResult(count=0)
    r = _result()
    assert sorted(r.state()) == ["comoment", "m2", "mean"] and r.state()["comoment"] is r.comoment and r.n_cov == 2
    assert torch.equal(r.var(), r.m2 / 6.0) and torch.equal(r.std(ddof=1), (r.m2 / 5.0).sqrt())
    for f in (r.var, r.std, r.covariance):
        with pytest.raises(ValueError, match="count - ddof = 6 - 6 is not positive"):
            f(ddof=6)
    assert r.coefficients().shape == (2, T, N) and r.r2().shape == (T, N) and r.intercept().shape == (T, N)
    assert bool((r.r2() >= 0).all()) and bool((r.r2() <= 1.0 + 1e-5).all())
    with pytest.raises(ValueError, match="into must be a RegressionResult, not dict"):
        RegressionResult.require({})
    RegressionResult.require(r)
    with pytest.raises(ValueError, match=r"into.comoment must be a contiguous"):
        r.continued({"comoment": ((2, T, N), torch.float32)})          # not on the device
    assert callable(Surrogate.regress) and callable(E.Engine.regress)
    assert "coefficients()" in Surrogate.regress.__doc__ and "r2()" in Surrogate.regress.__doc__


def test_singular_designs_are_refused():
    r = _result(n=6, K=2)
    r.count = 2
    with pytest.raises(ValueError, match="count = 2 members do not determine 2 coefficients"):
        r.coefficients()
    r = _result(n=6, K=3)
    r.cov_gram = np.array(r.cov_gram)
    r.cov_gram[1, :] = 0.0
    r.cov_gram[:, 1] = 0.0
    for f in (r.coefficients, r.intercept, r.r2):
        with pytest.raises(ValueError, match=r"covariate 1 does not vary \(gram\[1, 1\] = 0.0\)"):
            f()
    # two covariates that are multiples of each other
    Y = np.random.default_rng(8).standard_normal((10, 3))
    Y[:, 2] = -3.0 * Y[:, 0]
    r = _result(n=10, K=3)
    r.cov_mean, r.cov_gram = regression_weights(Y)[1:]
    with pytest.raises(ValueError, match=r"linearly dependent \(rank 2 of 3\)"):
        r.coefficients()
    # correlation and covariance need no inverse
    assert r.correlation().shape == (3, T, N) and r.covariance().shape == (3, T, N)


# ---- ABI ----
def test_new_entry_points_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "sgvae.h")).read()
    for s in NEW_SYMBOLS:
        assert re.search(rf"\bint {s}\s*\(", hdr), s
        assert s in E.ABI_SYMBOLS
    assert re.search(r"\}\s*sgv_regress_state;", hdr)
    assert [f for f, _ in E.RegressState._fields_] == ["mean", "m2", "comoment"]
    lib = E.load_library()
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s), s
    assert len(lib.sgv_regress.argtypes) == 11 and len(lib.sgv_test_recon_regress.argtypes) == 16
    # without an engine the call is an argument error that says who complains
    assert lib.sgv_regress(None, None, None, 1, 1, None, None, 1, None, 0, None) == -1 and "sgv_regress" in lib.sgv_last_error().decode()
    assert lib.sgv_test_recon_regress(0, None, 8, None, None, None, None, None, 1, None, 0, None, 1, 1, 8, None) == -1
    assert "sgv_test_recon_regress: null argument" in lib.sgv_last_error().decode()
