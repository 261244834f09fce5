"""Host side of the Sobol sensitivity indices (no GPU): predict.sobol_groups / sobol_design / sobol_members, SobolResult, the
declaration / binding of the new entry points, the numpy float32 emulation of the kernel's arithmetic (tests/sobol_reference.py)
against float64, and Jansen's estimators against an analytic case.

The emulation against float64, on the same fp32 values, u = 2^-24, no constant added anywhere:
  * first_sq, total_sq: |s - S| <= gamma_(n+2) S (sobol_reference.sumsq_bound, derived in its docstring);
  * m2: the a-priori bound of Welford's updating formula over the k = 2 n values of A and B (ensemble_reference.welford_bound).
Worst err / bound over all cases (numpy IEEE arithmetic, the same on any machine): sums of squares 0.84 (n = 1, where the bound is
3 u), m2 0.79 (n = 1, where the bound is only 2 u kappa); 0.035 and 0.22 at n = 4000."""
import os
import re
import sys

import numpy as np
import pytest

import simulgen_vae_amd  # noqa: F401
from simulgen_vae_amd import engine as E
from simulgen_vae_amd.predict import SobolResult, Surrogate, sobol_design, sobol_groups, sobol_members

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sobol_reference as SR  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["sgv_sobol", "sgv_test_recon_sobol"]


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


# ---- sobol_groups / sobol_design / sobol_members ----
def test_default_groups_are_the_columns():
    g = sobol_groups(None, 4)
    assert len(g) == 4 and all(a.dtype == np.int64 and a.tolist() == [i] for i, a in enumerate(g))


def test_good_groups_are_kept_in_order_and_may_overlap():
    g = sobol_groups([[2, 0], (1,), np.array([0, 1, 2]), [0]], 3)
    assert [a.tolist() for a in g] == [[2, 0], [1], [0, 1, 2], [0]]
    assert len(sobol_groups([[0]] * 30, 1)) == 30


@pytest.mark.parametrize("groups,msg", [
    ([], "at least one group"), ([[0]] * 31, "31 groups, at most 30"), (5, "a sequence of index lists"),
    ([[0], []], r"groups\[1\]: a non-empty 1-D list"), ([[0], [[1]]], r"groups\[1\]: a non-empty 1-D list"),
    ([[0], [0.5]], r"groups\[1\]: an integer dtype"), ([[0, 1], [1, 3, 4]], r"groups\[1\]\[1\] = 3 is outside \[0, 3\)"),
    ([[-1]], r"groups\[0\]\[0\] = -1 is outside")])
def test_bad_groups_are_named(groups, msg):
    with pytest.raises(ValueError, match=msg):
        sobol_groups(groups, 3)
    with pytest.raises(ValueError, match="31 groups"):
        sobol_groups(None, 31)


def test_design_is_uniform_in_its_bounds_and_reproducible():
    lo, hi = [0.0, -2.0, 5.0], [1.0, 2.0, 5.0]
    A, B = sobol_design(lo, hi, 500, seed=3)
    assert A.shape == B.shape == (500, 3) and A.dtype == B.dtype == np.float32 and not np.array_equal(A, B)
    for M in (A, B):
        assert (M >= np.float32(lo)).all() and (M <= np.float32(hi)).all() and (M[:, 2] == 5.0).all()
        assert abs(M[:, 0].mean() - 0.5) < 0.06 and abs(M[:, 1].mean()) < 0.24          # 4.6 sigma of a uniform mean at n = 500
    A2, B2 = sobol_design(lo, hi, 500, seed=3)
    assert np.array_equal(A, A2) and np.array_equal(B, B2)
    assert not np.array_equal(A, sobol_design(lo, hi, 500, seed=4)[0])


@pytest.mark.parametrize("lo,hi,n,msg", [
    ([0, 0], [1], 4, "one length"), ([[0]], [[1]], 4, "1-D"), ([], [], 4, "one length"), ([0, np.nan], [1, 1], 4, r"lo\[1\] = nan is not finite"),
    ([0, 0], [1, np.inf], 4, r"hi\[1\] = inf is not finite"), ([0, 2], [1, 1], 4, r"hi\[1\] = 1.0 is below lo\[1\] = 2.0"),
    ([0], [1], 0, "at least one base sample"), ([0], [1], -3, "at least one base sample")])
def test_bad_design_is_named(lo, hi, n, msg):
    with pytest.raises(ValueError, match=msg):
        sobol_design(lo, hi, n)


def test_members_are_blocks_of_a_b_and_the_mixed_rows():
    A, B = sobol_design([0, 0, 0], [1, 1, 1], 4, seed=1)
    M = sobol_members(A, B, [[0], [1, 2]])
    assert M.shape == (16, 3) and M.dtype == np.float32
    M = M.reshape(4, 4, 3)
    assert np.array_equal(M[:, 0], A) and np.array_equal(M[:, 1], B)
    assert np.array_equal(M[:, 2, 0], B[:, 0]) and np.array_equal(M[:, 2, 1:], A[:, 1:])
    assert np.array_equal(M[:, 3, 0], A[:, 0]) and np.array_equal(M[:, 3, 1:], B[:, 1:])
    assert sobol_members(A, B, None).shape == (20, 3)
    with pytest.raises(ValueError, match="one shape"):
        sobol_members(A, B[:3], None)


# ---- SobolResult ----
def test_sobol_result_fields_and_methods_on_cpu_tensors():
    import torch
    assert SobolResult.FIELDS == ("count", "n_params", "mean", "m2", "first_sq", "total_sq")
    with pytest.raises(KeyError):
        SobolResult(count=0)
    m2 = torch.tensor([[8.0, 0.0, 0.0]])                                   # n = 2: var = m2 / 4 = (2, 0, 0)
    first = torch.tensor([[[2.0, 0.0, 1.0]], [[8.0, 0.0, 0.0]]])
    total = torch.tensor([[[6.0, 0.0, 3.0]], [[0.0, 0.0, 0.0]]])
    r = SobolResult(count=2, n_params=2, mean=torch.zeros(1, 3), m2=m2, first_sq=first, total_sq=total)
    assert r.want() == ("first", "total") and sorted(r.state()) == ["first_sq", "m2", "mean", "total_sq"]
    assert torch.equal(r.var(), torch.tensor([[2.0, 0.0, 0.0]])) and torch.equal(r.var(ddof=1), m2 / 3.0)
    S, ST = r.first_order(), r.total_order()
    assert S.shape == ST.shape == (2, 1, 3)
    assert S[0, 0, 0] == 0.75 and S[1, 0, 0] == 0.0 and ST[0, 0, 0] == 0.75 and ST[1, 0, 0] == 0.0
    # var == 0: what the division says
    assert torch.isnan(S[0, 0, 1]) and torch.isnan(ST[0, 0, 1])            # 0 / 0
    assert S[0, 0, 2] == float("-inf") and ST[0, 0, 2] == float("inf")     # 1 - 1 / 0, 3 / 0
    with pytest.raises(ValueError, match="2 count - ddof"):
        r.var(ddof=4)
    only = SobolResult(count=2, n_params=2, mean=torch.zeros(1, 3), m2=m2, first_sq=None, total_sq=total)
    assert only.want() == ("total",) and sorted(only.state()) == ["m2", "mean", "total_sq"]
    with pytest.raises(ValueError, match="'first' was not asked for"):
        only.first_order()
    empty = SobolResult(count=0, n_params=2, mean=torch.zeros(1, 3), m2=m2, first_sq=first, total_sq=None)
    for f in (empty.var, empty.first_order, empty.total_order):
        with pytest.raises(ValueError):
            f()


def test_surrogate_and_engine_have_sobol():
    assert callable(Surrogate.sobol) and callable(E.Engine.sobol)
    doc = Surrogate.sobol.__doc__
    assert "1e-10" in doc and "not bit-zero" in doc and "first_order" in doc and "total_order" in doc
    assert E.SOBOL_MAX_PARAMS == 30 and E.SOBOL_FIELDS == ("mean", "m2", "first_sq", "total_sq")


def test_new_entry_points_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "sgvae.h")).read()
    for s in NEW_SYMBOLS:
        assert re.search(rf"\bint {s}\s*\(", hdr), s
        assert s in E.ABI_SYMBOLS
    assert re.search(r"\}\s*sgv_sobol_state;", hdr)
    assert [f for f, _ in E.SobolState._fields_] == ["mean", "m2", "first_sq", "total_sq"]
    lib = E.load_library()
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s), s
    assert len(lib.sgv_sobol.argtypes) == 10 and len(lib.sgv_test_recon_sobol.argtypes) == 15
    # without an engine the call is an argument error that says who complains
    assert lib.sgv_sobol(None, None, None, 4, 1, None, None, 2, 0, None) == -1 and "sgv_sobol" in lib.sgv_last_error().decode()
    assert lib.sgv_test_recon_sobol(0, None, 8, None, None, None, None, None, 1, 0, None, 3, 1, 8, None) == -1
    assert "sgv_test_recon_sobol: null argument" in lib.sgv_last_error().decode()


# ---- the emulation ----
def _blocks(nb, d, T, N, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((nb * (d + 2), T, N)) * 3 + 1).astype(np.float32)


def test_emulation_split_at_any_block_boundary_gives_the_same_bits():
    nb, d = 6, 3
    F = _blocks(nb, d, 2, 5, 7)
    whole = SR.update(F, d)
    for cut in range(1, nb):
        part = SR.update(F[cut * (d + 2):], d, SR.update(F[:cut * (d + 2)], d), cut)
        assert all(np.array_equal(bits(whole[k]), bits(part[k])) for k in SR.STATE), cut
    thirds = SR.update(F[4 * 5:], d, SR.update(F[5:4 * 5], d, SR.update(F[:5], d), 1), 4)
    assert all(np.array_equal(bits(whole[k]), bits(thirds[k])) for k in SR.STATE)
    one = SR.update(F[:5], d)
    assert np.array_equal(one["first_sq"][1], np.square(F[1] - F[3])) and np.array_equal(one["total_sq"][2], np.square(F[0] - F[4]))


def test_emulation_identical_members_give_exact_zeros():
    nb, d = 5, 3
    F = _blocks(nb, d, 2, 5, 8).reshape(nb, d + 2, 2, 5)
    F[:, 2 + 0] = F[:, 0]          # AB_1 == A: parameter 1 does nothing
    F[:, 2 + 2] = F[:, 1]          # AB_3 == B: parameter 3 does everything
    s = SR.update(F.reshape(-1, 2, 5), d)
    assert not s["total_sq"][0].any() and s["first_sq"][0].all()
    assert not s["first_sq"][2].any() and s["total_sq"][2].all()
    assert np.array_equal(bits(s["first_sq"][0]), bits(s["total_sq"][2]))          # both are sum (xA - xB)^2, in the same order
    assert s["first_sq"][1].all() and s["total_sq"][1].all()


WORST = {"sumsq": 0.0, "m2": 0.0}


@pytest.mark.parametrize("kind", ["centred", "offset", "tails"])
@pytest.mark.parametrize("n", [1, 100, 4000])
def test_emulation_is_within_the_a_priori_bounds_of_float64(kind, n):
    d, cols = 2, 64
    rng = np.random.default_rng(100 * n + len(kind))
    X = rng.standard_normal((n * (d + 2), 1, cols))
    X = {"centred": X, "offset": 1000.0 + X, "tails": np.exp(3 * X) * rng.choice([-1.0, 1.0], X.shape)}[kind].astype(np.float32)
    s, ref = SR.update(X, d), SR.exact(X, d)
    assert (ref["m2"] > 0).all() and (ref["first_sq"] > 0).all() and (ref["total_sq"] > 0).all()
    r_sq = max((np.abs(s[k].astype(np.float64) - ref[k]) / SR.sumsq_bound(n, ref[k])).max() for k in ("first_sq", "total_sq"))
    r_m2 = (np.abs(s["m2"].astype(np.float64) - ref["m2"]) / SR.welford_bound(2 * n, ref["mean"], ref["m2"])).max()
    WORST["sumsq"], WORST["m2"] = max(WORST["sumsq"], r_sq), max(WORST["m2"], r_m2)
    print(f"{kind} n={n}: worst err / bound  sums of squares {r_sq:.3f}  m2 {r_m2:.3f}  (so far: {WORST})")
    assert r_sq <= 1.0 and r_m2 <= 1.0


def test_estimators_approach_the_analytic_indices_of_a_linear_response():
    """f = a x1 + b x2, x uniform in [0, 1]: V = (a^2 + b^2) / 12, S_1 = ST_1 = a^2 / (a^2 + b^2), S_2 = ST_2 = b^2 / (a^2 + b^2).
    In float64 with N = 1, through SobolResult.

    Tolerance, from the estimators' standard error at n = 20000.  With AB_1 = (xB1, xA2): f(B) - f(AB_1) = b D, D = xB2 - xA2 the
    difference of two uniforms, E D^2 = 1/6, E D^4 = 1/15, so sd(D^2) = sqrt(1/15 - 1/36) = sqrt(7/180).  The numerator of
    1 - S_1, mean_j (b D_j)^2 / 2, has standard error (b^2 / 2) sqrt(7/180) / sqrt(n); relative to V that is
    6 b^2 sqrt(7/180) / ((a^2 + b^2) sqrt(n)).  The denominator, the variance of 2 n values whose kurtosis is below 3 (a sum of
    uniforms), has relative standard error below sqrt((3 - 1) / (2 n)) = 1 / sqrt(n), which enters times 1 - S_1 = b^2 / (a^2 + b^2).
    The two are added (they are correlated), and 5 standard errors are allowed: tol = 5 (6 sqrt(7/180) + 1) w / sqrt(n), w the
    other parameter's share; the same for ST_1 with (a D)^2 and w the parameter's own share."""
    import torch
    a, b, n = 3.0, 1.0, 20000
    A, B = (m.astype(np.float64) for m in sobol_design([0, 0], [1, 1], n, seed=11))
    M = sobol_members(A, B, None).astype(np.float64).reshape(n, 4, 2)
    f = a * M[..., 0] + b * M[..., 1]                                      # [n, 4]: A, B, AB_1, AB_2
    ab = f[:, :2].reshape(-1)
    tens = lambda v: torch.tensor(np.asarray(v, np.float64)).reshape(-1, 1, 1)
    r = SobolResult(count=n, n_params=2, mean=tens(ab.mean())[0], m2=tens(np.square(ab - ab.mean()).sum())[0],
                    first_sq=tens(np.square(f[:, 1:2] - f[:, 2:]).sum(0)), total_sq=tens(np.square(f[:, 0:1] - f[:, 2:]).sum(0)))
    S, ST = r.first_order().reshape(-1).numpy(), r.total_order().reshape(-1).numpy()
    assert S.dtype == np.float64
    share = np.array([a * a, b * b]) / (a * a + b * b)
    k = 5 * (6 * np.sqrt(7 / 180) + 1) / np.sqrt(n)
    print("S", S, "ST", ST, "analytic", share, "tol S", k * share[::-1], "tol ST", k * share)
    assert abs(float(r.var()) - (a * a + b * b) / 12) <= 5 * (a * a + b * b) / 12 / np.sqrt(n)
    assert (np.abs(S - share) <= k * share[::-1]).all() and (np.abs(ST - share) <= k * share).all()
