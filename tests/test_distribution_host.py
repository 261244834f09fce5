"""Host side of surrogate distributions (no GPU): the numpy float32 emulation of the kernel's rule (tests/distribution_reference.py)
against numpy.histogram and against exact order statistics, predict.hist_range, DistributionResult, and the declaration / binding of
the new entry points.

The quantile.  Data: M fp32 members per column, lo / hi their own minimum / maximum; reference: sort(x)[ceil(q M) - 1] of the SAME fp32
values, the exact order statistic.  Asserted: |quantile - reference| <= w + 4 ulp(max(|lo|, |hi|)), w = (hi - lo) / K the bin width
(distribution_reference.bound, derived in that module's docstring from the rule: both values lie in one bin, at most w apart, plus the
roundings of the rule and of the interpolation).  Worst err / bound over all cases below (numpy IEEE arithmetic, the same on any
machine): 0.9999998, at M = 3, K = 2 -- a member alone in its bin at the lower edge, the interpolated value at the upper."""
import os
import re
import sys

import numpy as np
import pytest

import simulgen_vae_amd  # noqa: F401
from simulgen_vae_amd import engine as E
from simulgen_vae_amd.predict import DistributionResult, EnsembleResult, Surrogate, hist_range, quantile_rank

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import distribution_reference as DR  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["sgv_distribution", "sgv_test_recon_distribution"]
T, N = 3, 8
QS = (0.001, 0.05, 0.25, 0.5, 0.75, 0.95, 1.0)


# ---- the emulation ----
@pytest.mark.parametrize("K", [2, 8, 32, 64])
def test_emulation_equals_numpy_histogram_where_the_edges_are_exact(K):
    rng = np.random.default_rng(K)
    lo, hi = np.full((T, N), -4, np.float32), np.full((T, N), 4, np.float32)          # bin widths 4, 1, 1/4, 1/8: every edge a float
    F = (rng.integers(-4 * 64, 4 * 64 + 1, (50, T, N)) / 64.0).astype(np.float32)     # on a grid of 1/64: x - lo is exact, many values on edges
    F[0], F[1] = lo, hi
    c = DR.update(F, lo, hi, K)
    assert c.dtype == np.int32 and c.shape == (K + 2, T, N) and not c[0].any() and not c[K + 1].any()
    for t in range(T):
        for n in range(N):
            assert np.array_equal(c[1:K + 1, t, n], np.histogram(F[:, t, n].astype(np.float64), bins=K, range=(-4.0, 4.0))[0]), (t, n)
    assert (c[K, :, :] >= 1).all()          # x == hi is in the last bin (numpy's convention), not in overflow


def test_columns_sum_to_the_members_and_any_split_gives_the_same_counts():
    rng = np.random.default_rng(1)
    F = rng.standard_normal((23, T, N)).astype(np.float32)
    lo, hi = np.full((T, N), -0.5, np.float32), np.full((T, N), 1.0, np.float32)      # narrower than the data
    whole = DR.update(F, lo, hi, 7)
    assert np.array_equal(whole.sum(0), np.full((T, N), 23))
    assert np.array_equal(whole[0], (F < lo).sum(0)) and np.array_equal(whole[8], (F > hi).sum(0)) and whole[0].any() and whole[8].any()
    part = DR.update(F[9:], lo, hi, 7, DR.update(F[5:9], lo, hi, 7, DR.update(F[:5], lo, hi, 7)))
    assert np.array_equal(whole, part)
    base = rng.integers(0, 100, whole.shape).astype(np.int32)                          # a state that is not zero is added to
    assert np.array_equal(DR.update(F, lo, hi, 7, base), base + whole) and base.max() < 100


def test_a_degenerate_range_puts_equal_values_in_bin_one():
    lo = np.full((T, N), 2.5, np.float32)
    F = np.full((4, T, N), 2.5, np.float32)
    F[3, 0, 0], F[2, 0, 1] = 3.0, 2.0
    c = DR.update(F, lo, lo, 5)
    want = np.zeros_like(c)
    want[1] = 4
    want[1, 0, 0], want[6, 0, 0], want[1, 0, 1], want[0, 0, 1] = 3, 1, 3, 1
    assert np.array_equal(c, want)
    assert np.array_equal(DR.quantile(DR.update(F[:2], lo, lo, 5), lo, lo, 0.5, 2), lo)


def _members(M, cols, rng):
    """M members in `cols` columns: centred, heavy-tailed, offset by up to 10^3 sigma, one column degenerate, one of two values"""
    sigma = np.exp(rng.uniform(-3, 3, cols))
    off = sigma * np.concatenate([np.zeros(cols // 4), rng.uniform(-1e3, 1e3, cols - cols // 4)])
    X = off + sigma * rng.standard_normal((M, cols))
    X[:, 1] = np.exp(3 * rng.standard_normal(M))
    X[:, 2] = 7.25
    X[:, 3] = rng.choice([-1.0, 1.0], M)
    return X.astype(np.float32)


WORST = {"ratio": 0.0}


@pytest.mark.parametrize("K", [2, 3, 8, 32, 64])
@pytest.mark.parametrize("M", [1, 2, 3, 5, 16, 40, 200])
def test_quantile_is_within_a_bin_width_of_the_exact_order_statistic(M, K):
    cols = 64
    rng = np.random.default_rng(100 * M + K)
    F = _members(M, cols, rng).reshape(M, 1, cols)
    lo, hi = F.min(0), F.max(0)
    c = DR.update(F, lo, hi, K)
    assert not c[0].any() and not c[K + 1].any() and np.array_equal(c.sum(0), np.full((1, cols), M))
    bound = DR.bound(lo, hi, K)
    for q in QS:
        got = DR.quantile(c, lo, hi, q, M)
        assert got.dtype == np.float32 and (got >= lo).all() and (got <= hi).all()
        err = np.abs(got.astype(np.float64) - DR.order_statistic(F, q).astype(np.float64))
        ratio = float((err / np.where(bound > 0, bound, 1.0)).max())
        WORST["ratio"] = max(WORST["ratio"], ratio)
        print(f"M={M} K={K} q={q}: worst err / bound {ratio:.7f} (so far {WORST['ratio']:.7f})")
        assert (err <= bound).all(), (q, int(np.argmax(err - bound)))
    assert np.array_equal(DR.quantile(c, lo, hi, 0.5, M)[:, 2], np.full(1, 7.25, np.float32))          # the degenerate column, exactly


def test_quantile_rank():
    assert [quantile_rank(q, 6) for q in (1e-9, 0.5, 0.51, 1.0)] == [1, 3, 4, 6]
    assert quantile_rank(0.05, 200) == 10 and quantile_rank(0.95, 200) == 190 and quantile_rank(0.5, 1) == 1
    assert all(quantile_rank(q, M) == DR.rank(q, M) for q in QS for M in (1, 2, 3, 5, 16, 40, 200))


# ---- hist_range ----
def test_hist_range_accepts_scalars_vectors_and_fields():
    lo, hi = hist_range((-1, 2.5), T, N)
    assert lo.dtype == hi.dtype == np.float32 and lo.shape == hi.shape == (T, N) and (lo == -1).all() and (hi == 2.5).all()
    assert lo.flags["C_CONTIGUOUS"] and lo.flags["WRITEABLE"]
    a = np.linspace(-3, 4, N)
    lo, hi = hist_range([a, a + 1], T, N)
    assert np.array_equal(lo, np.broadcast_to(a.astype(np.float32), (T, N))) and np.array_equal(hi[2], (a + 1).astype(np.float32))
    assert lo.flags["C_CONTIGUOUS"] and hi.flags["C_CONTIGUOUS"] and hi.flags["WRITEABLE"]
    f = np.arange(T * N, dtype=np.float64).reshape(T, N)
    lo, hi = hist_range((f, f), T, N)          # hi == lo is allowed
    assert np.array_equal(lo, f.astype(np.float32)) and np.array_equal(hi, lo)
    lo, hi = hist_range((0.0, f), T, N)        # the two bounds need not have one form
    assert not lo.any() and np.array_equal(hi, f.astype(np.float32))


def test_hist_range_names_what_is_wrong():
    for bad in (None, 3.0, (1, 2, 3), [1], np.zeros((2, T, N))[:1], {"lo": 0, "hi": 1}):
        with pytest.raises(ValueError, match="range: an EnsembleResult with the extrema or a pair"):
            hist_range(bad, T, N)
    with pytest.raises(ValueError, match=rf"range: hi: {N - 1} entries, expected N = {N}"):
        hist_range((0, np.zeros(N - 1)), T, N)
    with pytest.raises(ValueError, match=r"range: lo has shape \(8, 3\), expected \[T, N\] = \[3, 8\]"):
        hist_range((np.zeros((N, T)), np.ones((N, T))), T, N)
    with pytest.raises(ValueError, match=r"range: lo: a scalar, a 1-D array .* got shape \(1, 3, 8\)"):
        hist_range((np.zeros((1, T, N)), 1), T, N)
    for v in (np.nan, np.inf, -np.inf, 1e39):
        with pytest.raises(ValueError, match=r"range: hi = .* is not finite"):
            hist_range((0, v), T, N)
        a = np.zeros(N)
        a[5] = v
        with pytest.raises(ValueError, match=r"range: lo\[5\] = .* is not finite"):
            hist_range((a, 1e30), T, N)
        f = np.zeros((T, N))
        f[1, 6] = v
        with pytest.raises(ValueError, match=r"range: hi\[1, 6\] = .* is not finite"):
            hist_range((-1e30, f), T, N)
    hi = np.ones((T, N))
    hi[2, 3] = hi[2, 5] = -0.5
    with pytest.raises(ValueError, match=r"range: hi < lo at \[t, n\] = \[2, 3\]: lo = 0.0, hi = -0.5"):
        hist_range((0, hi), T, N)
    with pytest.raises(ValueError, match=r"range: hi < lo at \[t, n\] = \[0, 0\]"):
        hist_range((1, 0), T, N)


def test_hist_range_takes_the_extrema_of_an_ensemble_result():
    """on the host its tensors are read like arrays; on the device they are handed on as they are (tests/test_distribution_gpu.py)"""
    import torch
    kw = dict.fromkeys(EnsembleResult.FIELDS)
    mn, mx = torch.zeros(T, N), torch.ones(T, N)
    kw.update(count=4, max=mx, min=mn, arg_max=torch.zeros(T, N, dtype=torch.int32), arg_min=torch.zeros(T, N, dtype=torch.int32))
    lo, hi = hist_range(EnsembleResult(**kw), T, N)
    assert np.array_equal(lo, mn.numpy()) and np.array_equal(hi, mx.numpy())
    kw.update(max=mn, min=mx)
    with pytest.raises(ValueError, match=r"range: hi < lo at \[t, n\] = \[0, 0\]"):
        hist_range(EnsembleResult(**kw), T, N)
    kw.update(max=None, min=None)
    with pytest.raises(ValueError, match="does not hold the extrema"):
        hist_range(EnsembleResult(**kw), T, N)


# ---- the result type ----
def _result(F, K, lo=None, hi=None):
    import torch
    lo = F.min(0) if lo is None else lo
    hi = F.max(0) if hi is None else hi
    c = DR.update(F, lo, hi, K)
    return DistributionResult(count=F.shape[0], bins=K, lo=torch.from_numpy(lo), hi=torch.from_numpy(hi), counts=torch.from_numpy(c)), c, lo, hi


def test_distribution_result_on_cpu_tensors_equals_the_emulation():
    import torch
    assert DistributionResult.FIELDS == ("count", "bins", "lo", "hi", "counts") and DistributionResult.STATE == ("lo", "hi", "counts")
    rng = np.random.default_rng(3)
    F = _members(40, N, rng).reshape(40, 1, N).repeat(T, 1)
    for K in (2, 7, 64):
        r, c, lo, hi = _result(F, K)
        assert sorted(r.state()) == ["counts", "hi", "lo"] and r.state()["counts"] is r.counts
        assert r.under.shape == (T, N) and not r.under.any() and not r.over.any() and r.over.data_ptr() == r.counts[K + 1].data_ptr()
        assert torch.equal(r.fractions(), r.counts[1:K + 1].float() / 40.0) and r.fractions().shape == (K, T, N)
        q3 = r.quantile([0.05, 0.5, 0.95])
        assert q3.shape == (3, T, N) and q3.dtype == torch.float32
        for i, q in enumerate((0.05, 0.5, 0.95)):
            assert np.array_equal(q3[i].numpy().view(np.int32), DR.quantile(c, lo, hi, q, 40).view(np.int32)), (K, q)
        assert r.quantile(0.5).shape == (T, N) and torch.equal(r.quantile(0.5), q3[1]) and torch.equal(r.median(), q3[1])
        r.CHUNK = (K + 2) * N          # one time step per piece
        assert torch.equal(r.quantile([0.05, 0.5, 0.95]), q3)
    # a range narrower than the data: quantiles below lo / above hi come back as lo / hi
    lo, hi = np.full((T, N), -1e9, np.float32), np.full((T, N), -1e8, np.float32)
    r, c, _, _ = _result(F, 4, lo, hi)
    assert bool((r.over == 40).all()) and torch.equal(r.quantile(0.5), r.hi)
    r, c, _, _ = _result(F, 4, -hi, -lo)
    assert bool((r.under == 40).all()) and torch.equal(r.quantile(0.5), r.lo)


def test_distribution_result_errors():
    import torch
    with pytest.raises(KeyError):
        DistributionResult(count=0)
    empty = DistributionResult(count=0, bins=4, lo=torch.zeros(T, N), hi=torch.ones(T, N), counts=torch.zeros(6, T, N, dtype=torch.int32))
    for f in (empty.fractions, empty.median, lambda: empty.quantile(0.5)):
        with pytest.raises(ValueError, match="the distribution is empty"):
            f()
    r = _result(np.zeros((2, T, N), np.float32), 4)[0]
    for q in (0.0, -0.1, 1.0000001, np.nan, [0.5, 2.0]):
        with pytest.raises(ValueError, match=r"is outside \(0, 1\]"):
            r.quantile(q)
    for q in ([], [[0.5]]):
        with pytest.raises(ValueError, match="q must be a scalar or a non-empty 1-D sequence"):
            r.quantile(q)
    with pytest.raises(ValueError, match="into must be a DistributionResult, not dict"):
        DistributionResult.require({})
    with pytest.raises(ValueError, match=r"into.counts must be a contiguous"):
        r.continued({"counts": ((6, T, N), torch.int32)})          # not on the device


def test_surrogate_and_engine_have_distribution():
    assert callable(Surrogate.distribution) and callable(E.Engine.distribution)
    assert (E.DISTRIBUTION_MIN_BINS, E.DISTRIBUTION_MAX_BINS) == (2, 64)
    assert "quantile([0.05, 0.5, 0.95])" in Surrogate.distribution.__doc__


def test_new_entry_points_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "sgvae.h")).read()
    for s in NEW_SYMBOLS:
        assert re.search(rf"\bint {s}\s*\(", hdr), s
        assert s in E.ABI_SYMBOLS
    assert re.search(r"\}\s*sgv_distribution_state;", hdr)
    assert [f for f, _ in E.DistributionState._fields_] == ["lo", "hi", "counts", "bins"]
    lib = E.load_library()
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s), s
    assert len(lib.sgv_distribution.argtypes) == 9 and len(lib.sgv_test_recon_distribution.argtypes) == 14
    # without an engine the call is an argument error that says who complains
    assert lib.sgv_distribution(None, None, None, 1, 1, None, None, 0, None) == -1 and "sgv_distribution" in lib.sgv_last_error().decode()
    assert lib.sgv_test_recon_distribution(0, None, 8, None, None, None, None, None, 0, None, 1, 1, 8, None) == -1
    assert "sgv_test_recon_distribution: null argument" in lib.sgv_last_error().decode()
