"""Host side of surrogate ensemble statistics (no GPU): predict.exceed_limit, EnsembleResult, the declaration / binding of the new
entry points, and the numpy float32 emulation of the kernel's arithmetic (tests/ensemble_reference.py) against float64.

The emulation against float64.  Data: k fp32 values per column; reference: the float64 two-pass mean and M2 = sum (x - mean)^2 of
the SAME fp32 values.  u = 2^-24.
  * M2: the a-priori bound of Welford's updating formula, Chan, Golub and LeVeque 1983: relative error of order k u kappa,
    kappa = sqrt(1 + k mean^2 / M2); asserted as  |M2 - ref| <= k u kappa ref  (ensemble_reference.welford_bound), no constant added.
  * mean: mean_k = mean_{k-1} + d r_k commits, to first order, u |mean_k| in the sum and 3 u |d| r_k in d, r_k and their product,
    |d| <= 2 max|x|; the error carried over is multiplied by (1 - 1 / k) <= 1.  Summed over k steps:
    |mean - ref| <= (k + 6 (1 + ln k)) u max|x|.
Worst err / bound over all cases (numpy IEEE arithmetic, the same on any machine): M2 0.92 (k = 2, where the bound is only
2 u kappa; 0.11 at k = 1000), mean 0.078."""
import os
import re
import sys

import numpy as np
import pytest

import simulgen_vae_amd  # noqa: F401
from simulgen_vae_amd import engine as E
from simulgen_vae_amd.predict import EnsembleResult, Surrogate, exceed_limit

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ensemble_reference as ER  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["sgv_ensemble", "sgv_test_recon_ensemble"]
U = 2.0 ** -24
N = 8


def test_scalar_limit_is_broadcast():
    for s in (2.5, np.float32(2.5), np.array(2.5), 3):
        v = exceed_limit(s, N)
        assert v.dtype == np.float32 and v.shape == (N,) and v.flags["C_CONTIGUOUS"] and v.flags["WRITEABLE"] and (v == np.float32(s)).all()


def test_good_vector_is_accepted():
    a = np.linspace(-3, 4, N)
    v = exceed_limit(a, N)
    assert v.dtype == np.float32 and np.array_equal(v, a.astype(np.float32))
    assert np.array_equal(exceed_limit(list(a), N), v) and np.array_equal(exceed_limit(a.astype(np.float32), N), v)


@pytest.mark.parametrize("n", [0, 1, N - 1, N + 1])
def test_wrong_length_is_named(n):
    with pytest.raises(ValueError, match=rf"limit: {n} entries, expected N = {N}"):
        exceed_limit(np.zeros(n), N)


@pytest.mark.parametrize("shape", [(1, N), (N, 1), (2, 2, 2)])
def test_wrong_rank_is_named(shape):
    with pytest.raises(ValueError, match=r"limit: a scalar or a 1-D array of N = 8 entries is required, got shape " + re.escape(str(shape))):
        exceed_limit(np.zeros(shape), N)


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf, 1e39])
def test_non_finite_entry_is_named(bad):
    a = np.zeros(N)
    a[5] = bad
    with pytest.raises(ValueError, match=r"limit\[5\] = .* is not finite"):
        exceed_limit(a, N)
    with pytest.raises(ValueError, match=r"limit = .* is not finite"):
        exceed_limit(bad, N)


def test_ensemble_result_fields_and_groups():
    assert EnsembleResult.FIELDS == ("count", "mean", "m2", "max", "min", "arg_max", "arg_min", "exceed", "limit")
    r = EnsembleResult(**{k: i for i, k in enumerate(EnsembleResult.FIELDS)})
    assert tuple(getattr(r, k) for k in EnsembleResult.FIELDS) == tuple(range(9))
    assert r.groups() == ("moments", "extrema", "exceed")
    with pytest.raises(KeyError):
        EnsembleResult(count=0)
    kw = dict.fromkeys(EnsembleResult.FIELDS)
    kw.update(count=4, max=1, min=2, arg_max=3, arg_min=4)
    r = EnsembleResult(**kw)
    assert r.groups() == ("extrema",) and r.mean is None and r.exceed is None and sorted(r.state()) == ["arg_max", "arg_min", "max", "min"]
    for f in (r.var, r.std, r.exceed_fraction):
        with pytest.raises(ValueError):
            f()


def test_ensemble_result_methods_on_cpu_tensors():
    import torch
    kw = dict.fromkeys(EnsembleResult.FIELDS)
    kw.update(count=5, mean=torch.zeros(2, 3), m2=torch.full((2, 3), 10.0), limit=torch.zeros(3), exceed=torch.full((2, 3), 2, dtype=torch.int32))
    r = EnsembleResult(**kw)
    assert torch.equal(r.var(), torch.full((2, 3), 2.0)) and torch.equal(r.var(ddof=1), torch.full((2, 3), 2.5))
    assert torch.equal(r.std(ddof=1), torch.full((2, 3), 2.5).sqrt())
    assert torch.equal(r.exceed_fraction(), torch.full((2, 3), 0.4))
    with pytest.raises(ValueError, match="count - ddof"):
        r.var(ddof=5)


def test_surrogate_and_engine_have_ensemble():
    assert callable(Surrogate.ensemble) and callable(E.Engine.ensemble)
    assert E.ENSEMBLE_GROUPS == EnsembleResult.GROUPS
    assert "repeat(K, 1)" in Surrogate.ensemble.__doc__ and 'mode="random"' in Surrogate.ensemble.__doc__


def test_new_entry_points_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "sgvae.h")).read()
    for s in NEW_SYMBOLS:
        assert re.search(rf"\bint {s}\s*\(", hdr), s
        assert s in E.ABI_SYMBOLS
    assert re.search(r"\}\s*sgv_ensemble_state;", hdr)
    assert [f for f, _ in E.EnsembleState._fields_] == ["mean", "m2", "max", "min", "arg_max", "arg_min", "limit", "exceed"]
    lib = E.load_library()
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s), s
    assert len(lib.sgv_ensemble.argtypes) == 9 and len(lib.sgv_test_recon_ensemble.argtypes) == 14
    # without an engine the call is an argument error that says who complains
    assert lib.sgv_ensemble(None, None, None, 1, 1, None, None, 0, None) == -1 and "sgv_ensemble" in lib.sgv_last_error().decode()
    assert lib.sgv_test_recon_ensemble(0, None, 8, None, None, None, None, None, 0, None, 1, 1, 8, None) == -1
    assert "sgv_test_recon_ensemble: null argument" in lib.sgv_last_error().decode()


def test_emulation_first_member_and_split_invariance():
    rng = np.random.default_rng(5)
    F = rng.standard_normal((7, 3, N)).astype(np.float32)
    lim = np.zeros(N, np.float32)
    one = ER.update(F[:1], limit=lim)
    assert np.array_equal(one["mean"], F[0]) and not one["m2"].any() and np.array_equal(one["max"], F[0]) and np.array_equal(one["min"], F[0])
    assert not one["arg_max"].any() and np.array_equal(one["exceed"], (F[0] > 0).astype(np.int32))
    whole = ER.update(F, limit=lim)
    part = ER.update(F[3:], ER.update(F[:3], limit=lim), 3, limit=lim)
    for k in ER.STATE:
        assert np.array_equal(whole[k].view(np.int32), part[k].view(np.int32)), k
    assert np.array_equal(whole["max"], F.max(0)) and np.array_equal(whole["arg_max"], F.argmax(0))
    assert np.array_equal(whole["min"], F.min(0)) and np.array_equal(whole["arg_min"], F.argmin(0))
    assert np.array_equal(whole["exceed"], (F > 0).sum(0))


def _data(kind, k, cols, rng):
    if kind == "centred":
        return rng.standard_normal((k, cols))
    if kind == "offset":          # |mean| >> std: mean 1000, std 1
        return 1000.0 + rng.standard_normal((k, cols))
    if kind == "far":             # mean 3e4, std 0.5: kappa about 6e4
        return -3.0e4 + 0.5 * rng.standard_normal((k, cols))
    return np.exp(3 * rng.standard_normal((k, cols))) * rng.choice([-1.0, 1.0], (k, cols))      # heavy tails, both signs


WORST = {"m2": 0.0, "mean": 0.0}


@pytest.mark.parametrize("kind", ["centred", "offset", "far", "tails"])
@pytest.mark.parametrize("k", [2, 3, 10, 100, 1000])
def test_emulation_is_within_the_a_priori_bound_of_welford_updating(kind, k):
    cols = 256
    rng = np.random.default_rng(1000 * k + len(kind))
    X = _data(kind, k, cols, rng).astype(np.float32)
    s = ER.update(X.reshape(k, 1, cols))
    X64 = X.astype(np.float64)
    mean = X64.mean(axis=0)
    M2 = np.square(X64 - mean).sum(axis=0)
    assert (M2 > 0).all()
    r_m2 = np.abs(s["m2"][0].astype(np.float64) - M2) / ER.welford_bound(k, mean, M2)
    r_mean = np.abs(s["mean"][0].astype(np.float64) - mean) / ((k + 6 * (1 + np.log(k))) * U * np.abs(X64).max(axis=0))
    WORST["m2"], WORST["mean"] = max(WORST["m2"], r_m2.max()), max(WORST["mean"], r_mean.max())
    print(f"{kind} k={k}: worst err / bound  M2 {r_m2.max():.3f}  mean {r_mean.max():.3f}  (so far: {WORST})")
    assert r_m2.max() <= 1.0 and r_mean.max() <= 1.0
