"""Surrogate response surfaces on the GPU: Engine.regress (sgv_regress) against the numpy float32 emulation of the kernel's
arithmetic (tests/regression_reference.py) run on what Engine.generate writes on the same engine, latents and injected noise; what
a call leaves behind in the engine; and Surrogate.regress against the emulation on Surrogate.predict, against Surrogate.ensemble,
and its derived quantities against a float64 least-squares fit of the predicted fields, on the models of
tests/golden/predict_small.npz.

The state -- mean, m2, comoment -- is compared bit for bit everywhere.  predict draws the decoder's noise per call and a study by
member index (tests/test_ensemble_gpu.py), so the comparisons with predict make one call of it, batch >= P.

coefficients() against numpy.linalg.lstsq in float64 on predict's fields and the unrounded covariates (P = 24, K = 3 uniform
covariates): within the co-moment's a-priori bound -- with the rounding of the weights to fp32 -- propagated through |gram^-1|
plus the fp32 rounding of the K-term product (regression_reference.derived_bounds); r2() in [0, 1 + its slack]."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import simulgen_vae_amd  # noqa: F401
from simulgen_vae_amd import engine as E
from simulgen_vae_amd.predict import RegressionResult, regression_weights
from tests.gpu_common import G0, make_cfg
from tests.surrogate_common import (MAXB, bits, engine, latents, no_forward_after, same_result, signed_scaler, state_as_numpy, surrogate,
                                    training_unaffected)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ensemble_reference as ER  # noqa: E402
import regression_reference as RR  # noqa: E402

pytestmark = pytest.mark.gpu


def new_state(T, N, K):
    """the tensors of Engine.regress's state, filled with what a call from empty must not read"""
    return {"mean": torch.full((T, N), float("nan"), device="cuda"), "m2": torch.full((T, N), float("nan"), device="cuda"),
            "comoment": torch.full((K, T, N), float("nan"), device="cuda")}


def covariates(P, K, seed=0):
    """Y float64 [P, K], uniform in [-1, 1] with the last column a thousand times that"""
    Y = np.random.default_rng(seed).uniform(-1.0, 1.0, (P, K))
    Y[:, K - 1] *= 1000.0
    return Y


def as_numpy(res):
    return state_as_numpy(res, RR.STATE)


def assert_state(got, want):
    for k in RR.STATE:
        assert got[k].dtype == np.float32 and np.array_equal(bits(got[k]), bits(want[k])), k


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("B", [1, 3, MAXB])
@pytest.mark.parametrize("name", ["G0", "G1"])
def test_regress_is_the_emulation_on_what_generate_writes(name, B, dtype):
    cfg, eng = engine(name, dtype)
    T, N = cfg.num_time, cfg.num_node
    z, xs, eps = latents(cfg, B)
    scale, mn = (torch.from_numpy(a).cuda() for a in signed_scaler(N))
    eng.set_eps(eps)
    F = eng.generate(z, xs, scale, mn, fix=True).cpu().numpy()
    for K in (1, 3, 32):
        W, ybar, gram = regression_weights(np.concatenate([covariates(B, K), covariates(B, K, 1)]))
        st = new_state(T, N, K)
        eng.set_eps(eps)
        res = eng.regress(z, xs, scale, mn, st, torch.from_numpy(W[:B]).cuda(), 0, fix=True)
        assert res is st and sorted(res) == sorted(RR.STATE)
        want = RR.update(F, W[:B])
        assert_state(as_numpy(res), want)
        # the same members again, as members B .. 2B - 1 with other covariates: the state is read and continued
        eng.set_eps(eps)
        eng.regress(z, xs, scale, mn, st, torch.from_numpy(W[B:]).cuda(), B, fix=True)
        assert_state(as_numpy(st), RR.update(F, W[B:], want, B))
    # and the moments are the ensemble's
    ens = {"mean": torch.empty((T, N), device="cuda"), "m2": torch.empty((T, N), device="cuda")}
    for cb in (0, B):
        eng.set_eps(eps)
        eng.ensemble(z, xs, scale, mn, ens, cb, fix=True)
    assert all(torch.equal(ens[k].view(torch.int32), st[k].view(torch.int32)) for k in ens)


def test_regress_checks_its_arguments():
    cfg, eng = engine("G0", "f32")
    z, xs, eps = latents(cfg, 2)
    scale, mn = (torch.from_numpy(a).cuda() for a in signed_scaler(cfg.num_node))
    T, N, K = cfg.num_time, cfg.num_node, 3
    st = new_state(T, N, K)
    w = torch.zeros((2, K), device="cuda")
    with pytest.raises(ValueError, match="state must be a dict"):
        eng.regress(z, xs, scale, mn, {}, w, 0)
    with pytest.raises(ValueError, match="is not a tensor of the regression state"):
        eng.regress(z, xs, scale, mn, dict(st, var=st["m2"]), w, 0)
    for k in st:
        with pytest.raises(ValueError, match="needs all of"):
            eng.regress(z, xs, scale, mn, {n: v for n, v in st.items() if n != k}, w, 0)
    for k, bad in (("mean", st["mean"][:-1]), ("m2", st["m2"].double()), ("comoment", st["comoment"].cpu()), ("mean", st["mean"].t())):
        with pytest.raises(ValueError, match=rf"state\['{k}'\] must be a contiguous"):
            eng.regress(z, xs, scale, mn, dict(st, **{k: bad}), w, 0)
    with pytest.raises(ValueError, match=r"has 33 rows: n_cov is outside \[1, 32\]"):
        eng.regress(z, xs, scale, mn, dict(st, comoment=torch.zeros((33, T, N), device="cuda")), w, 0)
    for bad in (w[:1], w[:, :2], w.double(), w.cpu(), torch.zeros((2, 2 * K), device="cuda")[:, ::2]):
        with pytest.raises(ValueError, match="weights must be a contiguous float32 CUDA tensor of shape"):
            eng.regress(z, xs, scale, mn, st, bad, 0)
    with pytest.raises(ValueError, match="scale must be"):
        eng.regress(z, xs, scale[:-1], mn, st, w, 0)
    for cb in (-1, (1 << 24) - 1):
        with pytest.raises(ValueError, match="count_before"):
            eng.regress(z, xs, scale, mn, st, w, cb)
    # the C entry point itself: SGV_ERR_ARG before anything is enqueued, so the forward of a decode stays readable
    eng.set_eps(eps)
    eng.decode(z, xs, fix=True)
    xs_t = torch.stack(xs).contiguous()
    keep = {k: v.clone() for k, v in st.items()}
    ptr = {k: v.data_ptr() for k, v in st.items()}
    args = [z.data_ptr(), xs_t.data_ptr(), 2, 1, scale.data_ptr(), mn.data_ptr(), K, w.data_ptr(), 0]

    def rejected(msg, so=True, **kw):
        a = list(args)
        p = dict(ptr)
        for i, v in kw.items():
            if i in p:
                p[i] = v
            else:
                a[int(i[1:])] = v
        assert eng.lib.sgv_regress(eng.h, *a, C.byref(E.RegressState(**p)) if so else None) == -1
        assert msg in eng.lib.sgv_last_error().decode(), eng.lib.sgv_last_error().decode()

    rejected("null argument", so=False)
    for i in (0, 4, 5, 7):          # z, scale, min, weights
        rejected("null argument", **{f"a{i}": None})
    rejected("needs xs", a1=None)
    rejected("outside [0, 2^24]", a2=0)
    for k in ptr:
        rejected("mean, m2 and comoment are all required", **{k: None})
        rejected("misaligned pointer", **{k: ptr[k] + 4})
    rejected("misaligned pointer", a7=w.data_ptr() + 2)
    rejected("n_cov = 0 is outside [1, 32]", a6=0)
    rejected("n_cov = 33 is outside [1, 32]", a6=33)
    rejected("outside [0, 2^24]", a8=-1)
    rejected("outside [0, 2^24]", a8=(1 << 24) - 1)
    assert eng.lib.sgv_regress(None, *args, C.byref(E.RegressState(**ptr))) == -1
    eng.xhat()
    torch.cuda.synchronize()
    assert all(torch.equal(st[k].view(torch.int32), keep[k].view(torch.int32)) for k in st)


def test_no_forward_to_read_after_regress_and_generate_is_unchanged():
    cfg, eng = engine("G0", "bf16")
    st = new_state(cfg.num_time, cfg.num_node, 2)
    w = torch.ones((2, 2), device="cuda")
    no_forward_after(eng, cfg, lambda z, xs, scale, mn, before: eng.regress(z, xs, scale, mn, st, w, 0),
                     (eng.xhat, lambda: eng.activation("x_hat", (2, cfg.num_node, cfg.num_time)), lambda: eng.backward(1.0, 1.0)))


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_training_is_unaffected_by_regress(dtype):
    cfg = make_cfg(G0)
    st = new_state(cfg.num_time, cfg.num_node, 3)
    w = torch.from_numpy(regression_weights(covariates(4, 3))[0]).cuda()
    training_unaffected(dtype, lambda eng, z, xs, scale, mn, i: eng.regress(z, xs, scale, mn, st, w[2 * i:2 * i + 2].contiguous(), 2 * i), False)


# ---- Surrogate.regress ----
def expected(F, Y):
    """the emulation's state and the host's half for members F with covariates Y"""
    W, ybar, gram = regression_weights(Y)
    return RR.update(F, W), W, ybar, gram


@pytest.mark.parametrize("kind", ["img", "mlp"])
def test_regress_is_the_emulation_on_what_predict_writes(kind):
    s, x, g = surrogate(kind, "bf16", batch=8, seed=3)           # one call of predict: its draws are the study's
    F = s.predict(x, mode="fix").cpu().numpy()
    P, T, N = F.shape
    s, x, _ = surrogate(kind, "bf16", batch=4, seed=3)           # a new Surrogate re-seeds the engine; 6 members as 4 + 2
    if kind == "img":
        with pytest.raises(ValueError, match="conditions have 256 columns, more than 32: give explicit covariates"):
            s.regress(x)
        Y = covariates(P, 2, 5)
        res = s.regress(x, covariates=Y)
    else:
        Y = np.asarray(x, np.float64)                            # the 7 columns of the conditions themselves
        res = s.regress(x)
    want, W, ybar, gram = expected(F, Y)
    assert isinstance(res, RegressionResult) and res.count == P and res.n_cov == Y.shape[1]
    assert res.mean.shape == res.m2.shape == (T, N) and res.comoment.shape == (Y.shape[1], T, N) and res.comoment.is_contiguous()
    assert_state(as_numpy(res), want)
    assert res.cov_mean.dtype == res.cov_gram.dtype == np.float64
    assert np.array_equal(res.cov_mean, ybar) and np.array_equal(res.cov_gram, gram)
    assert torch.equal(res.var(), res.m2 / float(P)) and torch.equal(res.std(ddof=1), (res.m2 / float(P - 1)).sqrt())
    assert torch.equal(res.covariance(ddof=1), res.comoment / float(P - 1))
    if kind == "img":
        assert res.coefficients().shape == (2, T, N) and res.r2().shape == (T, N) and res.correlation().shape == (2, T, N)
    else:
        with pytest.raises(ValueError, match="count = 6 members do not determine 7 coefficients"):
            res.coefficients()


@pytest.mark.parametrize("kind", ["img", "mlp"])
def test_in_random_mode_the_moments_are_the_ensembles(kind):
    s, x, _ = surrogate(kind, "f32", batch=4, seed=21)
    ens = s.ensemble(x, want=("moments",), mode="random")
    s, x, _ = surrogate(kind, "f32", batch=4, seed=21)
    res = s.regress(x, covariates=covariates(6, 3), mode="random")
    assert torch.equal(res.mean.view(torch.int32), ens.mean.view(torch.int32)) and torch.equal(res.m2.view(torch.int32), ens.m2.view(torch.int32))
    s, x, _ = surrogate(kind, "f32", batch=4, seed=21)
    assert not torch.equal(s.regress(x, covariates=covariates(6, 3), mode="fix").m2, res.m2)


def design(P=24, seed=9):
    """P conditions of the parametric model, uniform over the range of its training set; the first three columns are the covariates"""
    return np.random.default_rng(seed).uniform(-0.7, 0.7, (P, 7)).astype(np.float32)


@pytest.mark.parametrize("mode", ["fix", "random"])
def test_batch_size_does_not_show_in_the_result(mode):
    x = design()
    s, _, _ = surrogate("mlp", "f32", batch=16, seed=11)
    a = s.regress(x, mode=mode)                                  # 24 members as 16 + 8: launches of 8 members in fp32
    s, _, _ = surrogate("mlp", "f32", batch=5, seed=11)
    b = s.regress(x, mode=mode)                                  # 5 + 5 + 5 + 5 + 4
    assert a.count == b.count == 24 and a.n_cov == 7
    same_result_with_host(a, b)
    s, _, _ = surrogate("mlp", "bf16", batch=16, seed=11)
    a = s.regress(x, mode=mode)                                  # bf16: one launch of 16 and one of 8
    s, _, _ = surrogate("mlp", "bf16", batch=5, seed=11)
    same_result_with_host(a, s.regress(x, mode=mode))


def same_result_with_host(a, b):
    """same_result for the device tensors and the count, bitwise equality for the host's float64 arrays"""
    for r in (a, b):
        assert r.cov_mean.dtype == np.float64 and r.cov_gram.dtype == np.float64
    assert np.array_equal(a.cov_mean.view(np.int64), b.cov_mean.view(np.int64)) and np.array_equal(a.cov_gram.view(np.int64), b.cov_gram.view(np.int64))
    strip = lambda r: RegressionResult(count=r.count, mean=r.mean, m2=r.m2, comoment=r.comoment, cov_mean=0, cov_gram=0)
    same_result(strip(a), strip(b))


def test_into_continues_and_equals_one_call_and_host_inputs_equal_device_inputs():
    s, x, g = surrogate("mlp", "f32", seed=11)
    Y = covariates(6, 3, 2)
    whole = s.regress(x, covariates=Y)                           # 6 conditions at batch 4: 4 + 2; host conditions and covariates (numpy)
    assert whole.count == 6 and whole.mean.shape == (12, 520)
    for cut in (1, 3, 5):                                        # cuts that are no batch boundary of the single call
        s, x, _ = surrogate("mlp", "f32", seed=11)
        first = s.regress(x[:cut], covariates=Y[:cut])
        ptrs = {k: v.data_ptr() for k, v in first.state().items()}
        second = s.regress(torch.from_numpy(x[cut:]).cuda(), covariates=torch.from_numpy(Y[cut:]).cuda(), into=first)      # device inputs
        assert second.count == 6 and {k: v.data_ptr() for k, v in second.state().items()} == ptrs          # the same tensors, updated in place
        same_result_with_host(whole, second)
    s, x, _ = surrogate("mlp", "f32", seed=11)
    same_result_with_host(whole, s.regress(torch.from_numpy(x).cuda(), covariates=torch.from_numpy(Y)))
    # the conditions' own columns from the device are those from the host
    s, x, _ = surrogate("mlp", "f32", seed=11)
    own = s.regress(x)
    s, x, _ = surrogate("mlp", "f32", seed=11)
    same_result_with_host(own, s.regress(torch.from_numpy(x).cuda()))
    assert torch.equal(own.mean.view(torch.int32), whole.mean.view(torch.int32))
    with pytest.raises(ValueError, match="into must be a RegressionResult"):
        s.regress(x, into=whole.state())
    with pytest.raises(ValueError, match="into holds 3 covariates, this call has 7"):
        s.regress(x, into=whole)
    with pytest.raises(ValueError, match="covariates: 5 rows, expected P = 6"):
        s.regress(x, covariates=Y[:5])
    with pytest.raises(ValueError, match=r"covariates\[2, 1\] = nan is not finite"):
        s.regress(x, covariates=np.where(np.arange(18).reshape(6, 3) == 7, np.nan, Y))
    with pytest.raises(ValueError, match="mode must be"):
        s.regress(x, mode="mean")
    with pytest.raises(ValueError, match=r"into.cov_mean / into.cov_gram must be \[K\] / \[K, K\]"):
        s.regress(x, covariates=Y, into=RegressionResult(count=6, mean=whole.mean, m2=whole.m2, comoment=whole.comoment, cov_mean=np.zeros(2), cov_gram=whole.cov_gram))
    with pytest.raises(ValueError, match="into.mean must be a contiguous"):
        s.regress(x, covariates=Y, into=RegressionResult(count=6, mean=whole.mean.cpu(), m2=whole.m2, comoment=whole.comoment, cov_mean=whole.cov_mean,
                                                         cov_gram=whole.cov_gram))
    empty = s.regress(x[:0], covariates=Y[:0])
    assert empty.count == 0 and not empty.comoment.any() and not empty.cov_gram.any()
    same_result_with_host(whole, surrogate("mlp", "f32", seed=11)[0].regress(x, covariates=Y, into=empty))


def test_a_probe_history_is_a_covariate():
    """what co-varies with the response at a probe node: the column of sweep()'s probe history at one time step"""
    s, x, _ = surrogate("mlp", "f32", batch=8, seed=11)
    F = s.predict(x, mode="fix").cpu().numpy()
    node, t = 17, 5
    s, x, _ = surrogate("mlp", "f32", batch=8, seed=11)
    hist = s.sweep(x, probes=[node]).probes                      # [P, T, 1] on the device
    assert np.array_equal(bits(hist[:, :, 0].cpu().numpy()), bits(F[:, :, node]))
    s, x, _ = surrogate("mlp", "f32", batch=4, seed=11)
    res = s.regress(x, covariates=hist[:, t, :])
    Y = F[:, t, node:node + 1].astype(np.float64)
    want, W, ybar, gram = expected(F, Y)
    assert_state(as_numpy(res), want)
    assert np.array_equal(res.cov_mean, ybar) and np.array_equal(res.cov_gram, gram)
    # the field at the probe regressed on itself: slope 1 and explained completely, within the propagated bound
    dbeta, _, dr2 = derived(F, W, ybar, res.gram_inverse())
    beta, r2 = res.coefficients()[0, t, node].item(), res.r2()[t, node].item()
    assert abs(beta - 1.0) <= dbeta[0, t, node] < 1e-3 and abs(r2 - 1.0) <= dr2[t, node] < 1e-3


def derived(F, W, ybar, ginv):
    """regression_reference.derived_bounds for the members F with weights W (rounded from float64 covariates)"""
    ref, _, _ = RR.update64(F, W)
    n = F.shape[0]
    return RR.derived_bounds(ginv, ref["comoment"], RR.comoment_bound(F, W, rounded_weights=True), ybar, ref["mean"], ref["m2"],
                             ER.welford_bound(n, ref["mean"], ref["m2"]), n, np.abs(F).max(0).astype(np.float64))


def test_coefficients_are_the_least_squares_fit_of_the_predicted_fields():
    x = design()
    P, K = 24, 3
    s, _, _ = surrogate("mlp", "f32", batch=24, seed=11)
    F = s.predict(x, mode="fix").cpu().numpy()
    T, N = F.shape[1:]
    s, _, _ = surrogate("mlp", "f32", batch=16, seed=11)
    Y = np.asarray(x[:, :K], np.float64)
    res = s.regress(x, covariates=x[:, :K])
    want, W, ybar, gram = expected(F, Y)
    assert_state(as_numpy(res), want)
    # float64 least squares with an intercept on the same fields and the unrounded covariates
    A = np.concatenate([np.ones((P, 1)), Y], axis=1)
    sol = np.linalg.lstsq(A, F.reshape(P, T * N).astype(np.float64), rcond=None)[0]
    icpt64, beta64 = sol[0].reshape(T, N), sol[1:].reshape(K, T, N)
    F64 = F.astype(np.float64)
    m2_64 = np.square(F64 - F64.mean(0)).sum(0)
    resid = F64.reshape(P, -1) - A @ sol
    r2_64 = 1.0 - np.square(resid).sum(0).reshape(T, N) / m2_64
    assert np.linalg.cond(gram) < 10.0                           # the design is well conditioned
    dbeta, dicpt, dr2 = derived(F, W, ybar, res.gram_inverse())
    beta, icpt, r2 = res.coefficients().cpu().numpy(), res.intercept().cpu().numpy(), res.r2().cpu().numpy()
    eb, ei, er = np.abs(beta - beta64), np.abs(icpt - icpt64), np.abs(r2 - r2_64)
    print("worst err / bound: coefficients", (eb / dbeta).max(), "intercept", (ei / dicpt).max(), "r2", (er / dr2).max())
    assert (eb <= dbeta).all() and (ei <= dicpt).all() and (er <= dr2).all()
    assert (dbeta <= 1e-3 * np.abs(beta64).max()).all()          # and the bound means something
    assert (r2 >= 0.0).all() and (r2 <= 1.0 + dr2).all()
    assert (m2_64 > 0).all()


def test_a_constant_covariate_is_refused():
    s, x, _ = surrogate("mlp", "f32", seed=11)
    Y = covariates(6, 2, 4)
    Y[:, 1] = 2.5
    res = s.regress(x, covariates=Y)
    assert res.cov_gram[1, 1] == 0.0
    for f in (res.coefficients, res.intercept, res.r2):
        with pytest.raises(ValueError, match=r"covariate 1 does not vary \(gram\[1, 1\] = 0.0\)"):
            f()
    assert torch.isfinite(res.covariance()).all() and not res.comoment[1].any()          # its weights are exactly zero
