"""Surrogate distributions on the GPU: Engine.distribution (sgv_distribution) against the numpy float32 emulation of the rule
(tests/distribution_reference.py) run on what Engine.generate writes on the same engine, latents and injected noise; what a call
leaves behind in the engine; and Surrogate.distribution between the envelope Surrogate.ensemble found, against the emulation and
against sorted fields of Surrogate.predict on the models of tests/golden/predict_small.npz.

Counts are compared bit for bit.  The quantile is compared with the exact order statistic sort(F, 0)[ceil(q P) - 1] of predict's
fields within w + 4 ulp(max(|lo|, |hi|)), w the bin width (distribution_reference.bound and the derivation there).

Noise: as tests/test_ensemble_gpu.py explains, a member's noise follows its index in the study, so the distribution pass sees the
fields of the ensemble pass on the same seed bit for bit -- nothing lies outside the envelope, in mode "random" too -- and both equal
Surrogate.predict exactly when predict makes one call (batch >= P)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import simulgen_vae_amd  # noqa: F401
from simulgen_vae_amd import engine as E
from simulgen_vae_amd.predict import DistributionResult
from tests.gpu_common import G0, make_cfg
from tests.surrogate_common import MAXB, engine, latents, no_forward_after, same_result, signed_scaler, surrogate, training_unaffected

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import distribution_reference as DR  # noqa: E402

pytestmark = pytest.mark.gpu


def new_state(lo, hi, K):
    lo, hi = (torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda() for a in (lo, hi))
    return {"lo": lo, "hi": hi, "counts": torch.zeros((K + 2,) + tuple(lo.shape), dtype=torch.int32, device="cuda")}


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("B,K", [(1, 7), (3, 2), (MAXB, 32), (MAXB, 64)])
@pytest.mark.parametrize("name", ["G0", "G1"])
def test_distribution_counts_what_generate_writes(name, B, K, dtype):
    cfg, eng = engine(name, dtype)
    T, N = cfg.num_time, cfg.num_node
    z, xs, eps = latents(cfg, B)
    scale, mn = (torch.from_numpy(a).cuda() for a in signed_scaler(N))
    eng.set_eps(eps)
    F = eng.generate(z, xs, scale, mn, fix=True).cpu().numpy()
    lo, hi = F.min(0), F.max(0)
    st = new_state(lo, hi, K)
    eng.set_eps(eps)
    res = eng.distribution(z, xs, scale, mn, st, 0, fix=True)
    assert res is st
    got = st["counts"].cpu().numpy()
    assert np.array_equal(got, DR.update(F, lo, hi, K))
    assert not got[0].any() and not got[K + 1].any() and np.array_equal(got.sum(0), np.full((T, N), B))
    # the same members again into the same state, between narrower bounds: the pass adds to what is there
    span = hi - lo
    lo2, hi2 = (lo + np.float32(0.25) * span).astype(np.float32), (hi - np.float32(0.25) * span).astype(np.float32)
    st2 = dict(new_state(lo2, hi2, K), counts=st["counts"])
    eng.set_eps(eps)
    eng.distribution(z, xs, scale, mn, st2, B, fix=True)
    got2 = st["counts"].cpu().numpy()
    assert np.array_equal(got2, DR.update(F, lo2, hi2, K, got))
    assert np.array_equal(got2[0], (F < lo2).sum(0)) and np.array_equal(got2[K + 1], (F > hi2).sum(0))
    assert np.array_equal(st["lo"].cpu().numpy(), lo) and np.array_equal(st2["hi"].cpu().numpy(), hi2)          # the bounds are inputs


def test_distribution_checks_its_arguments():
    cfg, eng = engine("G0", "f32")
    z, xs, eps = latents(cfg, 2)
    scale, mn = (torch.from_numpy(a).cuda() for a in signed_scaler(cfg.num_node))
    T, N = cfg.num_time, cfg.num_node
    st = new_state(np.zeros((T, N)), np.ones((T, N)), 7)
    with pytest.raises(ValueError, match="state must be a dict"):
        eng.distribution(z, xs, scale, mn, {}, 0)
    with pytest.raises(ValueError, match="is not a tensor of the distribution state"):
        eng.distribution(z, xs, scale, mn, dict(st, limit=st["lo"]), 0)
    for k in ("lo", "hi"):
        with pytest.raises(ValueError, match="state needs all of"):
            eng.distribution(z, xs, scale, mn, {n: v for n, v in st.items() if n != k}, 0)
    for rows in (3, 67):
        with pytest.raises(ValueError, match=r"is outside \[2, 64\]"):
            eng.distribution(z, xs, scale, mn, dict(st, counts=torch.zeros((rows, T, N), dtype=torch.int32, device="cuda")), 0)
    for k, bad in (("lo", st["lo"][:-1]), ("hi", st["hi"].double()), ("lo", st["lo"].cpu()), ("hi", st["hi"].t()), ("counts", st["counts"].long()),
                   ("counts", st["counts"].float()), ("counts", st["counts"][:, :-1]), ("counts", st["counts"][0])):
        with pytest.raises(ValueError, match=rf"state\['{k}'\] must be a contiguous"):
            eng.distribution(z, xs, scale, mn, dict(st, **{k: bad}), 0)
    with pytest.raises(ValueError, match="scale must be"):
        eng.distribution(z, xs, scale[:-1], mn, st, 0)
    for cb in (-1, (1 << 24) - 1):
        with pytest.raises(ValueError, match="count_before"):
            eng.distribution(z, xs, scale, mn, st, cb)
    # the C entry point itself: SGV_ERR_ARG before anything is enqueued, so the forward of a decode stays readable
    eng.set_eps(eps)
    eng.decode(z, xs, fix=True)
    xs_t = torch.stack(xs).contiguous()
    ptr = {k: v.data_ptr() for k, v in st.items()}
    args = [z.data_ptr(), xs_t.data_ptr(), 2, 1, scale.data_ptr(), mn.data_ptr(), 0]

    def rejected(msg, so=True, bins=7, **kw):
        a, p = list(args), dict(ptr)
        for i, v in kw.items():
            if i in p:
                p[i] = v
            else:
                a[int(i[1:])] = v
        assert eng.lib.sgv_distribution(eng.h, *a, C.byref(E.DistributionState(bins=bins, **p)) if so else None) == -1
        assert msg in eng.lib.sgv_last_error().decode(), eng.lib.sgv_last_error().decode()

    rejected("null argument", so=False)
    for i in (0, 4, 5):          # z, scale, min
        rejected("null argument", **{f"a{i}": None})
    rejected("needs xs", a1=None)
    rejected("outside [0, 2^24]", a2=0)
    for k in ptr:
        rejected("lo, hi and counts are all required", **{k: None})
        rejected("misaligned pointer", **{k: ptr[k] + 4})
    for bins in (1, 65):
        rejected("is outside [2, 64]", bins=bins)
    rejected("outside [0, 2^24]", a6=-1)
    rejected("outside [0, 2^24]", a6=(1 << 24) - 1)
    assert eng.lib.sgv_distribution(None, *args, C.byref(E.DistributionState(bins=7, **ptr))) == -1
    eng.xhat()
    torch.cuda.synchronize()
    assert not st["counts"].any()


def test_no_forward_to_read_after_distribution_and_generate_is_unchanged():
    cfg, eng = engine("G0", "bf16")

    def run(z, xs, scale, mn, before):
        F = before.cpu().numpy()
        st = new_state(F.min(0), F.max(0), 32)
        eng.distribution(z, xs, scale, mn, st, 0)
        assert np.array_equal(st["counts"].cpu().numpy(), DR.update(F, F.min(0), F.max(0), 32))

    no_forward_after(eng, cfg, run, (eng.xhat, lambda: eng.activation("x_hat", (2, cfg.num_node, cfg.num_time)), lambda: eng.backward(1.0, 1.0)))


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_training_is_unaffected_by_distribution(dtype):
    cfg = make_cfg(G0)
    st = new_state(np.full((cfg.num_time, cfg.num_node), -1.0), np.full((cfg.num_time, cfg.num_node), 1.0), 64)
    training_unaffected(dtype, lambda eng, z, xs, scale, mn, i: eng.distribution(z, xs, scale, mn, st, 2 * i), False)
    assert int(st["counts"].sum()) == 4 * cfg.num_time * cfg.num_node


# ---- Surrogate.distribution ----
QS = (0.05, 0.5, 0.95, 1.0)


@pytest.mark.parametrize("mode", ["fix", "random"])
@pytest.mark.parametrize("kind,K", [("img", 32), ("mlp", 7)])
def test_distribution_between_the_ensemble_envelope_counts_what_predict_writes(kind, K, mode):
    dtype, seed = ("bf16", 3) if mode == "fix" else ("f32", 21)
    s, x, g = surrogate(kind, dtype, batch=8, seed=seed)         # one call of predict: its draws are the study's
    F = s.predict(x, mode=mode).cpu().numpy()
    P, T, N = F.shape
    s, x, _ = surrogate(kind, dtype, batch=4, seed=seed)         # a new Surrogate re-seeds the engine; 6 members as 4 + 2
    env = s.ensemble(x, want=("extrema",), mode=mode)
    res = s.distribution(x, env, bins=K, mode=mode)              # the second pass regenerates the members of the first
    assert isinstance(res, DistributionResult) and res.count == P and res.bins == K
    assert res.lo is env.min and res.hi is env.max               # used as they are, no copy
    assert res.counts.shape == (K + 2, T, N) and res.counts.dtype == torch.int32 and res.counts.is_contiguous()
    assert not res.under.any() and not res.over.any()            # the noise-by-member-index contract, in "random" too
    got = res.counts.cpu().numpy()
    assert np.array_equal(got.sum(0), np.full((T, N), P))
    lo, hi = F.min(0), F.max(0)
    assert np.array_equal(env.min.cpu().numpy(), lo) and np.array_equal(env.max.cpu().numpy(), hi)
    assert np.array_equal(got, DR.update(F, lo, hi, K))
    assert torch.equal(res.fractions(), res.counts[1:K + 1].float() / float(P))
    # percentile bands against the sorted fields
    bound = DR.bound(lo, hi, K)
    qs = res.quantile(QS)
    assert qs.shape == (len(QS), T, N) and qs.dtype == torch.float32
    for i, q in enumerate(QS):
        err = np.abs(qs[i].cpu().numpy().astype(np.float64) - DR.order_statistic(F, q).astype(np.float64))
        print(f"{kind} {mode} K={K} q={q}: worst err / bound {float((err / np.where(bound > 0, bound, 1)).max()):.7f}")
        assert (err <= bound).all(), q
        assert bool((qs[i] >= res.lo).all()) and bool((qs[i] <= res.hi).all())
    assert torch.equal(res.median(), qs[1]) and torch.equal(res.quantile(0.5), qs[1])
    if mode == "random":
        assert bool((env.max > env.min).all())


@pytest.mark.parametrize("mode", ["fix", "random"])
def test_batch_size_does_not_show_in_the_counts(mode):
    s, x, _ = surrogate("img", "f32", batch=3, seed=11)
    x7 = np.concatenate([x, x[:1]])                              # P = 7 at batch 3: 3 + 3 + 1
    a = s.distribution(x7, s.ensemble(x7, want=("extrema",), mode=mode), bins=16, mode=mode)
    assert a.count == 7 and not a.under.any() and not a.over.any()
    s, x, _ = surrogate("img", "f32", batch=7, seed=11)
    b = s.distribution(x7, s.ensemble(x7, want=("extrema",), mode=mode), bins=16, mode=mode)      # one batch of 7
    same_result(a, b)


def test_into_continues_and_equals_one_call_and_host_conditions_equal_device_conditions():
    s, x, g = surrogate("mlp", "f32", seed=11)
    T, N = 12, 520
    env = s.ensemble(x, want=("extrema",))
    lo, hi = env.min.cpu().numpy(), env.max.cpu().numpy()
    whole = s.distribution(x, (lo, hi), bins=8)                  # 6 conditions at batch 4: 4 + 2; host conditions, host bounds [T, N]
    assert whole.count == 6 and whole.counts.shape == (10, T, N) and not whole.under.any() and not whole.over.any()
    assert np.array_equal(whole.lo.cpu().numpy(), lo)
    s, x, _ = surrogate("mlp", "f32", seed=11)
    first = s.distribution(x[:3], (lo, hi), bins=8)              # a cut that is no batch boundary of the single call
    ptr = first.counts.data_ptr()
    second = s.distribution(torch.from_numpy(x[3:]).cuda(), (first.lo, first.hi), bins=8, into=first)      # device conditions, device bounds
    assert second.count == 6 and second.counts.data_ptr() == ptr and second.lo is first.lo                # the same tensors, updated in place
    same_result(whole, second)
    s, x, _ = surrogate("mlp", "f32", seed=11)
    same_result(whole, s.distribution(torch.from_numpy(x).cuda(), (torch.from_numpy(lo).cuda(), torch.from_numpy(hi).cuda()), bins=8))
    # scalar and per-node bounds are broadcast; what lies outside is counted
    s, x, _ = surrogate("mlp", "f32", seed=11)
    F = s.predict(x).cpu().numpy()          # batch 4: not the study's draws bit for bit, but the bounds below are far from any value
    mid = np.median(F.reshape(-1, N), axis=0).astype(np.float32)
    s, x, _ = surrogate("mlp", "f32", seed=11)
    half = s.distribution(x, (mid, np.full(N, 3.0e38, np.float32)), bins=2)
    assert not half.over.any() and 0 < int(half.under.sum()) < 6 * T * N
    s, x, _ = surrogate("mlp", "f32", seed=11)
    wide = s.distribution(x, (-3.0e38, 3.0e38), bins=2)
    assert not wide.under.any() and not wide.over.any() and int(wide.counts.sum()) == 6 * T * N
    # what does not fit
    with pytest.raises(ValueError, match="into holds 8 bins, this call asks for 16"):
        s.distribution(x, (lo, hi), bins=16, into=whole)
    with pytest.raises(ValueError, match=r"into was counted between other bounds \(hi differs\)"):
        s.distribution(x, (lo, hi + 1), into=whole, bins=8)
    with pytest.raises(ValueError, match=r"into was counted between other bounds \(lo differs\)"):
        s.distribution(x, (torch.from_numpy(lo - 1).cuda(), whole.hi), into=whole, bins=8)
    with pytest.raises(ValueError, match="into must be a DistributionResult, not EnsembleResult"):
        s.distribution(x, env, bins=8, into=env)
    for bins in (1, 65, 2.5):
        with pytest.raises(ValueError, match=r"is outside \[2, 64\]"):
            s.distribution(x, env, bins=bins)
    with pytest.raises(ValueError, match="does not hold the extrema"):
        s.distribution(x, s.ensemble(x[:1], want=("moments",)))
    with pytest.raises(ValueError, match=r"range: lo has shape \(12, 519\)"):
        s.distribution(x, (env.min[:, :-1], env.max))
    with pytest.raises(ValueError, match="dtype float32 is required"):
        s.distribution(x, (env.min.double(), env.max))
    with pytest.raises(ValueError, match="is not a CUDA tensor, but the other bound is one"):
        s.distribution(x, (lo, env.max))
    with pytest.raises(ValueError, match="range: hi < lo"):
        s.distribution(x, (1.0, 0.0))
    with pytest.raises(ValueError, match="mode must be"):
        s.distribution(x, env, mode="mean")
    empty = s.distribution(x[:0], (lo, hi), bins=8)
    assert empty.count == 0 and not empty.counts.any()
    with pytest.raises(ValueError, match="the distribution is empty"):
        empty.quantile(0.5)
    same_result(whole, surrogate("mlp", "f32", seed=11)[0].distribution(x, (empty.lo, empty.hi), bins=8, into=empty))
