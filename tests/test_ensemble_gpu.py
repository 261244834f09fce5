"""Surrogate ensemble statistics on the GPU: Engine.ensemble (sgv_ensemble) against numpy reductions over axis 0 of what
Engine.generate writes on the same engine, latents and injected noise, and against the numpy float32 emulation of the kernel's
arithmetic (tests/ensemble_reference.py) run on those fields; what a call leaves behind in the engine; and Surrogate.ensemble
against reductions of Surrogate.predict on the models of tests/golden/predict_small.npz.

No tolerances: max / min, the member indices (ties to the earliest member, as np.argmax), the counts above the limit, and mean /
M2 against the emulation are all bit for bit.  The limit is the per-node median of the fields, so counts are neither 0 nor P.

Noise.  The decoder adds noise to its latents in both modes (mode "fix": times 1e-10, which still shows in the last bits of the
field).  predict / sweep / score draw it per call, so their fields depend on where batch boundaries fall (measured on an MI355X,
the fp32 image model, P = 7: batch 3 against batch 7 differs in 44 % of the elements, members 3 to 6 by up to 22605 units in the
last place, while the engine itself is bitwise the same for 4 against 3 + 1 members when the noise is injected).  An ensemble
member's noise follows its index instead: the rows count_before + b of the streams the first call after seeding draws from.  So
Surrogate.ensemble gives the same bits at any batch size and for any cut into `into=` calls, and equals the reductions of
Surrogate.predict exactly when predict makes one call, batch >= P, which is how the comparison below runs (P = 6, batch 8)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import simulgen_vae_amd  # noqa: F401
from simulgen_vae_amd import engine as E
from simulgen_vae_amd.predict import EnsembleResult
from tests.gpu_common import G0, make_cfg
from tests.surrogate_common import (MAXB, bits, engine, latents, no_forward_after, same_result, signed_scaler, state_as_numpy, surrogate,
                                    training_unaffected)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ensemble_reference as ER  # noqa: E402

pytestmark = pytest.mark.gpu

INT = ("arg_max", "arg_min", "exceed")


def new_state(T, N, limit=None, groups=("moments", "extrema", "exceed")):
    """the tensors of Engine.ensemble's state, filled with what a call from empty must not read"""
    st = {}
    for g in groups:
        for k in E.ENSEMBLE_GROUPS[g]:
            if k == "limit":
                st[k] = torch.from_numpy(np.ascontiguousarray(limit, np.float32)).cuda()
            else:
                st[k] = torch.full((T, N), -5, dtype=torch.int32, device="cuda") if k in INT else torch.full((T, N), float("nan"), device="cuda")
    return st


def as_numpy(res):
    """an EnsembleResult, or Engine.ensemble's dict, as numpy arrays under the emulation's names"""
    return state_as_numpy(res, ER.STATE)


def assert_reduces(got, F, limit=None, want=None):
    """got (as_numpy) is the reduction over axis 0 of F [P, T, N] fp32: all bit for bit"""
    assert F.dtype == np.float32 and np.isfinite(F).all()
    if "max" in got:
        assert got["max"].dtype == np.float32 and np.array_equal(bits(got["max"]), bits(F.max(0))) and np.array_equal(bits(got["min"]), bits(F.min(0)))
        assert got["arg_max"].dtype == np.int32 and np.array_equal(got["arg_max"], F.argmax(0)) and np.array_equal(got["arg_min"], F.argmin(0))
    if "exceed" in got:
        assert got["exceed"].dtype == np.int32 and np.array_equal(got["exceed"], (F > limit).sum(0))
    if "mean" in got:
        want = ER.update(F) if want is None else want
        assert np.array_equal(bits(got["mean"]), bits(want["mean"])), "mean"
        assert np.array_equal(bits(got["m2"]), bits(want["m2"])), "m2"


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("B", [1, 3, MAXB])
@pytest.mark.parametrize("name", ["G0", "G1"])
def test_ensemble_reduces_what_generate_writes(name, B, dtype):
    cfg, eng = engine(name, dtype)
    T, N = cfg.num_time, cfg.num_node
    z, xs, eps = latents(cfg, B)
    scale, mn = (torch.from_numpy(a).cuda() for a in signed_scaler(N))
    eng.set_eps(eps)
    F = eng.generate(z, xs, scale, mn, fix=True).cpu().numpy()
    limit = np.median(F.reshape(B * T, N), axis=0).astype(np.float32)
    st = new_state(T, N, limit)
    eng.set_eps(eps)
    res = eng.ensemble(z, xs, scale, mn, st, 0, fix=True)
    assert res is st and sorted(res) == sorted(ER.STATE + ("limit",))
    assert_reduces(as_numpy(res), F, limit)
    assert np.array_equal(res["limit"].cpu().numpy(), limit)
    # the same members again, as members B .. 2B - 1: the state is read and continued
    eng.set_eps(eps)
    eng.ensemble(z, xs, scale, mn, st, B, fix=True)
    F2 = np.concatenate([F, F])
    assert_reduces(as_numpy(st), F2, limit)
    assert as_numpy(st)["arg_max"].max() < B          # every tie stays with the first round
    # one group alone, into its own tensors: the bits of the full call, and nothing else is asked of the caller
    for g in E.ENSEMBLE_GROUPS:
        sub = new_state(T, N, limit, groups=(g,))
        for cb in (0, B):
            eng.set_eps(eps)
            eng.ensemble(z, xs, scale, mn, sub, cb, fix=True)
        assert all(torch.equal(sub[k].view(torch.int32), st[k].view(torch.int32)) for k in sub)


def test_ensemble_checks_its_arguments():
    cfg, eng = engine("G0", "f32")
    z, xs, eps = latents(cfg, 2)
    scale, mn = (torch.from_numpy(a).cuda() for a in signed_scaler(cfg.num_node))
    T, N = cfg.num_time, cfg.num_node
    st = new_state(T, N, np.zeros(N, np.float32))
    with pytest.raises(ValueError, match="state must be a dict"):
        eng.ensemble(z, xs, scale, mn, {}, 0)
    with pytest.raises(ValueError, match="is not a tensor of the ensemble state"):
        eng.ensemble(z, xs, scale, mn, dict(st, var=st["m2"]), 0)
    for k in st:
        with pytest.raises(ValueError, match="needs all of"):
            eng.ensemble(z, xs, scale, mn, {n: v for n, v in st.items() if n != k}, 0)
    for k, bad in (("mean", st["mean"][:-1]), ("m2", st["m2"].double()), ("max", st["max"].cpu()), ("min", st["min"].t()), ("arg_max", st["mean"]),
                   ("exceed", st["exceed"].long()), ("limit", st["limit"][:-1]), ("limit", st["mean"])):
        with pytest.raises(ValueError, match=rf"state\['{k}'\] must be a contiguous"):
            eng.ensemble(z, xs, scale, mn, dict(st, **{k: bad}), 0)
    with pytest.raises(ValueError, match="scale must be"):
        eng.ensemble(z, xs, scale[:-1], mn, st, 0)
    with pytest.raises(ValueError, match="xs of shape"):
        eng.ensemble(z, xs[:-1], scale, mn, st, 0)
    for cb in (-1, (1 << 24) - 1):
        with pytest.raises(ValueError, match="count_before"):
            eng.ensemble(z, xs, scale, mn, st, cb)
    # the C entry point itself: SGV_ERR_ARG before anything is enqueued, so the forward of a decode stays readable
    eng.set_eps(eps)
    eng.decode(z, xs, fix=True)
    xs_t = torch.stack(xs).contiguous()
    keep = {k: v.clone() for k, v in st.items()}
    ptr = {k: v.data_ptr() for k, v in st.items()}
    args = [z.data_ptr(), xs_t.data_ptr(), 2, 1, scale.data_ptr(), mn.data_ptr(), 0]

    def rejected(msg, so=True, **kw):
        a = list(args)
        p = dict(ptr)
        for i, v in kw.items():
            if i in p:
                p[i] = v
            else:
                a[int(i[1:])] = v
        assert eng.lib.sgv_ensemble(eng.h, *a, C.byref(E.EnsembleState(**p)) if so else None) == -1
        assert msg in eng.lib.sgv_last_error().decode(), eng.lib.sgv_last_error().decode()

    rejected("null argument", so=False)
    for i in (0, 4, 5):          # z, scale, min
        rejected("null argument", **{f"a{i}": None})
    rejected("needs xs", a1=None)
    rejected("outside [0, 2^24]", a2=0)
    rejected("no group of the state", **{k: None for k in ptr})
    for k in ptr:
        rejected("half a group", **{k: None})
        rejected("misaligned pointer", **{k: ptr[k] + (2 if k == "limit" else 4)})
    rejected("outside [0, 2^24]", a6=-1)
    rejected("outside [0, 2^24]", a6=(1 << 24) - 1)
    assert eng.lib.sgv_ensemble(None, *args, C.byref(E.EnsembleState(**ptr))) == -1
    eng.xhat()
    torch.cuda.synchronize()
    assert all(torch.equal(st[k].view(torch.int32), keep[k].view(torch.int32)) for k in st)
    # the limit needs 4-byte alignment only
    lim = torch.zeros(N + 4, device="cuda")
    eng.set_eps(eps)
    assert eng.lib.sgv_ensemble(eng.h, *args, C.byref(E.EnsembleState(**dict(ptr, limit=lim.data_ptr() + 4)))) == 0
    torch.cuda.synchronize()


def test_no_forward_to_read_after_ensemble_and_generate_is_unchanged():
    cfg, eng = engine("G0", "bf16")
    st = new_state(cfg.num_time, cfg.num_node, groups=("extrema",))
    no_forward_after(eng, cfg, lambda z, xs, scale, mn, before: eng.ensemble(z, xs, scale, mn, st, 0),
                     (eng.xhat, lambda: eng.activation("x_hat", (2, cfg.num_node, cfg.num_time)), lambda: eng.backward(1.0, 1.0)))


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_training_is_unaffected_by_ensemble(dtype):
    cfg = make_cfg(G0)
    st = new_state(cfg.num_time, cfg.num_node, np.zeros(cfg.num_node, np.float32))
    training_unaffected(dtype, lambda eng, z, xs, scale, mn, i: eng.ensemble(z, xs, scale, mn, st, 2 * i), False)


# ---- Surrogate.ensemble ----
@pytest.mark.parametrize("mode", ["fix", "random"])
@pytest.mark.parametrize("kind", ["img", "mlp"])
def test_ensemble_reduces_what_predict_writes(kind, mode):
    dtype, seed = ("bf16", 3) if mode == "fix" else ("f32", 21)
    s, x, g = surrogate(kind, dtype, batch=8, seed=seed)         # one call of predict: its draws are the ensemble's (see above)
    F = s.predict(x, mode=mode).cpu().numpy()
    P, T, N = F.shape
    limit = np.median(F.reshape(P * T, N), axis=0).astype(np.float32)
    s, x, _ = surrogate(kind, dtype, batch=4, seed=seed)         # a new Surrogate re-seeds the engine; 6 members as 4 + 2
    res = s.ensemble(x, limit=limit, mode=mode)
    assert isinstance(res, EnsembleResult) and res.count == P and res.groups() == ("moments", "extrema", "exceed")
    assert all(getattr(res, k).shape == (T, N) and getattr(res, k).is_contiguous() for k in ER.STATE)
    got = as_numpy(res)
    assert_reduces(got, F, limit)
    assert np.array_equal(res.limit.cpu().numpy(), limit)
    assert torch.equal(res.var(), res.m2 / float(P)) and torch.equal(res.std(ddof=1), (res.m2 / float(P - 1)).sqrt())
    assert torch.equal(res.exceed_fraction(), res.exceed.float() / float(P))
    if mode == "random":
        s, x, _ = surrogate(kind, dtype, seed=seed)
        assert not torch.equal(s.ensemble(x, want=("extrema",), mode="fix").max, res.max)


@pytest.mark.parametrize("mode", ["fix", "random"])
def test_batch_size_does_not_show_in_the_result(mode):
    s, x, _ = surrogate("img", "f32", batch=3, seed=11)
    x7 = np.concatenate([x, x[:1]])                              # P = 7 at batch 3: 3 + 3 + 1
    a = s.ensemble(x7, limit=0.0, mode=mode)
    assert a.count == 7 and a.arg_max.max() <= 6
    s, x, _ = surrogate("img", "f32", batch=7, seed=11)
    b = s.ensemble(x7, limit=0.0, mode=mode)                     # one batch of 7
    same_result(a, b)
    if mode == "random":                                         # members 0 and 6 share their condition and differ by their draws
        assert int(a.arg_max.max()) == 6 and bool((a.m2 > 0).all())


def test_into_continues_and_equals_one_call_and_host_conditions_equal_device_conditions():
    s, x, g = surrogate("mlp", "f32", seed=11)
    limit = 0.5 / np.asarray(g["data_scale"], np.float64)
    whole = s.ensemble(x, limit=limit)                           # 6 conditions at batch 4: 4 + 2; host conditions (numpy)
    assert whole.count == 6 and whole.mean.shape == (12, 520)
    s, x, _ = surrogate("mlp", "f32", seed=11)
    first = s.ensemble(x[:3], limit=limit)                       # a cut that is no batch boundary of the single call
    ptrs = {k: v.data_ptr() for k, v in first.state().items()}
    second = s.ensemble(torch.from_numpy(x[3:]).cuda(), limit=limit, into=first)      # device conditions
    assert second.count == 6 and {k: v.data_ptr() for k, v in second.state().items()} == ptrs          # the same tensors, updated in place
    same_result(whole, second)
    s, x, _ = surrogate("mlp", "f32", seed=11)
    same_result(whole, s.ensemble(torch.from_numpy(x).cuda(), limit=limit))
    # a subset of the groups gives the bits of the full call
    s, x, _ = surrogate("mlp", "f32", seed=11)
    ext = s.ensemble(x, want=("extrema",))
    assert ext.groups() == ("extrema",) and ext.mean is None and ext.exceed is None and ext.limit is None
    assert all(torch.equal(getattr(ext, k).view(torch.int32), getattr(whole, k).view(torch.int32)) for k in ("max", "min", "arg_max", "arg_min"))
    with pytest.raises(ValueError, match="want names 'exceed' but no limit is given"):
        s.ensemble(x, want=("exceed",))
    with pytest.raises(ValueError, match="want must name"):
        s.ensemble(x, want=("node",))
    with pytest.raises(ValueError, match="limit: 3 entries, expected N = 520"):
        s.ensemble(x, limit=[1.0, 2.0, 3.0])
    with pytest.raises(ValueError, match="into holds the groups"):
        s.ensemble(x, into=whole)                                # whole has a limit, this call none
    with pytest.raises(ValueError, match="into holds the groups"):
        s.ensemble(x, limit=limit, into=ext)
    with pytest.raises(ValueError, match="another limit"):
        s.ensemble(x, limit=2 * limit, into=whole)
    with pytest.raises(ValueError, match="into must be an EnsembleResult"):
        s.ensemble(x, into=whole.state())
    with pytest.raises(ValueError, match="mode must be"):
        s.ensemble(x, mode="mean")
    empty = s.ensemble(x[:0], limit=limit)
    assert empty.count == 0 and not empty.exceed.any() and bool(torch.isinf(empty.max).all())
    same_result(whole, surrogate("mlp", "f32", seed=11)[0].ensemble(x, limit=limit, into=empty))
