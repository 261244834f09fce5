"""Sobol sensitivity indices on the GPU: Engine.sobol (sgv_sobol) against the numpy float32 emulation of the kernel's arithmetic
(tests/sobol_reference.py) run on what Engine.generate writes on the same engine, latents and injected noise; what a call leaves
behind in the engine; and Surrogate.sobol against the emulation on the fields of Surrogate.predict for the same member matrix, on
the models of tests/golden/predict_small.npz.

No tolerances but one: every sum is bit for bit the emulation's.  As for an ensemble, the decoder's noise of a member follows its
index in the study, so Surrogate.sobol gives the same bits at any batch size and for any cut into `into=` calls, and equals the
emulation on Surrogate.predict exactly when predict makes one call (batch >= n (d + 2)), which is how the comparison runs.  The one
tolerance, for a parameter whose columns are equal in A and B, is measured on predict's fields of the same members (see the test)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import simulgen_vae_amd  # noqa: F401
from simulgen_vae_amd import engine as E
from simulgen_vae_amd.predict import SobolResult, sobol_members
from tests.gpu_common import G0, make_cfg
from tests.surrogate_common import bits, engine, latents, no_forward_after, same_result, signed_scaler, state_as_numpy, surrogate, training_unaffected

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sobol_reference as SR  # noqa: E402

pytestmark = pytest.mark.gpu

U = 2.0 ** -24


def new_state(d, T, N, parts=("first_sq", "total_sq")):
    """the tensors of Engine.sobol's state, filled with what a call from empty must not read"""
    st = {k: torch.full((T, N), float("nan"), device="cuda") for k in ("mean", "m2")}
    st.update({k: torch.full((d, T, N), float("nan"), device="cuda") for k in parts})
    return st


def as_numpy(res):
    return state_as_numpy(res, SR.STATE)


def assert_same(got, want):
    for k in got:
        assert got[k].dtype == np.float32 and np.array_equal(bits(got[k]), bits(want[k])), k


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("d", [1, 2])
@pytest.mark.parametrize("name", ["G0", "G1"])
def test_sobol_matches_the_emulation_on_what_generate_writes(name, d, dtype):
    cfg, eng = engine(name, dtype)
    T, N, B = cfg.num_time, cfg.num_node, d + 2
    z, xs, eps = latents(cfg, B)
    scale, mn = (torch.from_numpy(a).cuda() for a in signed_scaler(N))
    eng.set_eps(eps)
    F = eng.generate(z, xs, scale, mn, fix=True).cpu().numpy()
    st = new_state(d, T, N)
    eng.set_eps(eps)
    res = eng.sobol(z, xs, scale, mn, st, d, 0, fix=True)
    assert res is st and sorted(res) == sorted(SR.STATE)
    want = SR.update(F, d)
    assert_same(as_numpy(st), want)
    # the same block again, as base sample 1: the state is read and continued
    eng.set_eps(eps)
    eng.sobol(z, xs, scale, mn, st, d, 1, fix=True)
    assert_same(as_numpy(st), SR.update(F, d, want, 1))
    # one part alone, into its own tensors: the bits of the full call
    for part in ("first_sq", "total_sq"):
        sub = new_state(d, T, N, parts=(part,))
        for bb in (0, 1):
            eng.set_eps(eps)
            eng.sobol(z, xs, scale, mn, sub, d, bb, fix=True)
        assert all(torch.equal(sub[k].view(torch.int32), st[k].view(torch.int32)) for k in sub)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_a_parameter_whose_latents_equal_those_of_a_gives_an_exact_zero(dtype):
    cfg, eng = engine("G1", dtype)
    d, B = 2, 4
    z, xs, eps = latents(cfg, B)
    z[2], z[3] = z[0], z[1]                              # AB_1 has A's latents, AB_2 has B's
    for x in xs:
        x[2], x[3] = x[0], x[1]
    scale, mn = (torch.from_numpy(a).cuda() for a in signed_scaler(cfg.num_node))
    st = new_state(d, cfg.num_time, cfg.num_node)
    eng.set_eps([torch.zeros_like(e) for e in eps])
    eng.sobol(z, xs, scale, mn, st, d, 0, fix=True)
    got = as_numpy(st)
    assert not got["total_sq"][0].any() and not got["first_sq"][1].any()
    assert got["first_sq"][0].any() and np.array_equal(bits(got["first_sq"][0]), bits(got["total_sq"][1]))


def test_sobol_checks_its_arguments():
    cfg, eng = engine("G0", "f32")
    d = 2
    z, xs, eps = latents(cfg, 4)
    scale, mn = (torch.from_numpy(a).cuda() for a in signed_scaler(cfg.num_node))
    T, N = cfg.num_time, cfg.num_node
    st = new_state(d, T, N)
    with pytest.raises(ValueError, match="state must be a dict"):
        eng.sobol(z, xs, scale, mn, {}, d, 0)
    with pytest.raises(ValueError, match="is not a tensor of the Sobol state"):
        eng.sobol(z, xs, scale, mn, dict(st, var=st["m2"]), d, 0)
    for drop in (("mean",), ("m2",), ("first_sq", "total_sq")):
        with pytest.raises(ValueError, match="state needs 'mean', 'm2' and at least one of"):
            eng.sobol(z, xs, scale, mn, {k: v for k, v in st.items() if k not in drop}, d, 0)
    for k, bad in (("mean", st["mean"][:-1]), ("m2", st["m2"].double()), ("first_sq", st["first_sq"].cpu()), ("total_sq", st["total_sq"][:1]),
                   ("first_sq", st["first_sq"].transpose(1, 2))):
        with pytest.raises(ValueError, match=rf"state\['{k}'\] must be a contiguous"):
            eng.sobol(z, xs, scale, mn, dict(st, **{k: bad}), d, 0)
    for bad_d in (0, 31):
        with pytest.raises(ValueError, match="n_params"):
            eng.sobol(z, xs, scale, mn, st, bad_d, 0)
    with pytest.raises(ValueError, match="not whole blocks of n_params \\+ 2 = 3"):
        eng.sobol(z, xs, scale, mn, new_state(1, T, N), 1, 0)
    for bb in (-1, 1 << 23):
        with pytest.raises(ValueError, match="blocks_before"):
            eng.sobol(z, xs, scale, mn, st, d, bb)
    # the C entry point itself: SGV_ERR_ARG before anything is enqueued, so the forward of a decode stays readable
    eng.set_eps(eps)
    eng.decode(z, xs, fix=True)
    xs_t = torch.stack(xs).contiguous()
    keep = {k: v.clone() for k, v in st.items()}
    ptr = {k: v.data_ptr() for k, v in st.items()}
    args = [z.data_ptr(), xs_t.data_ptr(), 4, 1, scale.data_ptr(), mn.data_ptr(), d, 0]

    def rejected(msg, so=True, **kw):
        a, p = list(args), dict(ptr)
        for i, v in kw.items():
            if i in p:
                p[i] = v
            else:
                a[int(i[1:])] = v
        assert eng.lib.sgv_sobol(eng.h, *a, C.byref(E.SobolState(**p)) if so else None) == -1
        assert msg in eng.lib.sgv_last_error().decode(), eng.lib.sgv_last_error().decode()

    rejected("null argument", so=False)
    for i in (0, 4, 5):          # z, scale, min
        rejected("null argument", **{f"a{i}": None})
    rejected("needs xs", a1=None)
    rejected("mean and m2 are required", mean=None)
    rejected("mean and m2 are required", m2=None)
    rejected("neither first_sq nor total_sq", first_sq=None, total_sq=None)
    for k in ptr:
        rejected("misaligned pointer", **{k: ptr[k] + 4})
    rejected("n_params = 0 is outside [1, 30]", a6=0)
    rejected("n_params = 31 is outside [1, 30]", a6=31)
    rejected("not a positive multiple of n_params + 2 = 3", a6=1)
    rejected("not a positive multiple", a2=0)
    rejected("outside [0, 2^24]", a7=-1)
    rejected("outside [0, 2^24]", a7=1 << 23)
    assert eng.lib.sgv_sobol(None, *args, C.byref(E.SobolState(**ptr))) == -1
    eng.xhat()
    torch.cuda.synchronize()
    assert all(torch.equal(st[k].view(torch.int32), keep[k].view(torch.int32)) for k in st)


def test_no_forward_to_read_after_sobol_and_generate_is_unchanged():
    cfg, eng = engine("G0", "bf16")
    st = new_state(1, cfg.num_time, cfg.num_node, parts=("total_sq",))
    no_forward_after(eng, cfg, lambda z, xs, scale, mn, before: eng.sobol(z, xs, scale, mn, st, 1, 0),
                     (eng.xhat, lambda: eng.activation("x_hat", (3, cfg.num_node, cfg.num_time)), lambda: eng.backward(1.0, 1.0)), B=3)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_training_is_unaffected_by_sobol(dtype):
    cfg = make_cfg(G0)
    st = new_state(2, cfg.num_time, cfg.num_node)
    training_unaffected(dtype, lambda eng, z, xs, scale, mn, i: eng.sobol(z, xs, scale, mn, st, 2, i), False, B=4)


# ---- Surrogate.sobol ----
GROUPS = [[0], [1, 2]]          # d = 2: blocks of 4 members


def design(x):
    """A, B [3, F] from the fixture's six conditions, as copies: the conditions are shared with the other test modules"""
    return np.array(x[:3], np.float32), np.array(x[3:], np.float32)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_sobol_equals_the_emulation_on_what_predict_writes(dtype):
    s, x, _ = surrogate("mlp", dtype, batch=12, seed=3)          # one call of predict: its draws are the study's (see above)
    A, B = design(x)
    assert A.shape[1] >= 3
    F = s.predict(sobol_members(A, B, GROUPS)).cpu().numpy()
    assert F.shape[0] == 12
    T, N = F.shape[1:]
    s, x, _ = surrogate("mlp", dtype, batch=4, seed=3)           # a new Surrogate re-seeds the engine; one block per batch
    res = s.sobol(A, B, groups=GROUPS)
    assert isinstance(res, SobolResult) and res.count == 3 and res.n_params == 2 and res.want() == ("first", "total")
    assert res.mean.shape == (T, N) and res.first_sq.shape == res.total_sq.shape == (2, T, N) and res.first_sq.is_contiguous()
    assert_same(as_numpy(res), SR.update(F, 2))
    assert torch.equal(res.var(), res.m2 / 6.0)
    assert torch.equal(res.first_order(), 1.0 - res.first_sq / (6.0 * (res.m2 / 6.0))) and torch.equal(res.total_order(), res.total_sq / (6.0 * (res.m2 / 6.0)))
    assert res.first_order().shape == (2, T, N)


def test_batch_size_into_and_host_or_device_inputs_do_not_show_in_the_result():
    s, x, _ = surrogate("mlp", "f32", batch=4, seed=11)
    A, B = design(x)
    whole = s.sobol(A, B, groups=GROUPS)                          # 1 + 1 + 1 blocks; host inputs (numpy)
    s, _, _ = surrogate("mlp", "f32", batch=11, seed=11)
    same_result(whole, s.sobol(A, B, groups=GROUPS))                   # 2 + 1 blocks: 11 // 4 = 2
    s, _, _ = surrogate("mlp", "f32", batch=12, seed=11)
    same_result(whole, s.sobol(torch.from_numpy(A).cuda(), torch.from_numpy(B).cuda(), groups=GROUPS))      # one batch; device inputs
    s, _, _ = surrogate("mlp", "f32", batch=8, seed=11)
    first = s.sobol(A[:1], B[:1], groups=GROUPS)
    ptrs = {k: v.data_ptr() for k, v in first.state().items()}
    second = s.sobol(torch.from_numpy(A[1:]).cuda(), B[1:], groups=GROUPS, into=first)
    assert second.count == 3 and {k: v.data_ptr() for k, v in second.state().items()} == ptrs          # the same tensors, updated in place
    same_result(whole, second)
    # one part alone gives the bits of the full call
    s, _, _ = surrogate("mlp", "f32", batch=8, seed=11)
    tot = s.sobol(A, B, groups=GROUPS, want=("total",))
    assert tot.want() == ("total",) and tot.first_sq is None
    assert all(torch.equal(getattr(tot, k).view(torch.int32), getattr(whole, k).view(torch.int32)) for k in ("mean", "m2", "total_sq"))
    with pytest.raises(ValueError, match="'first' was not asked for"):
        tot.first_order()
    with pytest.raises(ValueError, match="into holds the parts"):
        s.sobol(A, B, groups=GROUPS, into=tot)
    with pytest.raises(ValueError, match="into holds 2 parameters, this call has 1"):
        s.sobol(A, B, groups=[[0]], into=whole)
    with pytest.raises(ValueError, match="into must be a SobolResult"):
        s.sobol(A, B, groups=GROUPS, into=whole.state())
    with pytest.raises(ValueError, match="want must name"):
        s.sobol(A, B, groups=GROUPS, want=("second",))
    with pytest.raises(ValueError, match="one shape"):
        s.sobol(A, B[:2], groups=GROUPS)
    with pytest.raises(ValueError, match=r"groups\[1\]\[0\] = 99 is outside"):
        s.sobol(A, B, groups=[[0], [99]])
    empty = s.sobol(A[:0], B[:0], groups=GROUPS)
    assert empty.count == 0 and not empty.total_sq.any()
    same_result(whole, surrogate("mlp", "f32", batch=8, seed=11)[0].sobol(A, B, groups=GROUPS, into=empty))


def test_a_block_larger_than_the_batch_is_refused():
    s, x, _ = surrogate("mlp", "f32", batch=3, seed=11)
    A, B = design(x)
    with pytest.raises(ValueError, match=r"d \+ 2 = 4 members does not fit a batch of 3"):
        s.sobol(A, B, groups=GROUPS)
    assert s.sobol(A, B, groups=[[0, 1, 2]]).n_params == 1          # d + 2 = 3 does


def test_a_group_of_columns_equal_in_a_and_b_has_a_negligible_total_index():
    """Parameter 1's columns are equal in A and B, so AB_1 == A as conditions and the two members differ by the decoder's "fix"
    noise alone (1e-10 of the latent noise, drawn per member): not bit-zero, numerically negligible.  The tolerance is measured on
    Surrogate.predict's fields of the same members, in float64: st64 = sum_j (F_A - F_AB1)^2 / M2 there.  The study's index is that
    ratio in fp32: numerator within gamma_(n+2) (sumsq_bound), M2 within welford_bound's relative error 2 n u kappa, and four more
    roundings in total_order() (two divisions and a product by 2 n in var, one division), so
    ST <= st64 (1 + gamma_(n+2) + 4 u) / (1 - 2 n u kappa), elementwise.  The index of the parameter that does vary is printed beside it."""
    s, x, _ = surrogate("mlp", "f32", batch=12, seed=5)
    A, B = design(x)
    B[:, 0] = A[:, 0]
    n = 3
    F = s.predict(sobol_members(A, B, GROUPS)).cpu().numpy().astype(np.float64).reshape(n, 4, *(s.T, s.N))
    ab = F[:, :2].reshape(2 * n, s.T, s.N)
    mean, m2 = ab.mean(0), np.square(ab - ab.mean(0)).sum(0)
    st64 = np.square(F[:, 0] - F[:, 2]).sum(0) / m2
    kappa = np.sqrt(1.0 + 2 * n * np.square(mean) / m2)
    tol = st64 * (1 + SR.sumsq_bound(n, 1.0) + 4 * U) / (1 - 2 * n * U * kappa)
    s, _, _ = surrogate("mlp", "f32", batch=4, seed=5)
    res = s.sobol(A, B, groups=GROUPS)
    ST = res.total_order().cpu().numpy().astype(np.float64)
    print(f"total index of the parameter that does not vary: max {ST[0].max():.3e} (float64 on predict's fields {st64.max():.3e}); of the other: "
          f"median {np.median(ST[1]):.3e}")
    assert (m2 > 0).all() and (2 * n * U * kappa < 0.5).all()
    assert (ST[0] <= tol).all()
