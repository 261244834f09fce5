"""Surrogate linear functionals on the GPU: Engine.project (sgv_project) against float64 sums over what Engine.generate writes on the
same engine, latents and injected noise; what a call leaves behind in the engine; and Surrogate.project against float64 sums over
Surrogate.predict, against the probe histories of Surrogate.sweep and against region means, on the models of
tests/golden/predict_small.npz.

Against float64 the values are held to the a-priori bound of an fp32 summation in any order,
|q - q64| <= (N + 2) 2^-24 sum_n |W[r, n] F[n]| (tests/project_reference.py), F the stored field.  predict and project draw the
decoder's noise per call, so a comparison of the two makes one call of each on Surrogates with the same seed (the rule of
tests/test_sweep_gpu.py)."""
import os
import sys

import numpy as np
import pytest
import torch

import simulgen_vae_amd  # noqa: F401
from simulgen_vae_amd.predict import ProjectResult, region_weights
from tests.surrogate_common import MAXB, engine, latents, no_forward_after, signed_scaler, surrogate, training_unaffected

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import project_reference as PR  # noqa: E402

pytestmark = pytest.mark.gpu


def within_bound(q, F, W, what):
    ratio = PR.worst_ratio(q, F, W)
    print(f"  {what}: worst err / bound {ratio:.4f}")
    assert ratio <= 1.0, f"{what}: worst err / bound {ratio:.3f}"


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("B", [1, 3, MAXB])
@pytest.mark.parametrize("name", ["G0", "G1"])
def test_project_sums_what_generate_writes(name, B, dtype):
    cfg, eng = engine(name, dtype)
    T, N = cfg.num_time, cfg.num_node
    z, xs, eps = latents(cfg, B)
    scale, mn = (torch.from_numpy(a).cuda() for a in signed_scaler(N))
    eng.set_eps(eps)
    F = eng.generate(z, xs, scale, mn, fix=True).cpu().numpy()
    for R in (1, 3, 32):
        W = PR.mixed_weights(R, N)
        eng.set_eps(eps)
        q = eng.project(z, xs, scale, mn, torch.from_numpy(W).cuda(), fix=True)
        assert q.dtype == torch.float32 and q.shape == (B, T, R) and q.is_contiguous()
        within_bound(q.cpu().numpy(), F, W, f"{name} B {B} R {R} {dtype}")
    # into the rows of a larger tensor, and one-hot rows are the field itself
    W = np.zeros((2, N), np.float32)
    W[0, 0] = W[1, N - 1] = 1.0
    big = torch.full((B + 2, T, 2), float("nan"), device="cuda")
    eng.set_eps(eps)
    assert eng.project(z, xs, scale, mn, torch.from_numpy(W).cuda(), fix=True, out=big[1:B + 1]).data_ptr() == big[1:].data_ptr()
    got = big.cpu().numpy()
    assert np.isnan(got[0]).all() and np.isnan(got[B + 1]).all()
    assert np.array_equal(got[1:B + 1, :, 0], F[:, :, 0]) and np.array_equal(got[1:B + 1, :, 1], F[:, :, N - 1])


def test_project_checks_its_arguments():
    cfg, eng = engine("G0", "f32")
    z, xs, eps = latents(cfg, 2)
    scale, mn = (torch.from_numpy(a).cuda() for a in signed_scaler(cfg.num_node))
    T, N, R = cfg.num_time, cfg.num_node, 3
    w = torch.zeros((R, N), device="cuda")
    for bad in (w[0], w[:, :-1], w.double(), w.cpu(), torch.zeros((33, N), device="cuda"), torch.zeros((0, N), device="cuda"),
                torch.zeros((R, 2 * N), device="cuda")[:, ::2], w.cpu().numpy()):
        with pytest.raises(ValueError, match="weights must be a contiguous float32 CUDA tensor of shape"):
            eng.project(z, xs, scale, mn, bad)
    for bad in (torch.zeros((2, T, R + 1), device="cuda"), torch.zeros((1, T, R), device="cuda"), torch.zeros((2, T, R), device="cuda").double(),
                torch.zeros((2, T, R)), torch.zeros((2, R, T), device="cuda").transpose(1, 2)):
        with pytest.raises(ValueError, match="out must be a contiguous float32 CUDA tensor of shape"):
            eng.project(z, xs, scale, mn, w, out=bad)
    with pytest.raises(ValueError, match="scale must be"):
        eng.project(z, xs, scale[:-1], mn, w)
    # the C entry point itself: SGV_ERR_ARG before anything is enqueued, so the forward of a decode stays readable
    eng.set_eps(eps)
    eng.decode(z, xs, fix=True)
    xs_t = torch.stack(xs).contiguous()
    out = torch.full((2, T, R), 768.0, device="cuda")
    args = [z.data_ptr(), xs_t.data_ptr(), 2, 1, scale.data_ptr(), mn.data_ptr(), w.data_ptr(), R, out.data_ptr()]

    def rejected(msg, **kw):
        a = list(args)
        for i, v in kw.items():
            a[int(i[1:])] = v
        assert eng.lib.sgv_project(eng.h, *a) == -1
        assert msg in eng.lib.sgv_last_error().decode(), eng.lib.sgv_last_error().decode()

    for i in (0, 4, 5, 6, 8):          # z, scale, min, weights, out
        rejected("null argument", **{f"a{i}": None})
    rejected("needs xs", a1=None)
    rejected("batch 0 outside", a2=0)
    rejected(f"batch {MAXB + 1} outside", a2=MAXB + 1)
    rejected("n_func = 0 is outside [1, 32]", a7=0)
    rejected("n_func = 33 is outside [1, 32]", a7=33)
    rejected("misaligned pointer", a6=w.data_ptr() + 4)
    rejected("misaligned pointer", a8=out.data_ptr() + 2)
    assert eng.lib.sgv_project(None, *args) == -1
    eng.xhat()
    torch.cuda.synchronize()
    assert bool((out == 768.0).all())


def test_no_forward_to_read_after_project_and_generate_is_unchanged():
    cfg, eng = engine("G0", "bf16")
    W = torch.from_numpy(PR.mixed_weights(3, cfg.num_node)).cuda()

    def run(z, xs, scale, mn, before):
        q = eng.project(z, xs, scale, mn, W)
        within_bound(q.cpu().numpy(), before.cpu().numpy(), W.cpu().numpy(), "after decode")
    no_forward_after(eng, cfg, run, (eng.xhat, lambda: eng.backward(1.0, 1.0)))


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_training_is_unaffected_by_project(dtype):
    W = {}

    def run(eng, z, xs, scale, mn, i):
        if "w" not in W:
            W["w"] = torch.from_numpy(PR.mixed_weights(32, eng.cfg.num_node)).cuda()
        eng.project(z, xs, scale, mn, W["w"])
    training_unaffected(dtype, run, True)


# ---- Surrogate.project on the fixture's models: P = 6 conditions, T = 12, N = 520 ----
def labels(N):
    """five regions of unequal size and some nodes in none"""
    lab = np.random.default_rng(23).integers(-1, 5, N)
    lab[:7] = 4
    return lab


@pytest.mark.parametrize("mode", ["fix", "random"])
@pytest.mark.parametrize("kind,dtype", [("img", "f32"), ("mlp", "bf16")])
def test_surrogate_project_sums_what_predict_writes(kind, dtype, mode):
    s, x, _ = surrogate(kind, dtype, batch=8, seed=5)          # batch >= P: one call of the decoder each
    F = s.predict(x, mode=mode).cpu().numpy()
    P, T, N = F.shape
    W = PR.mixed_weights(32, N)
    s, x, _ = surrogate(kind, dtype, batch=8, seed=5)          # a new Surrogate re-seeds the engine: the same draws again
    res = s.project(x, W, mode=mode)
    assert isinstance(res, ProjectResult) and res.values.dtype == torch.float32 and res.values.shape == (P, T, 32) and res.values.is_contiguous()
    within_bound(res.values.cpu().numpy(), F, W, f"{kind} {dtype} {mode}")
    # region means against the mean of predict's columns
    lab = labels(N)
    M = region_weights(lab)
    s, x, _ = surrogate(kind, dtype, batch=8, seed=5)
    q = s.project(x, M, mode=mode).values.cpu().numpy()
    within_bound(q, F, M, f"{kind} {dtype} {mode} region means")
    for r in range(5):
        idx = np.flatnonzero(lab == r)
        mean64 = F[:, :, idx].astype(np.float64).mean(-1)
        # the weights 1 / n are rounded to fp32 once: 2^-24 relative each, on top of the bound of the sum
        slack = PR.bound(F, M[r:r + 1])[..., 0] + 2.0 ** -24 * np.abs(F[:, :, idx]).astype(np.float64).mean(-1)
        assert np.all(np.abs(q[:, :, r] - mean64) <= slack), r


def test_one_hot_functionals_are_the_probe_histories_of_sweep():
    nodes = [0, 5, 5, 517, 519]
    s, x, _ = surrogate("img", "f32", batch=8, seed=11)          # batch >= P: one call of the decoder each, the same draws
    probes = s.sweep(x, probes=nodes).probes.cpu().numpy()
    W = np.zeros((len(nodes), 520), np.float32)
    W[np.arange(len(nodes)), nodes] = 1.0
    s, x, _ = surrogate("img", "f32", batch=8, seed=11)
    got = s.project(x, W).values.cpu().numpy()
    assert got.shape == probes.shape and np.array_equal(got, probes)
    s, x, _ = surrogate("img", "f32", batch=8, seed=11)
    assert np.array_equal(s.project(x, W[3]).values.cpu().numpy()[:, :, 0], probes[:, :, 3])          # [N]: a single functional


@pytest.mark.parametrize("mode", ["fix", "random"])
def test_the_batch_size_does_not_show(mode):
    """Batch sizes 1, 3 and MAXB = 4 (4 + 2: a ragged last batch) give bitwise-equal values: the kernel gives a sample the same bits
    in any batch, and condition p takes row p of the noise streams one call over all conditions would draw from, whatever the
    batch (Engine.set_draw_row), so the draw position also ends where one call leaves it."""
    W = PR.mixed_weights(3, 520)
    runs, draws = [], []
    for batch in (1, 3, MAXB, 8):
        s, x, _ = surrogate("mlp", "f32", batch=batch, seed=7)
        runs.append(s.project(x, W, mode=mode).values)
        draws.append(s.eng.train_state()["draw"])
    assert all(r.shape == (6, 12, 3) for r in runs)
    for batch, other in zip((3, MAXB, 8), runs[1:]):
        ulp = (runs[0].view(torch.int32).long() - other.view(torch.int32).long()).abs()
        print(f"  {mode}: batch 1 against batch {batch}: {int((ulp > 0).sum())} of {ulp.numel()} values differ, by at most {int(ulp.max())} ulp")
    for other in runs[1:]:
        assert torch.equal(runs[0].view(torch.int32), other.view(torch.int32))
    assert len(set(draws)) == 1 and draws[0] > 0
    # and the one call is predict's: the same draws, the same field
    s, x, _ = surrogate("mlp", "f32", batch=8, seed=7)
    F = s.predict(x, mode=mode).cpu().numpy()
    assert s.eng.train_state()["draw"] == draws[0]
    within_bound(runs[0].cpu().numpy(), F, W, f"batch 1 against a one-call predict, {mode}")


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_draw_row_gives_a_later_batch_the_rows_of_one_call(dtype):
    """Engine.set_draw_row: samples 1 .. 2 generated alone, from row 1 of the draws of the call over all three, have the bits they
    have in that call; ensemble() counts its members itself and does not notice; the default is row 0"""
    cfg, eng = engine("G1", dtype)
    z, xs, _ = latents(cfg, 3)
    scale, mn = (torch.from_numpy(a).cuda() for a in signed_scaler(cfg.num_node))
    st = eng.train_state()
    try:
        whole = eng.generate(z, xs, scale, mn, fix=False).clone()
        after = eng.train_state()["draw"]
        eng.set_train_state(st["step"], st["seed"], st["draw"])
        eng.set_draw_row(1)
        part = eng.generate(z[1:], [v[1:].contiguous() for v in xs], scale, mn, fix=False).clone()
        assert eng.train_state()["draw"] == after
        assert torch.equal(part.view(torch.int32), whole[1:].view(torch.int32))
        state = [{k: torch.zeros((cfg.num_time, cfg.num_node), device="cuda") for k in ("mean", "m2")} for _ in range(2)]
        eng.ensemble(z, xs, scale, mn, state[0], 0, fix=False)
        eng.set_draw_row(0)
        eng.ensemble(z, xs, scale, mn, state[1], 0, fix=False)
        assert all(torch.equal(state[0][k].view(torch.int32), state[1][k].view(torch.int32)) for k in state[0])
        eng.set_train_state(st["step"], st["seed"], st["draw"])
        assert torch.equal(eng.generate(z, xs, scale, mn, fix=False).view(torch.int32), whole.view(torch.int32))
        with pytest.raises(Exception, match="first_row = -1 is negative"):
            eng.set_draw_row(-1)
    finally:
        eng.set_draw_row(0)
        eng.set_train_state(st["step"], st["seed"], st["draw"])


def test_host_and_device_weights_give_the_same_bits():
    W = PR.mixed_weights(3, 520)
    s, x, _ = surrogate("mlp", "f32", batch=MAXB, seed=7)
    host = s.project(x, W).values
    s, x, _ = surrogate("mlp", "f32", batch=MAXB, seed=7)
    dev = s.project(torch.from_numpy(x).cuda(), torch.from_numpy(W).cuda()).values
    assert torch.equal(dev.view(torch.int32), host.view(torch.int32))
    s, x, _ = surrogate("mlp", "f32", batch=MAXB, seed=7)
    odd = torch.zeros(3 * 520 + 1, device="cuda")[1:].view(3, 520)          # device weights at an odd offset
    odd.copy_(torch.from_numpy(W))
    assert torch.equal(s.project(x, odd).values.view(torch.int32), host.view(torch.int32))
    s, x, _ = surrogate("mlp", "f32", batch=MAXB, seed=7)
    assert torch.equal(s.project(x, W.astype(np.float64)).values.view(torch.int32), host.view(torch.int32))          # float64 host rows
    with pytest.raises(ValueError, match="weights: the last dimension is 519, expected N = 520"):
        s.project(x, W[:, :-1])
    with pytest.raises(ValueError, match="mode must be"):
        s.project(x, W, mode="mean")


def test_sampling_differs_from_the_mean_and_the_values_feed_regress():
    W = region_weights(labels(520))
    s, x, _ = surrogate("mlp", "f32", seed=21)
    fix = s.project(x, W, mode="fix")
    s, x, _ = surrogate("mlp", "f32", seed=21)
    rnd = s.project(x, W, mode="random")
    assert not torch.equal(fix.values, rnd.values)
    # a [P, R] slice of values is a covariate matrix of regress: the hand-off, not regress itself
    s, x, _ = surrogate("mlp", "f32", seed=21)
    reg = s.regress(x, covariates=fix.values[:, 4, :].cpu().numpy())
    assert reg.count == 6 and reg.comoment.shape == (5, 12, 520)


def test_peak_and_time_integral_of_the_values():
    s, x, _ = surrogate("img", "bf16", seed=2)
    res = s.project(x, PR.mixed_weights(3, 520))
    v = res.values.cpu().numpy()
    top, when = res.peak()
    assert np.array_equal(top.cpu().numpy(), v.max(axis=1)) and np.array_equal(when.cpu().numpy(), v.argmax(axis=1))
    trapezoid = getattr(np, "trapezoid", None) or np.trapz
    got = res.time_integral(0.5).cpu().numpy()
    want = trapezoid(v.astype(np.float64), dx=0.5, axis=1)
    assert got.dtype == np.float32 and got.shape == (6, 3)
    assert np.all(np.abs(got - want) <= 2.0 ** -23 * np.abs(want))          # float64 sums rounded to fp32 once; the order of the float64 additions is torch's
