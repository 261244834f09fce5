"""Surrogate temporal functionals on the GPU: Engine.temporal (sgv_temporal) against float64 sums over what Engine.generate writes on
the same engine, latents and injected noise; what a call leaves behind in the engine; and Surrogate.temporal against float64 sums over
Surrogate.predict, against Surrogate.project (the two contractions commute) and against numpy's FFT, on the models of
tests/golden/predict_small.npz.

Against float64 the values are held to the a-priori bound of an fp32 summation in any order,
|q - q64| <= (T + 2) 2^-24 sum_t |W[r, t] F[t, n]| (tests/temporal_reference.py), F the stored field.  predict, project and temporal draw
the decoder's noise per call, so a comparison of two of them makes one call of each on Surrogates with the same seed (the rule of
tests/test_sweep_gpu.py)."""
import os
import sys

import numpy as np
import pytest
import torch

import simulgen_vae_amd  # noqa: F401
from simulgen_vae_amd.predict import TemporalResult, fourier_rows, window_rows
from tests.surrogate_common import MAXB, engine, latents, no_forward_after, signed_scaler, surrogate, training_unaffected

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import project_reference as PR  # noqa: E402
import temporal_reference as TR  # noqa: E402

pytestmark = pytest.mark.gpu
U = 2.0 ** -24


def within_bound(q, F, W, what):
    ratio = TR.worst_ratio(q, F, W)
    print(f"  {what}: worst err / bound {ratio:.4f}")
    assert ratio <= 1.0, f"{what}: worst err / bound {ratio:.3f}"


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("B", [1, 3, MAXB])
@pytest.mark.parametrize("name", ["G0", "G1"])
def test_temporal_sums_what_generate_writes(name, B, dtype):
    cfg, eng = engine(name, dtype)
    T, N = cfg.num_time, cfg.num_node
    z, xs, eps = latents(cfg, B)
    scale, mn = (torch.from_numpy(a).cuda() for a in signed_scaler(N))
    eng.set_eps(eps)
    F = eng.generate(z, xs, scale, mn, fix=True).cpu().numpy()
    for R in (1, 3, 32):
        W = TR.mixed_weights(R, T)
        eng.set_eps(eps)
        q = eng.temporal(z, xs, scale, mn, torch.from_numpy(W).cuda(), fix=True)
        assert q.dtype == torch.float32 and q.shape == (B, R, N) and q.is_contiguous()
        within_bound(q.cpu().numpy(), F, W, f"{name} B {B} R {R} {dtype}")
    # into the rows of a larger tensor, and one-hot rows are the field itself
    W = np.zeros((2, T), np.float32)
    W[0, 0] = W[1, T - 1] = 1.0
    big = torch.full((B + 2, 2, N), float("nan"), device="cuda")
    eng.set_eps(eps)
    assert eng.temporal(z, xs, scale, mn, torch.from_numpy(W).cuda(), fix=True, out=big[1:B + 1]).data_ptr() == big[1:].data_ptr()
    got = big.cpu().numpy()
    assert np.isnan(got[0]).all() and np.isnan(got[B + 1]).all()
    assert np.array_equal(got[1:B + 1, 0], F[:, 0]) and np.array_equal(got[1:B + 1, 1], F[:, T - 1])


def test_temporal_checks_its_arguments():
    cfg, eng = engine("G0", "f32")
    z, xs, eps = latents(cfg, 2)
    scale, mn = (torch.from_numpy(a).cuda() for a in signed_scaler(cfg.num_node))
    T, N, R = cfg.num_time, cfg.num_node, 3
    w = torch.zeros((R, T), device="cuda")
    for bad in (w[0], w[:, :-1], w.double(), w.cpu(), torch.zeros((33, T), device="cuda"), torch.zeros((0, T), device="cuda"),
                torch.zeros((R, 2 * T), device="cuda")[:, ::2], w.cpu().numpy()):
        with pytest.raises(ValueError, match="weights must be a contiguous float32 CUDA tensor of shape"):
            eng.temporal(z, xs, scale, mn, bad)
    for bad in (torch.zeros((2, R + 1, N), device="cuda"), torch.zeros((1, R, N), device="cuda"), torch.zeros((2, R, N), device="cuda").double(),
                torch.zeros((2, R, N)), torch.zeros((2, N, R), device="cuda").transpose(1, 2)):
        with pytest.raises(ValueError, match="out must be a contiguous float32 CUDA tensor of shape"):
            eng.temporal(z, xs, scale, mn, w, out=bad)
    with pytest.raises(ValueError, match="scale must be"):
        eng.temporal(z, xs, scale[:-1], mn, w)
    # the C entry point itself: SGV_ERR_ARG before anything is enqueued, so the forward of a decode stays readable
    eng.set_eps(eps)
    eng.decode(z, xs, fix=True)
    xs_t = torch.stack(xs).contiguous()
    out = torch.full((2, R, N), 768.0, device="cuda")
    args = [z.data_ptr(), xs_t.data_ptr(), 2, 1, scale.data_ptr(), mn.data_ptr(), w.data_ptr(), R, out.data_ptr()]

    def rejected(msg, **kw):
        a = list(args)
        for i, v in kw.items():
            a[int(i[1:])] = v
        assert eng.lib.sgv_temporal(eng.h, *a) == -1
        assert msg in eng.lib.sgv_last_error().decode(), eng.lib.sgv_last_error().decode()

    for i in (0, 4, 5, 6, 8):          # z, scale, min, weights, out
        rejected("null argument", **{f"a{i}": None})
    rejected("needs xs", a1=None)
    rejected("batch 0 outside", a2=0)
    rejected(f"batch {MAXB + 1} outside", a2=MAXB + 1)
    rejected("n_func = 0 is outside [1, 32]", a7=0)
    rejected("n_func = 33 is outside [1, 32]", a7=33)
    rejected("misaligned pointer", a6=w.data_ptr() + 2)
    rejected("misaligned pointer", a8=out.data_ptr() + 4)
    rejected("misaligned pointer", a8=out.data_ptr() + 8)
    assert eng.lib.sgv_temporal(None, *args) == -1
    eng.xhat()
    torch.cuda.synchronize()
    assert bool((out == 768.0).all())


def test_no_forward_to_read_after_temporal_and_generate_is_unchanged():
    cfg, eng = engine("G0", "bf16")
    W = torch.from_numpy(TR.mixed_weights(3, cfg.num_time)).cuda()

    def run(z, xs, scale, mn, before):
        q = eng.temporal(z, xs, scale, mn, W)
        within_bound(q.cpu().numpy(), before.cpu().numpy(), W.cpu().numpy(), "after decode")
    no_forward_after(eng, cfg, run, (eng.xhat, lambda: eng.backward(1.0, 1.0)))


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_training_is_unaffected_by_temporal(dtype):
    W = {}

    def run(eng, z, xs, scale, mn, i):
        if "w" not in W:
            W["w"] = torch.from_numpy(TR.mixed_weights(32, eng.cfg.num_time)).cuda()
        eng.temporal(z, xs, scale, mn, W["w"])
    training_unaffected(dtype, run, True)


# ---- Surrogate.temporal on the fixture's models: P = 6 conditions, T = 12, N = 520 ----
@pytest.mark.parametrize("mode", ["fix", "random"])
@pytest.mark.parametrize("kind,dtype", [("img", "f32"), ("mlp", "bf16")])
def test_surrogate_temporal_sums_what_predict_writes(kind, dtype, mode):
    s, x, _ = surrogate(kind, dtype, batch=8, seed=5)          # batch >= P: one call of the decoder each
    F = s.predict(x, mode=mode).cpu().numpy()
    P, T, N = F.shape
    W = TR.mixed_weights(32, T)
    s, x, _ = surrogate(kind, dtype, batch=8, seed=5)          # a new Surrogate re-seeds the engine: the same draws again
    res = s.temporal(x, W, mode=mode)
    assert isinstance(res, TemporalResult) and res.values.dtype == torch.float32 and res.values.shape == (P, 32, N) and res.values.is_contiguous()
    within_bound(res.values.cpu().numpy(), F, W, f"{kind} {dtype} {mode}")
    # one-hot rows are predict's time steps, bit for bit; a 1 / T row and window means against the float64 means of predict
    M = np.concatenate([np.eye(T, dtype=np.float32)[[0, 5, T - 1]], window_rows(T, [0, T]), window_rows(T, [0, 3, 4, T])])
    s, x, _ = surrogate(kind, dtype, batch=8, seed=5)
    q = s.temporal(x, M, mode=mode).values.cpu().numpy()
    for k, t in enumerate((0, 5, T - 1)):
        assert np.array_equal(q[:, k] + 0.0, F[:, t] + 0.0) and np.array_equal((q[:, k] + 0.0).view(np.int32), (F[:, t] + 0.0).view(np.int32)), t
    within_bound(q, F, M, f"{kind} {dtype} {mode} window means")
    for r, (lo, hi) in zip(range(3, 7), ((0, T), (0, 3), (3, 4), (4, T))):
        mean64 = F[:, lo:hi].astype(np.float64).mean(1)
        # the weights 1 / n are rounded to fp32 once: 2^-24 relative each, on top of the bound of the sum
        slack = TR.bound(F, M[r:r + 1])[:, 0] + U * np.abs(F[:, lo:hi]).astype(np.float64).mean(1)
        assert np.all(np.abs(q[:, r] - mean64) <= slack), r
    assert np.array_equal(q[:, 5].view(np.int32), ((F[:, 3] + 0.0)).view(np.int32))          # a window of one step: weight 1


@pytest.mark.parametrize("mode", ["fix", "random"])
def test_the_batch_size_does_not_show(mode):
    """Batch sizes 1, 3, MAXB = 4 (4 + 2: a ragged last batch) and 8 give bitwise-equal values: the kernel gives a sample the same
    bits in any batch, and condition p takes row p of the noise streams one call over all conditions would draw from, whatever the
    batch (Engine.set_draw_row), so the draw position also ends where one call leaves it."""
    W = TR.mixed_weights(3, 12)
    runs, draws = [], []
    for batch in (1, 3, MAXB, 8):
        s, x, _ = surrogate("mlp", "f32", batch=batch, seed=7)
        runs.append(s.temporal(x, W, mode=mode).values)
        draws.append(s.eng.train_state()["draw"])
    assert all(r.shape == (6, 3, 520) for r in runs)
    for other in runs[1:]:
        assert torch.equal(runs[0].view(torch.int32), other.view(torch.int32))
    assert len(set(draws)) == 1 and draws[0] > 0
    # and the one call is predict's: the same draws, the same field
    s, x, _ = surrogate("mlp", "f32", batch=8, seed=7)
    F = s.predict(x, mode=mode).cpu().numpy()
    assert s.eng.train_state()["draw"] == draws[0]
    within_bound(runs[0].cpu().numpy(), F, W, f"batch 1 against a one-call predict, {mode}")


def test_host_and_device_weights_give_the_same_bits():
    W = TR.mixed_weights(3, 12)
    s, x, _ = surrogate("mlp", "f32", batch=MAXB, seed=7)
    host = s.temporal(x, W).values
    s, x, _ = surrogate("mlp", "f32", batch=MAXB, seed=7)
    dev = s.temporal(torch.from_numpy(x).cuda(), torch.from_numpy(W).cuda()).values
    assert torch.equal(dev.view(torch.int32), host.view(torch.int32))
    s, x, _ = surrogate("mlp", "f32", batch=MAXB, seed=7)
    odd = torch.zeros(3 * 12 + 1, device="cuda")[1:].view(3, 12)          # device weights at an odd offset
    odd.copy_(torch.from_numpy(W))
    assert torch.equal(s.temporal(x, odd).values.view(torch.int32), host.view(torch.int32))
    s, x, _ = surrogate("mlp", "f32", batch=MAXB, seed=7)
    assert torch.equal(s.temporal(x, W.astype(np.float64)).values.view(torch.int32), host.view(torch.int32))          # float64 host rows
    s, x, _ = surrogate("mlp", "f32", batch=MAXB, seed=7)
    assert torch.equal(s.temporal(x, W[1]).values[:, 0].view(torch.int32), host[:, 1].view(torch.int32))          # [T]: a single functional
    with pytest.raises(ValueError, match="weights: the last dimension is 11, expected T = 12"):
        s.temporal(x, W[:, :-1])
    with pytest.raises(ValueError, match="mode must be"):
        s.temporal(x, W, mode="mean")


def test_the_draw_row_is_reset_after_an_exception():
    """a batch that fails leaves the engine's draw row at 0: the next call of anything draws as if temporal had never been called"""
    W = TR.mixed_weights(3, 12)
    s, x, _ = surrogate("mlp", "f32", batch=2, seed=7)
    rows, calls = [], []
    set_draw_row, temporal = s.eng.set_draw_row, s.eng.temporal

    def recording(first_row):
        rows.append(int(first_row))
        return set_draw_row(first_row)

    def failing(*a, **kw):
        calls.append(1)
        if len(calls) == 2:
            raise RuntimeError("the second batch fails")
        return temporal(*a, **kw)
    s.eng.set_draw_row, s.eng.temporal = recording, failing
    try:
        with pytest.raises(RuntimeError, match="the second batch fails"):
            s.temporal(x, W, mode="random")
    finally:
        del s.eng.set_draw_row, s.eng.temporal
    assert rows == [0, 2, 0]          # the two batches that were started, then the reset
    # and the engine is as good as new: a fresh Surrogate on it gives the bits of test_the_batch_size_does_not_show's runs
    s, x, _ = surrogate("mlp", "f32", batch=2, seed=7)
    a = s.temporal(x, W, mode="random").values
    s, x, _ = surrogate("mlp", "f32", batch=8, seed=7)
    assert torch.equal(a.view(torch.int32), s.temporal(x, W, mode="random").values.view(torch.int32))


@pytest.mark.parametrize("kind,dtype", [("img", "f32"), ("mlp", "bf16")])
def test_temporal_commutes_with_project(kind, dtype):
    """sum_t Wt[a, t] project(Wm)[p, t, b] and sum_n Wm[b, n] temporal(Wt)[p, a, n] are the same double sum over the field; both are
    finished in float64 and held to the sum of their propagated a-priori bounds, sum_t |Wt| bound_project + sum_n |Wm| bound_temporal,
    plus the float64 roundings of the finishing contractions (2^-50 of the sum of the magnitudes: generous)"""
    s, x, _ = surrogate(kind, dtype, batch=8, seed=9)
    F = s.predict(x).cpu().numpy()
    P, T, N = F.shape
    Wt, Wm = TR.mixed_weights(5, T, seed=1), PR.mixed_weights(4, N, seed=1)
    s, x, _ = surrogate(kind, dtype, batch=8, seed=9)
    proj = s.project(x, Wm).values.cpu().numpy().astype(np.float64)          # [P, T, 4]
    s, x, _ = surrogate(kind, dtype, batch=8, seed=9)
    temp = s.temporal(x, Wt).values.cpu().numpy().astype(np.float64)         # [P, 5, N]
    Wt64, Wm64 = Wt.astype(np.float64), Wm.astype(np.float64)
    a = np.einsum("at,ptb->pab", Wt64, proj)
    b = np.einsum("pan,bn->pab", temp, Wm64)
    slack = np.einsum("at,ptb->pab", np.abs(Wt64), PR.bound(F, Wm)) + np.einsum("pan,bn->pab", TR.bound(F, Wt), np.abs(Wm64))
    mag = np.einsum("at,ptn,bn->pab", np.abs(Wt64), np.abs(F).astype(np.float64), np.abs(Wm64))
    ratio = float((np.abs(a - b) / (slack + 2.0 ** -50 * mag)).max())
    print(f"  {kind} {dtype}: worst |project then time - temporal then mesh| / bound {ratio:.4f}")
    assert ratio <= 1.0


@pytest.mark.parametrize("kind,dtype", [("img", "f32"), ("mlp", "bf16")])
def test_fourier_amplitudes_against_the_fft_of_predict(kind, dtype):
    """fourier_rows -> amplitude() against 2 / T |rfft(predict)| at bin frequencies 1 .. 3 of T = 12.  Propagated bound per node: the
    cos and the sin value are each off by at most the a-priori bound of their sum plus the fp32 rounding of their weights
    (2^-24 sum_t |W F|); the modulus of a vector moves by no more than the vector, |d hypot| <= hypot(dc, ds) <= dc + ds; hypot itself is
    computed in fp32, a few ulp: 4 * 2^-24 relative allowed."""
    dt = 0.05
    s, x, _ = surrogate(kind, dtype, batch=8, seed=4)
    F = s.predict(x).cpu().numpy()
    P, T, N = F.shape
    ks = [1, 2, 3]
    W = fourier_rows(T, [k / (T * dt) for k in ks], dt=dt)
    s, x, _ = surrogate(kind, dtype, batch=8, seed=4)
    res = s.temporal(x, W)
    amp, ph = res.amplitude().cpu().numpy(), res.phase().cpu().numpy()
    assert amp.shape == (P, 3, N) and ph.shape == (P, 3, N)
    spec = np.fft.rfft(F.astype(np.float64), axis=1)
    want = 2.0 / T * np.abs(spec[:, ks])
    part = TR.bound(F, W) + U * (np.abs(W.astype(np.float64)) @ np.abs(F.astype(np.float64)))          # [P, 6, N]
    slack = part[:, 0::2] + part[:, 1::2] + 4 * U * want
    ratio = float((np.abs(amp - want) / slack).max())
    print(f"  {kind} {dtype}: worst |amplitude - 2 / T |rfft|| / bound {ratio:.4f}")
    assert ratio <= 1.0
    # the phase of A cos(w t - phi) is -arg of the FFT's coefficient; compared where the amplitude is far above its own error
    sure = want > 1e3 * slack
    assert sure.any()
    dphi = ph - (-np.angle(spec[:, ks]))
    assert np.all(np.abs((dphi[sure] + np.pi) % (2 * np.pi) - np.pi) <= 2e-3)
    where, top = res.peak()
    v = res.values.cpu().numpy()
    assert np.array_equal(where.cpu().numpy(), np.abs(v).argmax(axis=2))
    assert np.array_equal(top.cpu().numpy(), np.take_along_axis(v, np.abs(v).argmax(axis=2)[..., None], 2)[..., 0])
