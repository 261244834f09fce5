"""Surrogate Gram matrices and POD on the GPU: Engine.gram (sgv_gram) against float64 on what Engine.generate writes on the same
engine, latents and injected noise; what a call leaves behind in the engine; and Surrogate.gram / Surrogate.pod against float64 on
Surrogate.predict, on the models of tests/golden/predict_small.npz.

Against float64 the matrices are held to the a-priori bound of an fp32 summation in any order,
|G - G64| <= (N + 3) 2^-24 sum_n |w d_t d_t'| with d the fp32 difference F - m (tests/gram_reference.py), F the stored field.  predict,
gram and temporal draw the decoder's noise per call, so a comparison of two of them makes one call of each on Surrogates with the same
seed (the rule of tests/test_sweep_gpu.py)."""
import os
import sys

import numpy as np
import pytest
import torch

import simulgen_vae_amd  # noqa: F401
from simulgen_vae_amd.predict import GramResult, PodResult
from tests.surrogate_common import MAXB, engine, latents, no_forward_after, signed_scaler, surrogate, training_unaffected

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gram_reference as GR  # noqa: E402
import temporal_reference as TR  # noqa: E402

pytestmark = pytest.mark.gpu
U = 2.0 ** -24


def within_bound(g, F, w, m, what):
    ratio = GR.worst_ratio(g, F, w, m)
    print(f"  {what}: worst err / bound {ratio:.4f}")
    assert ratio <= 1.0, f"{what}: worst err / bound {ratio:.3f}"
    g = np.asarray(g)
    assert np.array_equal(g.view(np.int32), np.ascontiguousarray(np.swapaxes(g, 1, 2)).view(np.int32)), f"{what}: bitwise symmetric"
    assert (np.diagonal(g, axis1=1, axis2=2) >= 0).all()


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("B", [1, 3, MAXB])
@pytest.mark.parametrize("name", ["G0", "G1"])
def test_gram_multiplies_what_generate_writes(name, B, dtype):
    cfg, eng = engine(name, dtype)
    T, N = cfg.num_time, cfg.num_node
    z, xs, eps = latents(cfg, B)
    scale, mn = (torch.from_numpy(a).cuda() for a in signed_scaler(N))
    eng.set_eps(eps)
    F = eng.generate(z, xs, scale, mn, fix=True).cpu().numpy()
    w, m = GR.mixed_weights(N), GR.mixed_offset(F)
    for what, ww, mm in (("neither", None, None), ("w", w, None), ("m", None, m), ("both", w, m)):
        eng.set_eps(eps)
        g = eng.gram(z, xs, scale, mn, node_weights=dev(ww), offset=dev(mm), fix=True)
        assert g.dtype == torch.float32 and g.shape == (B, T, T) and g.is_contiguous()
        within_bound(g.cpu().numpy(), F, ww, mm, f"{name} B {B} {dtype} {what}")
    # into the rows of a larger tensor
    big = torch.full((B + 2, T, T), float("nan"), device="cuda")
    eng.set_eps(eps)
    assert eng.gram(z, xs, scale, mn, node_weights=dev(w), offset=dev(m), fix=True, out=big[1:B + 1]).data_ptr() == big[1:].data_ptr()
    got = big.cpu().numpy()
    assert np.isnan(got[0]).all() and np.isnan(got[B + 1]).all()
    assert np.array_equal(got[1:B + 1].view(np.int32), g.cpu().numpy().view(np.int32))


def test_gram_checks_its_arguments():
    cfg, eng = engine("G0", "f32")
    z, xs, eps = latents(cfg, 2)
    scale, mn = (torch.from_numpy(a).cuda() for a in signed_scaler(cfg.num_node))
    T, N = cfg.num_time, cfg.num_node
    w = torch.ones(N, device="cuda")
    for bad in (w[:-1], w.double(), w.cpu(), torch.ones((1, N), device="cuda"), torch.ones(2 * N, device="cuda")[::2], w.cpu().numpy()):
        with pytest.raises(ValueError, match="node_weights must be None or a contiguous float32 CUDA tensor of shape"):
            eng.gram(z, xs, scale, mn, node_weights=bad)
        with pytest.raises(ValueError, match="offset must be None or a contiguous float32 CUDA tensor of shape"):
            eng.gram(z, xs, scale, mn, offset=bad)
    for bad in (torch.zeros((2, T, T + 1), device="cuda"), torch.zeros((1, T, T), device="cuda"), torch.zeros((2, T, T), device="cuda").double(),
                torch.zeros((2, T, T))):
        with pytest.raises(ValueError, match="out must be a contiguous float32 CUDA tensor of shape"):
            eng.gram(z, xs, scale, mn, out=bad)
    with pytest.raises(ValueError, match="scale must be"):
        eng.gram(z, xs, scale[:-1], mn)
    # the C entry point itself: SGV_ERR_ARG before anything is enqueued, so the forward of a decode stays readable
    eng.set_eps(eps)
    eng.decode(z, xs, fix=True)
    xs_t = torch.stack(xs).contiguous()
    out = torch.full((2, T, T), 768.0, device="cuda")
    args = [z.data_ptr(), xs_t.data_ptr(), 2, 1, scale.data_ptr(), mn.data_ptr(), w.data_ptr(), w.data_ptr(), out.data_ptr()]

    def rejected(msg, **kw):
        a = list(args)
        for i, v in kw.items():
            a[int(i[1:])] = v
        assert eng.lib.sgv_gram(eng.h, *a) == -1
        assert msg in eng.lib.sgv_last_error().decode(), eng.lib.sgv_last_error().decode()

    for i in (0, 4, 5, 8):          # z, scale, min, out
        rejected("null argument", **{f"a{i}": None})
    rejected("needs xs", a1=None)
    rejected("batch 0 outside", a2=0)
    rejected(f"batch {MAXB + 1} outside", a2=MAXB + 1)
    rejected("misaligned pointer", a6=w.data_ptr() + 4)
    rejected("misaligned pointer", a7=w.data_ptr() + 8)
    rejected("misaligned pointer", a8=out.data_ptr() + 2)
    assert eng.lib.sgv_gram(None, *args) == -1
    eng.xhat()
    torch.cuda.synchronize()
    assert bool((out == 768.0).all())


def test_no_forward_to_read_after_gram_and_generate_is_unchanged():
    cfg, eng = engine("G0", "bf16")
    w = GR.mixed_weights(cfg.num_node)

    def run(z, xs, scale, mn, before):
        g = eng.gram(z, xs, scale, mn, node_weights=dev(w))
        within_bound(g.cpu().numpy(), before.cpu().numpy(), w, None, "after decode")
    no_forward_after(eng, cfg, run, (eng.xhat, lambda: eng.backward(1.0, 1.0)))


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_training_is_unaffected_by_gram(dtype):
    def run(eng, z, xs, scale, mn, i):
        eng.gram(z, xs, scale, mn, node_weights=dev(GR.mixed_weights(eng.cfg.num_node)))
    training_unaffected(dtype, run, True)


# ---- Surrogate.gram and Surrogate.pod on the fixture's models: P = 6 conditions, T = 12, N = 520 ----
N_FIX = 520


def weights_and_offset(F):
    return GR.mixed_weights(F.shape[-1], seed=3), GR.mixed_offset(F, seed=3)


@pytest.mark.parametrize("mode", ["fix", "random"])
@pytest.mark.parametrize("kind,dtype", [("img", "f32"), ("mlp", "bf16")])
def test_surrogate_gram_multiplies_what_predict_writes(kind, dtype, mode):
    s, x, _ = surrogate(kind, dtype, batch=8, seed=5)          # batch >= P: one call of the decoder each
    F = s.predict(x, mode=mode).cpu().numpy()
    P, T, N = F.shape
    w, m = weights_and_offset(F)
    for what, ww, mm in (("neither", None, None), ("both", w, m)):
        s, x, _ = surrogate(kind, dtype, batch=8, seed=5)          # a new Surrogate re-seeds the engine: the same draws again
        res = s.gram(x, node_weights=ww, offset=mm, mode=mode)
        assert isinstance(res, GramResult) and res.values.dtype == torch.float32 and res.values.shape == (P, T, T) and res.values.is_contiguous()
        assert res.num_node == N
        within_bound(res.values.cpu().numpy(), F, ww, mm, f"{kind} {dtype} {mode} {what}")
    # energy() is the weighted sum of squares of predict about the offset, in float64, within the bound of the diagonal
    d = (F - m).astype(np.float32).astype(np.float64)
    e64 = (d * d * w.astype(np.float64)).sum(axis=2)
    bnd = np.diagonal(GR.bound(F, w, m), axis1=1, axis2=2)
    assert res.energy().shape == (P, T) and res.energy().dtype == np.float64
    assert (np.abs(res.energy() - e64) <= bnd).all()
    assert np.abs(res.total() - GR.reference64(F, w, m).sum(axis=0)).max() <= res.noise_floor()


@pytest.mark.parametrize("mode", ["fix", "random"])
def test_the_batch_size_does_not_show(mode):
    """Batch sizes 2 and 3 at P = 5 (a ragged last batch either way) and 8 give bitwise-equal matrices: the kernel gives a sample the
    same bits in any batch, and condition p takes row p of the noise streams one call over all conditions would draw from
    (Engine.set_draw_row), so the draw position also ends where one call leaves it."""
    runs, draws = [], []
    for batch in (2, 3, 8):
        s, x, _ = surrogate("mlp", "f32", batch=batch, seed=7)
        w = GR.mixed_weights(N_FIX, seed=3)
        runs.append(s.gram(x[:5], node_weights=w, offset=np.full(N_FIX, 0.25, np.float32), mode=mode).values)
        draws.append(s.eng.train_state()["draw"])
    assert all(r.shape == (5, 12, 12) for r in runs)
    for other in runs[1:]:
        assert torch.equal(runs[0].view(torch.int32), other.view(torch.int32))
    assert len(set(draws)) == 1 and draws[0] > 0
    # and the one call is predict's: the same draws, the same field
    s, x, _ = surrogate("mlp", "f32", batch=8, seed=7)
    F = s.predict(x[:5], mode=mode).cpu().numpy()
    assert s.eng.train_state()["draw"] == draws[0]
    within_bound(runs[0].cpu().numpy(), F, w, np.full(N_FIX, 0.25, np.float32), f"batch 2 against a one-call predict, {mode}")


def test_host_and_device_weights_and_offsets_give_the_same_bits():
    w = GR.mixed_weights(N_FIX, seed=3)
    m = np.random.default_rng(1).standard_normal(N_FIX).astype(np.float32)
    s, x, _ = surrogate("mlp", "f32", batch=MAXB, seed=7)
    host = s.gram(x, node_weights=w, offset=m).values
    s, x, _ = surrogate("mlp", "f32", batch=MAXB, seed=7)
    got = s.gram(torch.from_numpy(x).cuda(), node_weights=dev(w), offset=dev(m)).values
    assert torch.equal(got.view(torch.int32), host.view(torch.int32))
    s, x, _ = surrogate("mlp", "f32", batch=MAXB, seed=7)
    odd_w, odd_m = (torch.zeros(N_FIX + 1, device="cuda")[1:] for _ in range(2))          # device vectors at an odd offset
    odd_w.copy_(torch.from_numpy(w))
    odd_m.copy_(torch.from_numpy(m))
    assert odd_w.data_ptr() % 16 == 4
    assert torch.equal(s.gram(x, node_weights=odd_w, offset=odd_m).values.view(torch.int32), host.view(torch.int32))
    s, x, _ = surrogate("mlp", "f32", batch=MAXB, seed=7)
    assert torch.equal(s.gram(x, node_weights=w.astype(np.float64), offset=m.astype(np.float64)).values.view(torch.int32), host.view(torch.int32))
    s, x, _ = surrogate("mlp", "f32", batch=MAXB, seed=7)
    ones = s.gram(x, node_weights=np.ones(N_FIX), offset=np.zeros(N_FIX)).values
    s, x, _ = surrogate("mlp", "f32", batch=MAXB, seed=7)
    assert torch.equal(s.gram(x).values.view(torch.int32), ones.view(torch.int32))          # w = 1, m = 0 are the defaults
    with pytest.raises(ValueError, match=r"node_weights: an \[N\] array with N = 520 is required"):
        s.gram(x, node_weights=w[:-1])
    with pytest.raises(ValueError, match="is negative"):
        s.gram(x, node_weights=-dev(w) - 1.0)
    with pytest.raises(ValueError, match="offset: an entry is not finite"):
        s.gram(x, offset=dev(m) / 0.0)
    with pytest.raises(ValueError, match="mode must be"):
        s.gram(x, mode="mean")


def test_the_draw_row_is_reset_after_an_exception():
    """a batch that fails leaves the engine's draw row at 0: the next call of anything draws as if gram had never been called"""
    s, x, _ = surrogate("mlp", "f32", batch=2, seed=7)
    rows, calls = [], []
    set_draw_row, gram = s.eng.set_draw_row, s.eng.gram

    def recording(first_row):
        rows.append(int(first_row))
        return set_draw_row(first_row)

    def failing(*a, **kw):
        calls.append(1)
        if len(calls) == 2:
            raise RuntimeError("the second batch fails")
        return gram(*a, **kw)
    s.eng.set_draw_row, s.eng.gram = recording, failing
    try:
        with pytest.raises(RuntimeError, match="the second batch fails"):
            s.gram(x, mode="random")
    finally:
        del s.eng.set_draw_row, s.eng.gram
    assert rows == [0, 2, 0]          # the two batches that were started, then the reset
    s, x, _ = surrogate("mlp", "f32", batch=2, seed=7)
    a = s.gram(x, mode="random").values
    s, x, _ = surrogate("mlp", "f32", batch=8, seed=7)
    assert torch.equal(a.view(torch.int32), s.gram(x, mode="random").values.view(torch.int32))


@pytest.mark.parametrize("kind,dtype", [("img", "f32"), ("mlp", "bf16")])
def test_modes_then_temporal_diagonalise_the_study(kind, dtype):
    """A = temporal(modes) gives sum_p A_p diag(w) A_p^T = rows G rows^T = diag(eigenvalues).  Propagated bound per entry: the
    computed total and the clamp are each within noise_floor() of the exact matrix in the 2-norm (rows orthonormal); the rows are
    rounded to fp32, 4 * 2^-24 sqrt(T) of the largest eigenvalue to first order; the amplitudes carry the a-priori bound dc of the
    temporal pass, 2 |A| w dc^T + dc w dc^T."""
    s, x, _ = surrogate(kind, dtype, batch=8, seed=9)
    F = s.predict(x).cpu().numpy()
    P, T, N = F.shape
    w = GR.mixed_weights(N, seed=3)
    s, x, _ = surrogate(kind, dtype, batch=8, seed=9)
    res = s.gram(x, node_weights=w)
    rows, lam, frac = res.modes()
    assert rows.shape == (T, T) and frac == 1.0
    s, x, _ = surrogate(kind, dtype, batch=8, seed=9)
    A = s.temporal(x, rows).values.cpu().numpy().astype(np.float64)          # [P, T, N]
    w64 = w.astype(np.float64)
    got = np.einsum("pan,n,pbn->ab", A, w64, A)
    dc = TR.bound(F, rows)
    slack = (2 * res.noise_floor() + 4 * U * np.sqrt(T) * lam[0] + np.einsum("pan,n,pbn->ab", np.abs(A), w64, dc)
             + np.einsum("pan,n,pbn->ab", dc, w64, np.abs(A)) + np.einsum("pan,n,pbn->ab", dc, w64, dc))
    ratio = float((np.abs(got - np.diag(lam)) / slack).max())
    print(f"  {kind} {dtype}: worst |A w A^T - diag(eigenvalues)| / bound {ratio:.4f}")
    assert ratio <= 1.0


@pytest.mark.parametrize("mode", ["fix", "random"])
@pytest.mark.parametrize("kind,dtype", [("img", "f32"), ("mlp", "bf16")])
def test_pod_at_full_rank_returns_predict(kind, dtype, mode):
    """pod(rank = T).reconstruct(p) against predict: the sum of the a-priori bounds of the two fp32 steps -- the temporal pass and the
    subtraction of S_r m (gram_reference.coefficient_bound), spread by |rows^T| -- plus the fp32 rounding of the rows and of F - m"""
    s, x, _ = surrogate(kind, dtype, batch=8, seed=11)          # batch >= P: predict draws per call, pod gives condition p row p of one call's streams
    F = s.predict(x, mode=mode).cpu().numpy()
    P, T, N = F.shape
    w, m = weights_and_offset(F)
    s, x, _ = surrogate(kind, dtype, batch=4, seed=11)
    pod = s.pod(x, rank=T, node_weights=w, offset=m, mode=mode)
    assert isinstance(pod, PodResult) and pod.rows.shape == (T, T) and pod.coefficients.shape == (P, T, N) and pod.fraction == 1.0
    assert pod.coefficients.dtype == torch.float32 and pod.eigenvalues.shape == (T,)
    dc = GR.coefficient_bound(pod.rows, F, pod.coefficients.cpu().numpy(), m)
    R = np.abs(pod.rows.astype(np.float64))
    d = np.abs(F.astype(np.float64) - m.astype(np.float64))
    worst = 0.0
    for p in range(P):
        rec = pod.reconstruct(p)
        assert rec.shape == (T, N) and rec.dtype == torch.float64
        bnd = R.T @ dc[p] + 4 * U * (R.T @ (R @ d[p])) + U * d[p] + 1e-30
        worst = max(worst, float((np.abs(rec.cpu().numpy() - F[p].astype(np.float64)) / bnd).max()))
    print(f"  {kind} {dtype} {mode}: worst |reconstruct - predict| / bound {worst:.4f}")
    assert worst <= 1.0


@pytest.mark.parametrize("rank", [1, 3])
@pytest.mark.parametrize("kind,dtype", [("img", "f32"), ("mlp", "bf16")])
def test_eckart_young_identity_at_a_truncated_rank(kind, dtype, rank):
    """sum_p ||Y_p - reconstruct_R(p)||_w^2 = the eigenvalues of total() left out, within gram_reference.eckart_young_tol -- the
    tolerance tests/test_gram_host.py holds the emulation to"""
    s, x, _ = surrogate(kind, dtype, batch=8, seed=11)          # batch >= P: one call of the decoder, the noise pod and gram see at any batch size
    F = s.predict(x).cpu().numpy()
    P, T, N = F.shape
    w, m = weights_and_offset(F)
    s, x, _ = surrogate(kind, dtype, batch=4, seed=11)
    res = s.gram(x, node_weights=w, offset=m)
    lam_all = res.modes()[1]
    s, x, _ = surrogate(kind, dtype, batch=4, seed=11)
    pod = s.pod(x, rank=rank, node_weights=w, offset=m)
    assert pod.rows.shape == (rank, T) and np.array_equal(pod.eigenvalues, lam_all[:rank]) and 0.0 < pod.fraction <= 1.0
    recon = np.stack([pod.reconstruct(p).cpu().numpy() for p in range(P)])
    lhs = GR.residual_energy(F, recon, w, m)
    rhs = float(lam_all[rank:].sum())
    dc = GR.coefficient_bound(pod.rows, F, pod.coefficients.cpu().numpy(), m)
    tol = GR.eckart_young_tol(res.noise_floor(), float(np.trace(res.total())), T, rank, pod.rows, dc, w)
    print(f"  {kind} {dtype} rank {rank}: residual {lhs:.9g}, eigenvalues left out {rhs:.9g}, |difference| {abs(lhs - rhs):.3g}, tolerance {tol:.3g}")
    assert abs(lhs - rhs) <= tol
