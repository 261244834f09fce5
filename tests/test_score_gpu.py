"""Surrogate scoring on the GPU: Engine.score (sgv_score) against numpy reductions of what Engine.generate writes on the same
engine, latents and injected noise, minus the truth; what a score leaves behind in the engine; and Surrogate.score against the
reference's fields (tests/golden/predict_small.npz) and against reductions of Surrogate.predict.

u = 2^-24.  Bounds:
  * max |e| and its indices against reductions of E = generated field - truth (numpy float32, the kernel's one subtraction): none,
    bit for bit (ties to the smallest index as np.argmax);
  * bias, the mean squares and the mean of truth^2 against float64 sums of E, E^2, truth^2: the summation bound of
    tests/test_score_kernel_gpu.py, (m - 1 + 2) u sum|terms| / count -- an fp32 sum of m terms in any order, the squares' rounding
    and the one division; m = T for the node sums, m = min(N, 512) (one column block) for the frame sums, combined in fp64;
  * Surrogate.score on fp32 models against float64 reductions of (the fixture's fields - truth): the bound tests/test_predict_gpu.py
    asserts for predict, tol_n = 3e-4 / |scale_n| per element, widened by the subtraction, te = tol + u |e_ref|, and carried through
    the reductions as in tests/test_score_kernel_gpu.py (a maximum within the largest te over the reduced axis, an index i accepted
    iff | |e_ref[i]| - |e_ref[j]| | <= te[i] + te[j] with j the reference's own argmax, the bias within mean(te) + the summation
    bound, a mean square within mean(2 |e_ref| te + te^2) + the summation bound);
  * rmse, rel_l2 (fp64 on the device) against numpy float64 of the frame outputs: (T + 4) 2^-52 relative, an fp64 sum of T terms,
    the division and the square root; max_abs exactly."""
import ctypes as C

import numpy as np
import pytest
import torch

import simulgen_vae_amd  # noqa: F401
from simulgen_vae_amd import engine as E
from simulgen_vae_amd.predict import ScoreResult
from tests.surrogate_common import MAXB, engine, latents, no_forward_after, same_result, signed_scaler, surrogate, training_unaffected

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
INT_FIELDS = ("t_worst", "n_worst")
F64_FIELDS = ("rmse", "rel_l2")


def perturbed(F, scale, seed=41):
    """a truth near the field F [P, T, N]: F (1 + 0.1 g1) + 0.05 g2 / |scale_n|, fp32"""
    g = np.random.default_rng(seed)
    F64 = np.asarray(F, np.float32).astype(np.float64)
    return (F64 * (1 + 0.1 * g.standard_normal(F64.shape)) + 0.05 * g.standard_normal(F64.shape) / np.abs(np.asarray(scale, np.float64))).astype(np.float32)


def sum_bound(abs_terms, axis, m):
    return (m - 1 + 2) * U * abs_terms.sum(axis=axis) / abs_terms.shape[axis]


def as_numpy(res):
    """a ScoreResult, or Engine.score's dict, under ScoreResult's names (the per-condition fields only for a ScoreResult)"""
    if isinstance(res, ScoreResult):
        return {k: getattr(res, k).cpu().numpy() for k in ScoreResult.FIELDS}
    ne, nw, fe, fw = (res[k].cpu().numpy() for k in ("node_err", "node_when", "frame_err", "frame_where"))
    return dict(node_max_abs=ne[:, 0], node_bias=ne[:, 1], node_mse=ne[:, 2], t_worst=nw, frame_max_abs=fe[:, :, 0], frame_mse=fe[:, :, 1],
                frame_truth_ms=fe[:, :, 2], n_worst=fw)


def assert_reduces(got, F, truth):
    """got (as_numpy) is the reduction of E = F - truth (fp32): maxima and indices exact, the sums within the summation bound"""
    E32 = F - truth
    assert E32.dtype == np.float32 and np.isfinite(E32).all()
    A, E64, t64 = np.abs(E32), E32.astype(np.float64), truth.astype(np.float64)
    P, T, N = F.shape
    mf = min(N, 512)
    for k, want in (("node_max_abs", A.max(axis=1)), ("frame_max_abs", A.max(axis=2))):
        assert got[k].dtype == np.float32 and got[k].shape == want.shape and np.array_equal(got[k].view(np.int32), want.view(np.int32)), k
    for k, want in (("t_worst", A.argmax(axis=1)), ("n_worst", A.argmax(axis=2))):
        assert got[k].dtype == np.int32 and np.array_equal(got[k], want), k
    for k, want, bound in (("node_bias", E64.mean(axis=1), sum_bound(np.abs(E64), 1, T)), ("node_mse", (E64 ** 2).mean(axis=1), sum_bound(E64 ** 2, 1, T)),
                           ("frame_mse", (E64 ** 2).mean(axis=2), sum_bound(E64 ** 2, 2, mf)), ("frame_truth_ms", (t64 ** 2).mean(axis=2), sum_bound(t64 ** 2, 2, mf))):
        err = np.abs(got[k].astype(np.float64) - want)
        assert got[k].dtype == np.float32 and np.all(err <= bound), f"{k}: worst err/bound {np.max(err / bound):.3f}"


def assert_per_condition(got):
    """rmse, rel_l2, max_abs against numpy float64 of the frame outputs"""
    mse, tms = got["frame_mse"].astype(np.float64), got["frame_truth_ms"].astype(np.float64)
    T = mse.shape[1]
    assert got["rmse"].dtype == np.float64 and got["rel_l2"].dtype == np.float64 and got["max_abs"].dtype == np.float32
    for k, want in (("rmse", np.sqrt(mse.mean(axis=1))), ("rel_l2", np.sqrt(mse.sum(axis=1) / tms.sum(axis=1)))):
        assert got[k].shape == want.shape and np.all(np.abs(got[k] - want) <= (T + 4) * 2.0 ** -52 * want), k
    assert np.array_equal(got["max_abs"], got["frame_max_abs"].max(axis=1))


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("B", [1, 3, MAXB])
@pytest.mark.parametrize("name", ["G0", "G1"])
def test_score_reduces_what_generate_writes_minus_truth(name, B, dtype):
    cfg, eng = engine(name, dtype)
    z, xs, eps = latents(cfg, B)
    sc_np, mn_np = signed_scaler(cfg.num_node)
    scale, mn = torch.from_numpy(sc_np).cuda(), torch.from_numpy(mn_np).cuda()
    eng.set_eps(eps)
    F = eng.generate(z, xs, scale, mn, fix=True).cpu().numpy()
    truth = perturbed(F, sc_np)
    tr = torch.from_numpy(truth).cuda()
    eng.set_eps(eps)
    res = eng.score(z, xs, scale, mn, tr, fix=True)
    assert sorted(res) == ["frame_err", "frame_where", "node_err", "node_when"]
    assert res["node_err"].shape == (B, 3, cfg.num_node) and res["node_when"].shape == (B, cfg.num_node)
    assert res["frame_err"].shape == (B, cfg.num_time, 3) and res["frame_where"].shape == (B, cfg.num_time)
    assert_reduces(as_numpy(res), F, truth)
    assert torch.equal(tr, torch.from_numpy(truth).cuda())
    # a subset of the outputs, into buffers of the caller
    for want, names in ((("frame",), ["frame_err", "frame_where"]), (("node",), ["node_err", "node_when"])):
        eng.set_eps(eps)
        mine = {names[0]: torch.full_like(res[names[0]], float("nan"))}
        sub = eng.score(z, xs, scale, mn, tr, fix=True, want=want, out=mine)
        assert sorted(sub) == names and sub[names[0]] is mine[names[0]]
        assert all(torch.equal(sub[k].view(torch.int32), res[k].view(torch.int32)) for k in names)


def test_score_checks_its_arguments():
    cfg, eng = engine("G0", "f32")
    z, xs, eps = latents(cfg, 2)
    scale, mn = (torch.from_numpy(a).cuda() for a in signed_scaler(cfg.num_node))
    T, N = cfg.num_time, cfg.num_node
    tr = torch.zeros(2, T, N, device="cuda")
    with pytest.raises(ValueError, match="want must name"):
        eng.score(z, xs, scale, mn, tr, want=("probes",))
    with pytest.raises(ValueError, match="want must name"):
        eng.score(z, xs, scale, mn, tr, want=())
    with pytest.raises(ValueError, match="scale must be"):
        eng.score(z, xs, scale[:-1], mn, tr)
    with pytest.raises(ValueError, match="xs of shape"):
        eng.score(z, xs[:-1], scale, mn, tr)
    for bad in (tr[:1], tr.cpu(), tr.double(), tr.transpose(1, 2), torch.zeros(2, N, T, device="cuda"), tr.cpu().numpy()):
        with pytest.raises(ValueError, match="truth must be a contiguous float32 CUDA tensor"):
            eng.score(z, xs, scale, mn, bad)
    with pytest.raises(ValueError, match=r"out\['node_when'\]"):
        eng.score(z, xs, scale, mn, tr, want=("node",), out={"node_when": torch.empty(2, 2, N, device="cuda")})
    # the C entry point itself: SGV_ERR_ARG before anything is enqueued, so the forward of a decode stays readable
    eng.set_eps(eps)
    eng.decode(z, xs, fix=True)
    xs_t = torch.stack(xs).contiguous()
    ne = torch.empty(2, 3, N, device="cuda")
    fe = torch.empty(2 * T * 3 + 4, device="cuda")
    trp = torch.zeros(2 * T * N + 4, device="cuda")
    good = E.ScoreOut(node_err=ne.data_ptr())
    args = [z.data_ptr(), xs_t.data_ptr(), 2, 1, scale.data_ptr(), mn.data_ptr(), trp.data_ptr()]

    def rejected(msg, so=good, **kw):
        a = list(args)
        for i, v in kw.items():
            a[int(i[1:])] = v
        assert eng.lib.sgv_score(eng.h, *a, None if so is None else C.byref(so)) == -1
        assert msg in eng.lib.sgv_last_error().decode(), eng.lib.sgv_last_error().decode()

    rejected("null argument", so=None)
    for i in (0, 4, 5, 6):          # z, scale, min, truth
        rejected("null argument", **{f"a{i}": None})
    rejected("needs xs", a1=None)
    rejected("batch 0 outside", a2=0)
    rejected("all four outputs are NULL", so=E.ScoreOut())
    rejected("misaligned pointer", so=E.ScoreOut(node_err=ne.data_ptr() + 4))
    rejected("misaligned pointer", so=E.ScoreOut(node_when=ne.data_ptr() + 8))
    rejected("misaligned pointer", so=E.ScoreOut(frame_err=fe.data_ptr() + 2))
    rejected("misaligned pointer", so=E.ScoreOut(frame_where=fe.data_ptr() + 1))
    rejected("misaligned pointer", a6=trp.data_ptr() + 4)
    assert eng.lib.sgv_score(None, *args, C.byref(good)) == -1
    eng.xhat()
    # frame outputs need 4-byte alignment only
    eng.set_eps(eps)
    assert eng.lib.sgv_score(eng.h, *args, C.byref(E.ScoreOut(frame_err=fe.data_ptr() + 4))) == 0
    torch.cuda.synchronize()


def test_no_forward_to_read_after_score_and_generate_is_unchanged():
    cfg, eng = engine("G0", "bf16")
    no_forward_after(eng, cfg, lambda z, xs, scale, mn, before: eng.score(z, xs, scale, mn, before * 1.25),
                     (eng.xhat, lambda: eng.activation("x_hat", (2, cfg.num_node, cfg.num_time)), lambda: eng.backward(1.0, 1.0)))


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_training_is_unaffected_by_score(dtype):
    training_unaffected(dtype, lambda eng, z, xs, scale, mn, i: eng.score(z, xs, scale, mn, torch.ones(2, eng.cfg.num_time, eng.cfg.num_node, device="cuda")), True)


# ---- Surrogate.score ----
def _index_ok(a_ref, te, idx, axis):
    j = a_ref.argmax(axis=axis)
    pick = lambda a, i: np.take_along_axis(a, np.expand_dims(i, axis), axis).squeeze(axis)
    return np.abs(pick(a_ref, idx) - pick(a_ref, j)) <= pick(te, idx) + pick(te, j)


@pytest.mark.parametrize("kind", ["img", "mlp"])
def test_score_matches_the_reference_fp32(kind):
    s, x, g = surrogate(kind, "f32")
    ref = np.asarray(g[kind + "_fields"], np.float64)            # [6, 12, 520]
    P, T, N = ref.shape
    sc64 = np.asarray(g["data_scale"], np.float64)
    truth = perturbed(ref, sc64)
    res = s.score(x, truth)
    assert isinstance(res, ScoreResult)
    got = as_numpy(res)
    assert got["node_max_abs"].shape == (P, N) and got["t_worst"].shape == (P, N) and got["frame_mse"].shape == (P, T) and got["n_worst"].shape == (P, T)
    assert got["rmse"].shape == (P,) and got["rel_l2"].shape == (P,) and got["max_abs"].shape == (P,)
    assert all(getattr(res, k).is_contiguous() for k in ("node_bias", "t_worst", "frame_truth_ms", "n_worst"))
    e = ref - truth.astype(np.float64)
    a = np.abs(e)
    te = np.broadcast_to(3e-4 / np.abs(sc64)[None, None, :], ref.shape) + U * a
    sq_el, up, t64 = 2 * a * te + te ** 2, a + te, truth.astype(np.float64)
    mf = min(N, 512)
    checks = {
        "node_max_abs": (np.abs(got["node_max_abs"] - a.max(axis=1)), te.max(axis=1)),
        "frame_max_abs": (np.abs(got["frame_max_abs"] - a.max(axis=2)), te.max(axis=2)),
        "node_bias": (np.abs(got["node_bias"] - e.mean(axis=1)), te.mean(axis=1) + sum_bound(up, 1, T)),
        "node_mse": (np.abs(got["node_mse"] - (e ** 2).mean(axis=1)), sq_el.mean(axis=1) + sum_bound(up ** 2, 1, T)),
        "frame_mse": (np.abs(got["frame_mse"] - (e ** 2).mean(axis=2)), sq_el.mean(axis=2) + sum_bound(up ** 2, 2, mf)),
        "frame_truth_ms": (np.abs(got["frame_truth_ms"] - (t64 ** 2).mean(axis=2)), sum_bound(t64 ** 2, 2, mf)),
    }
    print(f"  {kind} fp32: worst err/bound " + ", ".join(f"{k} {np.max(err / b):.3f}" for k, (err, b) in checks.items()))
    for k, (err, b) in checks.items():
        assert np.all(err <= b), f"{k}: worst err/bound {np.max(err / b):.3f}"
    assert _index_ok(a, te, got["t_worst"], 1).all() and _index_ok(a, te, got["n_worst"], 2).all()
    assert_per_condition(got)


@pytest.mark.parametrize("kind", ["img", "mlp"])
def test_score_reduces_what_predict_writes_bf16(kind):
    s, x, g = surrogate(kind, "bf16", seed=3)
    F = s.predict(x).cpu().numpy()
    truth = perturbed(F, g["data_scale"])
    s, x, _ = surrogate(kind, "bf16", seed=3)                    # a new Surrogate re-seeds the engine: the same draws again
    got = as_numpy(s.score(x, truth))
    assert_reduces(got, F, truth)
    assert_per_condition(got)


def test_ragged_last_batch_equals_split_calls_and_host_truth_equals_device_truth():
    s, x, g = surrogate("img", "f32", seed=11)
    truth = perturbed(g["img_fields"], g["data_scale"])
    whole = s.score(x, truth)                                    # 6 conditions at batch 4: 4 + 2; host truth (numpy)
    assert whole.node_mse.shape == (6, 520) and whole.n_worst.shape == (6, 12)
    s, x, _ = surrogate("img", "f32", seed=11)
    first, second = s.score(x[:4], truth[:4]), s.score(torch.from_numpy(x[4:]).cuda(), torch.from_numpy(truth[4:]).cuda())
    same_result(whole, ScoreResult(**{k: torch.cat([getattr(first, k), getattr(second, k)]) for k in ScoreResult.FIELDS}))
    s, x, _ = surrogate("img", "f32", seed=11)
    same_result(whole, s.score(x, torch.from_numpy(truth).cuda()))    # device truth
    s, x, _ = surrogate("img", "f32", seed=11)
    same_result(whole, s.score(x, torch.from_numpy(truth)))           # CPU tensor
    with pytest.raises(ValueError, match="truth: dimension P is 5, expected P = 6"):
        s.score(x, truth[:5])
    with pytest.raises(ValueError, match="truth: dtype float32 is required, not float64"):
        s.score(x, truth.astype(np.float64))
    with pytest.raises(ValueError, match="mode must be"):
        s.score(x, truth, mode="mean")


def test_sampling_mode_scores_what_predict_samples():
    s, x, g = surrogate("mlp", "f32", seed=21)
    F = s.predict(x, mode="random").cpu().numpy()
    truth = perturbed(F, g["data_scale"])
    s, x, _ = surrogate("mlp", "f32", seed=21)
    got = s.score(x, truth, mode="random")
    assert_reduces(as_numpy(got), F, truth)
    s, x, _ = surrogate("mlp", "f32", seed=21)
    assert not torch.equal(s.score(x, truth, mode="fix").node_max_abs, got.node_max_abs)
