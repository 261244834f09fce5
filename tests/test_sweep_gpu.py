"""Surrogate field summaries on the GPU: Engine.summarize (sgv_summarize) against numpy reductions of what Engine.generate writes on
the same engine, latents and injected noise; what a summarize leaves behind in the engine; and Surrogate.sweep against the
reference's fields (tests/golden/predict_small.npz) and against reductions of Surrogate.predict.

Bounds:
  * extrema, their indices and the probes against reductions of a generated field: none, bit for bit (the summary pass reduces the
    values generate stores, ties to the smallest index as np.argmax / np.argmin);
  * the mean over time against the float64 mean of the generated field: (T + 2) * 2^-24 * max_t|field|, the worst case of an fp32 sum
    of T terms plus the division (tests/test_summary_kernel_gpu.py; the elements themselves are the same numbers here);
  * Surrogate.sweep on fp32 models against float64 reductions of the fixture's fields: the bound tests/test_predict_gpu.py asserts
    for predict, tol_n = 3e-4 / |scale_n| per element, carried through the reductions as in tests/test_summary_kernel_gpu.py
    (extrema within the largest tol over the reduced axis, probes within tol, the mean within mean_t(tol) + (T + 2) * 2^-24 *
    max_t|ref|, an index i accepted iff |ref[i] - ref[j]| <= tol[i] + tol[j] with j the reference's own arg-extremum)."""
import numpy as np
import pytest
import torch

import simulgen_vae_amd  # noqa: F401
from simulgen_vae_amd import engine as E
from simulgen_vae_amd.predict import SweepResult
from tests.surrogate_common import MAXB, engine, latents, no_forward_after, same_result, signed_scaler, surrogate, training_unaffected

pytestmark = pytest.mark.gpu


def probes_for(N):
    return np.array([0, N - 1, N // 3, N // 3, 7], np.int32)


def reduce_field(F, nodes=None):
    """numpy reductions of a [P, T, N] field under SweepResult's names (node_mean in float64)"""
    r = dict(node_max=F.max(axis=1), node_min=F.min(axis=1), node_mean=F.astype(np.float64).mean(axis=1), t_max=F.argmax(axis=1), t_min=F.argmin(axis=1),
             frame_max=F.max(axis=2), frame_min=F.min(axis=2), n_max=F.argmax(axis=2), n_min=F.argmin(axis=2))
    r["probes"] = None if nodes is None else F[:, :, nodes]
    return r


def as_numpy(res):
    """a SweepResult, or Engine.summarize's dict, under SweepResult's names"""
    if isinstance(res, SweepResult):
        return {k: None if getattr(res, k) is None else getattr(res, k).cpu().numpy() for k in SweepResult.FIELDS}
    ns, nw, fs, fw = (res[k].cpu().numpy() for k in ("node_stats", "node_when", "frame_stats", "frame_where"))
    return dict(node_max=ns[:, 0], node_min=ns[:, 1], node_mean=ns[:, 2], t_max=nw[:, 0], t_min=nw[:, 1], frame_max=fs[:, :, 0], frame_min=fs[:, :, 1],
                n_max=fw[:, :, 0], n_min=fw[:, :, 1], probes=res["probes"].cpu().numpy() if "probes" in res else None)


def assert_reduces(got, F, nodes=None):
    """got (as_numpy) is the reduction of the fp32 field F: exact but for the mean"""
    want = reduce_field(F, nodes)
    T = F.shape[1]
    for k in SweepResult.FIELDS:
        if k == "node_mean":
            err = np.abs(got[k].astype(np.float64) - want[k])
            assert got[k].dtype == np.float32 and np.all(err <= (T + 2) * 2.0 ** -24 * np.abs(F).max(axis=1)), k
        elif want[k] is None:
            assert got[k] is None
        else:
            assert got[k].dtype == (np.int32 if k in ("t_max", "t_min", "n_max", "n_min") else np.float32), k
            assert got[k].shape == want[k].shape and np.array_equal(got[k].view(np.int32), np.ascontiguousarray(want[k].astype(got[k].dtype)).view(np.int32)), k


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("B", [1, 3, MAXB])
@pytest.mark.parametrize("name", ["G0", "G1"])
def test_summarize_reduces_what_generate_writes(name, B, dtype):
    cfg, eng = engine(name, dtype)
    z, xs, eps = latents(cfg, B)
    scale, mn = (torch.from_numpy(a).cuda() for a in signed_scaler(cfg.num_node))
    nodes = probes_for(cfg.num_node)
    eng.set_eps(eps)
    F = eng.generate(z, xs, scale, mn, fix=True).cpu().numpy()
    eng.set_probes(nodes)
    eng.set_eps(eps)
    res = eng.summarize(z, xs, scale, mn, fix=True)
    assert sorted(res) == ["frame_stats", "frame_where", "node_stats", "node_when", "probes"]
    assert res["node_stats"].shape == (B, 3, cfg.num_node) and res["frame_where"].shape == (B, cfg.num_time, 2) and res["probes"].shape == (B, cfg.num_time, 5)
    assert_reduces(as_numpy(res), F, nodes)
    # a subset of the outputs, into buffers of the caller
    eng.set_eps(eps)
    mine = {"frame_stats": torch.full((B, cfg.num_time, 2), float("nan"), device="cuda")}
    sub = eng.summarize(z, xs, scale, mn, fix=True, want=("frame",), out=mine)
    assert sorted(sub) == ["frame_stats", "frame_where"] and sub["frame_stats"] is mine["frame_stats"]
    assert torch.equal(sub["frame_stats"], res["frame_stats"]) and torch.equal(sub["frame_where"], res["frame_where"])


def test_summarize_checks_its_arguments():
    cfg, eng = engine("G0", "f32")
    z, xs, eps = latents(cfg, 2)
    scale, mn = (torch.from_numpy(a).cuda() for a in signed_scaler(cfg.num_node))
    with pytest.raises(ValueError, match="want must name"):
        eng.summarize(z, xs, scale, mn, want=("nodes",))
    with pytest.raises(ValueError, match="want must name"):
        eng.summarize(z, xs, scale, mn, want=())
    with pytest.raises(ValueError, match="scale must be"):
        eng.summarize(z, xs, scale[:-1], mn)
    with pytest.raises(ValueError, match="xs of shape"):
        eng.summarize(z, xs[:-1], scale, mn)
    with pytest.raises(ValueError, match=r"out\['node_when'\]"):
        eng.summarize(z, xs, scale, mn, want=("node",), out={"node_when": torch.empty(2, 2, cfg.num_node, device="cuda")})
    eng.set_probes([])
    with pytest.raises(ValueError, match="no probe nodes are set"):
        eng.summarize(z, xs, scale, mn)
    for bad, msg in (([0, cfg.num_node], rf"nodes\[1\] = {cfg.num_node} is outside"), ([-1], r"nodes\[0\] = -1 is outside"), (np.zeros(4097, np.int32), "count 4097")):
        with pytest.raises(E.SgvError, match=msg):
            eng.set_probes(bad)
    # the C entry point itself: SGV_ERR_ARG before anything is enqueued, so the forward of a decode stays readable
    eng.set_eps(eps)
    eng.decode(z, xs, fix=True)
    xs_t = torch.stack(xs).contiguous()
    ns = torch.empty(2, 3, cfg.num_node, device="cuda")
    pr = torch.empty(2, cfg.num_time, 4, device="cuda")
    args = (z.data_ptr(), xs_t.data_ptr(), 2, 1, scale.data_ptr(), mn.data_ptr())
    import ctypes as C
    for so, msg in ((None, "null argument"), (E.SummaryOut(), "all five outputs are NULL"), (E.SummaryOut(probes=pr.data_ptr()), "no probe nodes are set"),
                    (E.SummaryOut(node_stats=ns.data_ptr() + 4), "misaligned output")):
        assert eng.lib.sgv_summarize(eng.h, *args, None if so is None else C.byref(so)) == -1
        assert msg in eng.lib.sgv_last_error().decode()
    assert eng.lib.sgv_summarize(eng.h, z.data_ptr(), None, 2, 1, scale.data_ptr(), mn.data_ptr(), C.byref(E.SummaryOut(node_stats=ns.data_ptr()))) == -1
    assert "needs xs" in eng.lib.sgv_last_error().decode()
    eng.xhat()


def test_no_forward_to_read_after_summarize_and_generate_is_unchanged():
    cfg, eng = engine("G0", "bf16")
    no_forward_after(eng, cfg, lambda z, xs, scale, mn, before: eng.summarize(z, xs, scale, mn, want=("node", "frame")),
                     (eng.xhat, lambda: eng.backward(1.0, 1.0)))


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_training_is_unaffected_by_summarize(dtype):
    training_unaffected(dtype, lambda eng, z, xs, scale, mn, i: eng.summarize(z, xs, scale, mn), True,
                        prepare=lambda eng: eng.set_probes(probes_for(eng.cfg.num_node)))


# ---- Surrogate.sweep ----
def _index_ok(ref, tol, idx, axis, largest):
    j = ref.argmax(axis=axis) if largest else ref.argmin(axis=axis)
    pick = lambda a, i: np.take_along_axis(a, np.expand_dims(i, axis), axis).squeeze(axis)
    return np.abs(pick(ref, idx) - pick(ref, j)) <= pick(tol, idx) + pick(tol, j)


@pytest.mark.parametrize("kind", ["img", "mlp"])
def test_sweep_matches_the_reference_fp32(kind):
    s, x, g = surrogate(kind, "f32")
    nodes = probes_for(520)
    got = as_numpy(s.sweep(x, probes=nodes))
    ref = np.asarray(g[kind + "_fields"], np.float64)            # [6, 12, 520]
    P, T, N = ref.shape
    tol = np.broadcast_to(3e-4 / np.abs(np.asarray(g["data_scale"], np.float64))[None, None, :], ref.shape)
    assert got["node_max"].shape == (P, N) and got["t_min"].shape == (P, N) and got["frame_min"].shape == (P, T) and got["n_max"].shape == (P, T)
    assert got["probes"].shape == (P, T, 5)
    checks = {
        "node_max": (np.abs(got["node_max"] - ref.max(axis=1)), tol.max(axis=1)),
        "node_min": (np.abs(got["node_min"] - ref.min(axis=1)), tol.max(axis=1)),
        "node_mean": (np.abs(got["node_mean"] - ref.mean(axis=1)), tol.mean(axis=1) + (T + 2) * 2.0 ** -24 * np.abs(ref).max(axis=1)),
        "frame_max": (np.abs(got["frame_max"] - ref.max(axis=2)), tol.max(axis=2)),
        "frame_min": (np.abs(got["frame_min"] - ref.min(axis=2)), tol.max(axis=2)),
        "probes": (np.abs(got["probes"] - ref[:, :, nodes]), tol[:, :, nodes]),
    }
    print(f"  {kind} fp32: worst err/bound " + ", ".join(f"{k} {np.max(e / b):.3f}" for k, (e, b) in checks.items()))
    for k, (e, b) in checks.items():
        assert np.all(e <= b), f"{k}: worst err/bound {np.max(e / b):.3f}"
    assert _index_ok(ref, tol, got["t_max"], 1, True).all() and _index_ok(ref, tol, got["t_min"], 1, False).all()
    assert _index_ok(ref, tol, got["n_max"], 2, True).all() and _index_ok(ref, tol, got["n_min"], 2, False).all()


@pytest.mark.parametrize("kind", ["img", "mlp"])
def test_sweep_reduces_what_predict_writes_bf16(kind):
    nodes = probes_for(520)
    s, x, _ = surrogate(kind, "bf16", seed=3)
    F = s.predict(x).cpu().numpy()
    s, x, _ = surrogate(kind, "bf16", seed=3)                    # a new Surrogate re-seeds the engine: the same draws again
    assert_reduces(as_numpy(s.sweep(x, probes=nodes)), F, nodes)


def test_ragged_last_batch_equals_split_calls():
    s, x, _ = surrogate("img", "f32", seed=11)
    whole = s.sweep(x, probes=[5, 5, 519])                       # 6 conditions at batch 4: 4 + 2
    assert whole.probes.shape == (6, 12, 3) and whole.node_max.is_contiguous() and whole.n_min.is_contiguous()
    s, x, _ = surrogate("img", "f32", seed=11)
    first, second = s.sweep(x[:4], probes=[5, 5, 519]), s.sweep(torch.from_numpy(x[4:]).cuda(), probes=[5, 5, 519])
    parts = SweepResult(**{k: torch.cat([getattr(first, k), getattr(second, k)]) for k in SweepResult.FIELDS})
    same_result(whole, parts)
    s, x, _ = surrogate("img", "f32", seed=11)
    bare = s.sweep(x)
    assert bare.probes is None
    same_result(bare, SweepResult(**dict({k: getattr(whole, k) for k in SweepResult.FIELDS}, probes=None)))
    with pytest.raises(ValueError, match=r"probes\[1\] = 520 is outside"):
        s.sweep(x, probes=[0, 520])
    with pytest.raises(ValueError, match="mode must be"):
        s.sweep(x, mode="mean")


def test_sampling_mode_reduces_what_predict_samples():
    nodes = probes_for(520)
    s, x, _ = surrogate("mlp", "f32", seed=21)
    F = s.predict(x, mode="random").cpu().numpy()
    s, x, _ = surrogate("mlp", "f32", seed=21)
    got = s.sweep(x, probes=nodes, mode="random")
    assert_reduces(as_numpy(got), F, nodes)
    s, x, _ = surrogate("mlp", "f32", seed=21)
    assert not torch.equal(s.sweep(x, mode="fix").node_max, got.node_max)
