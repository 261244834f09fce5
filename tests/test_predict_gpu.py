"""Surrogate prediction on the GPU: Engine.generate (sgv_generate) against the existing decode -> xhat path, what it leaves
behind in the engine, and simulgen_vae_amd.predict.Surrogate against a run of the reference's own models
(tests/golden/predict_small.npz <- tests/golden/gen_predict_fixtures.py).

Bounds:
  * generate vs decode(fix) + xhat() of the same fp32 engine, descaled in float64 on the host: the bound of
    tests/test_generate_kernel_gpu.py, (ELT32 * max|x_hat| + 4 * 2^-24 * (|x_hat| + |min_n|)) / |scale_n|;
  * Surrogate.predict vs the reference, fp32 engine: the bound tests/test_e2e_gpu.py asserts for the evaluator's arrays, 3e-4 of the
    scaled field's range, per node 3e-4 / |scale_n|;
  * bf16 engine vs the reference: 3 x the worst value measured on an MI355X (the project's rule for bf16 bounds, DESIGN.md
    section 2), in scaled units (error * |scale_n|); the measured values stand next to BF16_BOUND;
  * bf16 engine, new path vs old path: no tolerance -- the error of generate() against the float64 descale of the fp32 engine's x_hat
    must be smaller than the error of bf16 xhat() descaled on the host, on the maximum and on the mean."""
import types

import numpy as np
import pytest
import torch

import simulgen_vae_amd  # noqa: F401
from simulgen_vae_amd import engine as E
from simulgen_vae_amd.init import lc_synthetic
from simulgen_vae_amd.modules.latent_conditioner_model_cnn import LatentConditionerImg
from simulgen_vae_amd.predict import Surrogate
from tests.gpu_common import G0, make_cfg
from tests.surrogate_common import MAXB, _fixture, _fresh, _same_state, _train_step, engine, latents, node_scaler, surrogate

pytestmark = pytest.mark.gpu

ELT32 = 2e-5
# worst |error| * |scale_n| of Surrogate.predict on bf16 models (VAE and, for "img", the conditioner) against the fixture, measured on
# an MI355X: image conditioner 1.978e-1, parametric 3.751e-2 (the fp32 models: 1.65e-5 and 7.5e-6 against the bound of 3e-4)
BF16_BOUND = {"img": 3 * 1.978e-1, "mlp": 3 * 3.751e-2}
# the mean over the field of the same quantity, measured: image conditioner 1.193e-2, parametric 3.947e-3; asserted at 3 x as well (the
# maximum's bound is wide against the scaled range of 1.4: the mean is what notices a decoder that is wrong everywhere a little)
BF16_MEAN_BOUND = {"img": 3 * 1.193e-2, "mlp": 3 * 3.947e-3}

def descale64(xhat_bnt, scale, mn, layout):
    """float64 (x_hat - min) / scale of a reference-layout [B, N, T] array, in the layout asked for"""
    r = (np.asarray(xhat_bnt, np.float64) - mn.astype(np.float64)[None, :, None]) / scale.astype(np.float64)[None, :, None]
    return r.transpose(0, 2, 1) if layout == "TN" else r


def old_path(eng, z, xs, eps):
    eng.set_eps(eps)
    eng.decode(z, xs, fix=True)
    return eng.xhat().cpu().numpy()


def new_path(eng, z, xs, eps, scale, mn, layout):
    eng.set_eps(eps)
    return eng.generate(z, xs, torch.from_numpy(scale).cuda(), torch.from_numpy(mn).cuda(), layout=layout, fix=True).cpu().numpy()


@pytest.mark.parametrize("layout", ["TN", "NT"])
@pytest.mark.parametrize("B", [1, 3, MAXB])
@pytest.mark.parametrize("name", ["G0", "G1"])
def test_generate_matches_decode_and_host_descale(name, B, layout):
    cfg, eng = engine(name, "f32")
    z, xs, eps = latents(cfg, B)
    scale, mn = node_scaler(cfg.num_node)
    xhat = old_path(eng, z, xs, eps)
    got = new_path(eng, z, xs, eps, scale, mn, layout)
    assert got.shape == ((B, cfg.num_time, cfg.num_node) if layout == "TN" else (B, cfg.num_node, cfg.num_time)) and got.dtype == np.float32
    ref = descale64(xhat, scale, mn, layout)
    bshape = (1, 1, -1) if layout == "TN" else (1, -1, 1)
    ax = descale64(np.abs(xhat), np.ones_like(scale), np.zeros_like(mn), layout)
    tol = (ELT32 * np.abs(xhat).max() + 4 * 2.0 ** -24 * (ax + np.abs(mn.astype(np.float64)).reshape(bshape))) / np.abs(scale.astype(np.float64)).reshape(bshape)
    err = np.abs(got - ref)
    print(f"  {name} B {B} {layout}: worst err/tol {np.max(err / tol):.3f}")
    assert np.all(err <= tol), f"worst err/tol {np.max(err / tol):.3f}"


@pytest.mark.parametrize("name", ["G0", "G1"])
def test_bf16_generate_is_closer_to_fp32_than_the_old_path(name):
    cfg, e32 = engine(name, "f32")
    _, e16 = engine(name, "bf16")
    z, xs, eps = latents(cfg, MAXB)
    scale, mn = node_scaler(cfg.num_node)
    ref = descale64(old_path(e32, z, xs, eps), scale, mn, "TN")
    old = descale64(old_path(e16, z, xs, eps), scale, mn, "TN")            # bf16 x_hat, descaled on the host in float64
    new = new_path(e16, z, xs, eps, scale, mn, "TN")
    e_old, e_new = np.abs(old - ref), np.abs(new - ref)
    s = np.abs(scale.astype(np.float64))[None, None, :]
    print(f"  {name}: error against the fp32 engine, physical units: old path max {e_old.max():.4e} mean {e_old.mean():.4e}; "
          f"generate max {e_new.max():.4e} mean {e_new.mean():.4e}")
    print(f"  {name}: the same in scaled units: old path max {(e_old * s).max():.4e} mean {(e_old * s).mean():.4e}; "
          f"generate max {(e_new * s).max():.4e} mean {(e_new * s).mean():.4e}")
    assert e_new.max() < e_old.max() and e_new.mean() < e_old.mean()


def test_no_forward_to_read_after_generate():
    cfg, eng = engine("G0", "f32")
    z, xs, eps = latents(cfg, 2)
    scale, mn = node_scaler(cfg.num_node)
    old_path(eng, z, xs, eps)
    eng.xhat()                                                   # readable after decode ...
    new_path(eng, z, xs, eps, scale, mn, "TN")
    for call in (eng.xhat, lambda: eng.activation("x_hat", (2, cfg.num_node, cfg.num_time)), lambda: eng.backward(1.0, 1.0)):
        with pytest.raises(E.SgvError, match=r"\(-3\)"):          # ... SGV_ERR_STATE after generate
            call()
    # argument errors: SGV_ERR_ARG, and the forward of a decode stays readable (nothing was enqueued)
    old_path(eng, z, xs, eps)
    xs_t, sc_t, mn_t = torch.stack(xs).contiguous(), torch.from_numpy(scale).cuda(), torch.from_numpy(mn).cuda()
    out = torch.empty(2, cfg.num_time, cfg.num_node, device="cuda")
    for args, msg in (((z.data_ptr(), xs_t.data_ptr(), 2, 1, sc_t.data_ptr(), mn_t.data_ptr(), 7, out.data_ptr()), "unknown layout"),
                      ((z.data_ptr(), xs_t.data_ptr(), 2, 1, None, mn_t.data_ptr(), 0, out.data_ptr()), "null argument"),
                      ((z.data_ptr(), xs_t.data_ptr(), 2, 1, sc_t.data_ptr(), mn_t.data_ptr(), 0, None), "null argument"),
                      ((z.data_ptr(), None, 2, 1, sc_t.data_ptr(), mn_t.data_ptr(), 0, out.data_ptr()), "needs xs"),
                      ((z.data_ptr(), xs_t.data_ptr(), MAXB + 1, 1, sc_t.data_ptr(), mn_t.data_ptr(), 0, out.data_ptr()), "batch")):
        assert eng.lib.sgv_generate(eng.h, *args) == -1
        assert msg in eng.lib.sgv_last_error().decode()
    eng.xhat()


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_training_is_unaffected_by_generate(dtype):
    cfg = make_cfg(G0)
    scale, mn = node_scaler(cfg.num_node)
    z, xs, eps = latents(cfg, 2)
    a, b = _fresh(cfg, dtype), _fresh(cfg, dtype)
    try:
        # generate first, then a training step: the state a fresh engine reaches with the same step
        new_path(a, z, xs, eps, scale, mn, "NT")
        _train_step(a, cfg, 0)
        _train_step(b, cfg, 0)
        assert _same_state(a, b) == []
        # generate between two training steps (noise of the training forwards injected: only the draw counter moves)
        new_path(a, z, xs, eps[:1], scale, mn, "TN")                # sites 1.. drawn by the engine
        _train_step(a, cfg, 1)
        _train_step(b, cfg, 1)
        assert _same_state(a, b) == []
        assert a.train_state()["draw"] > b.train_state()["draw"]
    finally:
        a.close(); b.close()


# ---- Surrogate against the reference ----
@pytest.mark.parametrize("kind", ["img", "mlp"])
def test_predict_matches_the_reference_fp32(kind):
    s, x, g = surrogate(kind, "f32")
    got = s.predict(x).cpu().numpy()
    want = g[kind + "_fields"]
    assert got.shape == want.shape == (6, 12, 520) and got.dtype == np.float32
    scaled = np.abs(got.astype(np.float64) - want) * np.abs(g["data_scale"])[None, None, :]
    print(f"  {kind} fp32: worst |error| * |scale_n| {scaled.max():.3e} (bound 3e-4)")
    assert scaled.max() <= 3e-4
    s, x, g = surrogate(kind, "f32")                             # a new Surrogate re-seeds the engine: mode "fix" still adds 1e-10 * noise
    nt = s.predict(x, layout="NT")
    assert torch.equal(nt.transpose(1, 2).cpu(), torch.from_numpy(got))


@pytest.mark.parametrize("kind", ["img", "mlp"])
def test_predict_matches_the_reference_bf16(kind):
    s, x, g = surrogate(kind, "bf16")
    got = s.predict(x).cpu().numpy()
    scaled = np.abs(got.astype(np.float64) - g[kind + "_fields"]) * np.abs(g["data_scale"])[None, None, :]
    print(f"  {kind} bf16: worst |error| * |scale_n| {scaled.max():.3e}, mean {scaled.mean():.3e} (bound {BF16_BOUND[kind]:.2e})")
    assert scaled.max() <= BF16_BOUND[kind]
    assert scaled.mean() <= BF16_MEAN_BOUND[kind]


def test_image_conditions_are_ranged_once_not_per_batch(monkeypatch):
    """predict decides the [-1, 1] -> [0, 1] mapping once for all conditions; the model's forward is told and reads nothing back"""
    seen = []
    real = LatentConditionerImg.forward

    def forward(self, x, dropout_masks=None, remap=None):
        seen.append(remap)
        return real(self, x, dropout_masks, remap)
    monkeypatch.setattr(LatentConditionerImg, "__call__", forward)
    s, x, _ = surrogate("img", "f32", seed=2)
    a = s.predict(x)                                             # U[0, 1): not remapped
    s, x, _ = surrogate("img", "f32", seed=2)
    b = s.predict(torch.from_numpy(2 * x - 1).cuda())            # the same images in [-1, 1]: remapped, in both batches
    assert seen == [False, False, True, True]
    scaled = (a - b).abs().cpu().numpy() * np.abs(_fixture()["data_scale"])[None, None, :]
    assert scaled.max() < 1e-4                                   # (2x - 1 + 1) / 2 is x to a rounding of the image
    # the model's own forward, asked to decide by itself, agrees with what predict told it
    lc = s.conditioner
    y_auto, y_told = lc(torch.from_numpy(2 * x[:2] - 1).cuda()), lc(torch.from_numpy(2 * x[:2] - 1).cuda(), remap=True)
    assert torch.equal(y_auto[0], y_told[0]) and torch.equal(y_auto[1], y_told[1])


def test_from_files_loads_what_the_mirrors_write(tmp_path):
    import pickle
    s, x, g = surrogate("mlp", "f32", seed=9)
    want = s.predict(x)
    d = tmp_path / "model_save"
    d.mkdir()
    torch.save(s.vae, str(d / "SimulGen-VAE"))                   # modules/train.py
    with open(d / "LatentConditioner", "wb") as f:               # modules/latent_conditioner.py
        pickle.dump(s.conditioner, f)
    for fname, n in (("latent_vectors_scaler.pkl", "latent"), ("xs_scaler.pkl", "xs"), ("scaler.pkl", "data")):
        with open(d / fname, "wb") as f:                         # modules/data_preprocess.py
            pickle.dump(types.SimpleNamespace(scale_=g[n + "_scale"], min_=g[n + "_min"]), f)
    loaded = Surrogate.from_files(str(d), batch=MAXB, seed=9)
    assert loaded.vae is not s.vae and loaded.vae.compute_dtype == "f32"
    assert torch.equal(loaded.predict(x), want)
    loaded.vae._engine.close()


@pytest.mark.parametrize("mode", ["fix", "random"])
def test_ragged_last_batch_equals_split_calls(mode):
    s, x, _ = surrogate("img", "f32", seed=11)
    whole = s.predict(x, mode=mode)                              # 6 conditions at batch 4: 4 + 2
    s, x, _ = surrogate("img", "f32", seed=11)                   # re-seeds the engine: the same draws again
    parts = torch.cat([s.predict(x[:4], mode=mode), s.predict(torch.from_numpy(x[4:]).cuda(), mode=mode)])
    assert torch.equal(whole, parts)


@pytest.mark.parametrize("layout", ["TN", "NT"])
def test_predict_to_host_equals_predict(layout):
    x = lc_synthetic(5, 10, 256, 32, 3, 8)[0]                    # P = 10 at batch 4: both buffers are reused, the last batch is ragged
    # the same seed in front of every call: mode "fix" adds 1e-10 * noise, which shows in the last bit where a latent is tiny
    dev = surrogate("img", "f32", seed=4)[0].predict(x, layout=layout).cpu()
    host = surrogate("img", "f32", seed=4)[0].predict_to_host(x, layout=layout)
    assert host.is_pinned() and host.shape == dev.shape == ((10, 12, 520) if layout == "TN" else (10, 520, 12))
    assert torch.equal(host, dev)
    again = torch.full(tuple(dev.shape), float("nan")).pin_memory()
    assert surrogate("img", "f32", seed=4)[0].predict_to_host(torch.from_numpy(x).cuda(), out=again, layout=layout) is again and torch.equal(again, dev)


def test_same_seed_same_samples():
    s, x, _ = surrogate("mlp", "f32", seed=21)
    a = [s.predict(x, mode="random").clone(), s.predict(x[:3], mode="random").clone()]
    s, x, _ = surrogate("mlp", "f32", seed=21)
    b = [s.predict(x, mode="random"), s.predict(x[:3], mode="random")]
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert not torch.equal(a[0][:3], a[1])                       # the second call drew new noise
    s, x, _ = surrogate("mlp", "f32", seed=22)
    assert not torch.equal(s.predict(x, mode="random"), a[0])
