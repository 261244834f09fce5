"""What the integration tests of the surrogate layer share: tests/test_{predict,sweep,score,ensemble,sobol,distribution,regression,
project,temporal,gram,exceedance,cycles}_gpu.py take their engines, latents, scalers and Surrogates from here, and the two checks every
output pass repeats (what it leaves behind in the engine, and that training does not notice it).  The caches live in this module
alone, imported as tests.surrogate_common, so a session builds each engine and each model once.  `bits` comes from
tests.recon_kernel_common, a second module object beside the `recon_kernel_common` of the kernel tests: nothing else is taken from
it, so its memo of cases stays under that other name."""
import types

import numpy as np
import pytest
import torch

import simulgen_vae_amd  # noqa: F401
from simulgen_vae_amd import engine as E
from simulgen_vae_amd.init import init_state, lc_csv_synthetic, lc_init_state, lc_synthetic, synthetic_samples
from simulgen_vae_amd.modules.VAE_network import VAE
from simulgen_vae_amd.modules.latent_conditioner_model_cnn import LatentConditionerImg
from simulgen_vae_amd.modules.latent_conditioner_model_parametric import LatentConditioner
from simulgen_vae_amd.predict import Surrogate
from tests.gpu_common import G0, G1, GOLD, make_cfg
from tests.recon_kernel_common import bits  # noqa: F401  (the one copy, handed on to the test modules)

MAXB = 4

_ENGINES = {}


def engine(name, dtype):
    """one engine per (configuration, dtype) for the read-only tests"""
    if (name, dtype) not in _ENGINES:
        cfg = make_cfg({"G0": G0, "G1": G1}[name])
        eng = E.Engine(cfg, max_batch=MAXB, compute_dtype=dtype)
        eng.load_state(init_state(cfg, 7))
        _ENGINES[(name, dtype)] = (cfg, eng)
    return _ENGINES[(name, dtype)]


def latents(cfg, B, seed=3):
    rng = np.random.default_rng(seed)
    z = torch.from_numpy(rng.standard_normal((B, cfg.latent_dim)).astype(np.float32)).cuda()
    xs = [torch.from_numpy((0.5 * rng.standard_normal((B, cfg.hierarchical_dim))).astype(np.float32)).cuda() for _ in range(len(cfg.num_filter_enc) - 1)]
    eps = [torch.zeros(B, cfg.latent_dim).cuda()] + [torch.from_numpy(rng.standard_normal((B, c, cfg.num_time)).astype(np.float32)).cuda()
                                                     for c in cfg.num_filter_dec[1:-1]]
    return z, xs, eps


def node_scaler(N, seed=5):
    rng = np.random.default_rng(seed)
    scale = np.exp(rng.uniform(np.log(1e-3), np.log(50.0), N)).astype(np.float32)
    mn = (rng.standard_normal(N) * np.where(rng.random(N) < 0.5, 1.0, 30.0)).astype(np.float32)
    return scale, mn


def signed_scaler(N):
    """node_scaler with about a quarter of the scales negative"""
    scale, mn = node_scaler(N)
    flip = np.random.default_rng(17).random(N) < 0.25
    return np.where(flip, -scale, scale).astype(np.float32), mn


def _train_step(eng, cfg, k):
    x = synthetic_samples(20251003, range(3 * k, 3 * k + 3), cfg.num_node, cfg.num_time)
    rng = np.random.default_rng(100 + k)
    eps = [torch.from_numpy(rng.standard_normal((3, cfg.latent_dim)).astype(np.float32)).cuda()] + [
        torch.from_numpy(rng.standard_normal((3, c, cfg.num_time)).astype(np.float32)).cuda() for c in cfg.num_filter_dec[1:-1]]
    eng.set_input(torch.from_numpy(x).cuda())
    eng.set_eps(eps)
    eng.forward(train=True)
    eng.backward_step(1e6, 1e-4, 1e-3)


def _fresh(cfg, dtype):
    eng = E.Engine(cfg, max_batch=MAXB, compute_dtype=dtype)
    eng.load_state(init_state(cfg, 7))
    return eng


def _same_state(a, b):
    sa, sb = a.state_dict(), b.state_dict()
    bad = [k for k in sa if not np.array_equal(sa[k], sb[k])]
    for k in [k for k in sa if k.endswith("weight_orig")][::7]:          # and the optimizer's moments of a few weights
        ma, mb = a.adam_state(k), b.adam_state(k)
        if not (np.array_equal(ma[0], mb[0]) and np.array_equal(ma[1], mb[1])):
            bad.append("adam." + k)
    return bad


def no_forward_after(eng, cfg, run, calls, B=2):
    """What an output pass leaves behind in `eng`: the forward of a decode is readable, after run(z, xs, scale, mn, before) -- the
    call under test on B latents with their noise set, the signed scaler and the field generate writes for them -- every one of
    `calls` raises SGV_ERR_STATE, and generate still writes the same bits."""
    z, xs, eps = latents(cfg, B)
    scale, mn = (torch.from_numpy(a).cuda() for a in signed_scaler(cfg.num_node))
    eng.set_eps(eps)
    before = eng.generate(z, xs, scale, mn, fix=True).clone()
    eng.set_eps(eps)
    eng.decode(z, xs, fix=True)
    eng.xhat()                                                   # readable after decode ...
    eng.set_eps(eps)
    run(z, xs, scale, mn, before)
    for call in calls:
        with pytest.raises(E.SgvError, match=r"\(-3\)"):          # ... SGV_ERR_STATE after the call under test
            call()
    eng.set_eps(eps)
    assert torch.equal(eng.generate(z, xs, scale, mn, fix=True), before)


def training_unaffected(dtype, run, draw_moves, prepare=None, B=2):
    """Two fresh G0 engines take the same two training steps; in front of each, one of them makes the call under test,
    run(eng, z, xs, scale, mn, i) for i = 0, 1, on B latents and the signed scaler, after prepare(eng) if given.  Parameters and
    optimizer moments stay equal; the noise position has moved (draw_moves) or has not."""
    cfg = make_cfg(G0)
    scale, mn = (torch.from_numpy(a).cuda() for a in signed_scaler(cfg.num_node))
    z, xs, eps = latents(cfg, B)
    a, b = _fresh(cfg, dtype), _fresh(cfg, dtype)
    try:
        if prepare is not None:
            prepare(a)
        a.set_eps(eps)
        run(a, z, xs, scale, mn, 0)
        _train_step(a, cfg, 0)
        _train_step(b, cfg, 0)
        assert _same_state(a, b) == []
        a.set_eps(eps[:1])                                        # sites 1.. drawn by the engine
        run(a, z, xs, scale, mn, 1)
        _train_step(a, cfg, 1)
        _train_step(b, cfg, 1)
        assert _same_state(a, b) == []
        if draw_moves:                                            # drawn per call: only the draw counter moves
            assert a.train_state()["draw"] > b.train_state()["draw"]
        else:                                                     # drawn by member index: the draw position stays
            assert a.train_state()["draw"] == b.train_state()["draw"]
    finally:
        a.close(); b.close()


def state_as_numpy(res, names):
    """the tensors `names` of a running result, or of the engine's state dict, that are not None, as numpy arrays"""
    get = res.get if isinstance(res, dict) else (lambda k: getattr(res, k))
    return {k: get(k).cpu().numpy() for k in names if get(k) is not None}


def same_result(a, b):
    """two results of one class agree in every one of its FIELDS: counts equal, both None, or tensors of one dtype and shape
    that are equal and have the same bits"""
    assert type(a) is type(b)
    for k in a.FIELDS:
        va, vb = getattr(a, k), getattr(b, k)
        if torch.is_tensor(va) and torch.is_tensor(vb):
            assert va.dtype == vb.dtype and va.shape == vb.shape and torch.equal(va, vb), k
            as_bits = torch.int64 if va.element_size() == 8 else torch.int32
            assert torch.equal(va.contiguous().view(as_bits), vb.contiguous().view(as_bits)), k
        else:
            assert not torch.is_tensor(va) and not torch.is_tensor(vb) and va == vb, k


# ---- Surrogates on the models of the reference's run ----
def _fixture():
    return np.load(f"{GOLD}/predict_small.npz")


_SUR = {}


def surrogate(kind, dtype, batch=MAXB, seed=0):
    """(Surrogate, conditions [6, F]) on the fixture's models; VAE and conditioner are built once per (kind, dtype)"""
    g = _fixture()
    P, data_seed, _, img, img_seed, n_param, mlp_seed, vae_seed = (int(v) for v in g["meta"])
    if (kind, dtype) not in _SUR:
        cfg = make_cfg(G1)
        vae = VAE(cfg.latent_dim, cfg.hierarchical_dim, cfg.num_filter_enc, cfg.num_filter_dec, cfg.num_node, cfg.num_time, lossfun="MSE",
                  batch_size=MAXB, small=True, compute_dtype=dtype)
        vae.load_state_dict({k: torch.from_numpy(v) for k, v in init_state(cfg, vae_seed).items()})
        vae.eval()
        if kind == "img":
            lc = LatentConditionerImg([int(v) for v in g["img_filters"]], cfg.latent_dim, (1, img, img), cfg.hierarchical_dim, 3, (img, img),
                                      dropout_rate=0.0, use_attention=True, compute_dtype=dtype)
            seed_lc = img_seed
            x = lc_synthetic(data_seed, P, img * img, cfg.latent_dim, 3, cfg.hierarchical_dim)[0]
        else:
            lc = LatentConditioner([int(v) for v in g["mlp_filters"]], cfg.latent_dim, n_param, cfg.hierarchical_dim, 3, dropout_rate=0.3)
            seed_lc = mlp_seed
            x = lc_csv_synthetic(data_seed, P, n_param, cfg.latent_dim, 3, cfg.hierarchical_dim)[0]
        st = lc_init_state({k: tuple(v.shape) for k, v in lc.state_dict().items()}, seed_lc)
        lc.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in st.items()})
        _SUR[(kind, dtype)] = (vae, lc, x)
    vae, lc, x = _SUR[(kind, dtype)]
    sc = [types.SimpleNamespace(scale_=g[n + "_scale"], min_=g[n + "_min"]) for n in ("latent", "xs", "data")]
    return Surrogate(vae, lc, sc[0], sc[1], sc[2], batch=batch, seed=seed), x, g
