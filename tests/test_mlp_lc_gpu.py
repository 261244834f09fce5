"""The parametric (CSV) latent conditioner on the MI355X: the fused dense-layer operators (csrc/mlp.hip) against a float64
CPU computation, bitwise replay, parity with the reference model (tests/golden/mlp_lc_small.npz, mlp_lc_preset.npz) and its
training loop (loop_mlp_lc.npz) recorded by tests/golden/gen_mlp_lc_fixtures.py, the fused parameter path at CSV widths that
are not multiples of 4, and the `csv` branch of SimulGen-VAE.py (reader, scaler, model, loop, evaluator) on synthetic data.

Stated tolerances (fp32 kernels; the measured value is in each assertion's message): see TOL."""
import os
import re

import numpy as np
import pytest
import torch

import simulgen_vae_amd
from simulgen_vae_amd import ops
from simulgen_vae_amd.init import init_state, lc_csv_synthetic, lc_init_state, synthetic_samples
from tests.gpu_common import G1, GOLD, make_cfg
from tests.mlp_lc_torch import dense_reference, sample_positions

simulgen_vae_amd.install_reference_api()
from modules import latent_conditioner as L  # noqa: E402
from modules import utils as U  # noqa: E402
from modules.VAE_network import VAE  # noqa: E402
from modules.data_preprocess import latent_conditioner_scaler  # noqa: E402
from modules.latent_conditioner_model_parametric import LatentConditioner, dropout_sites, param_spec  # noqa: E402
from modules.reconstruction_evaluator import ReconstructionEvaluator  # noqa: E402

pytestmark = pytest.mark.gpu
# op: max |error| / max |reference| of outputs (fwd) and gradients (grad) against float64; golden: outputs, gradients
# (per tensor, relative to its max), total norm, parameters after one clipped AdamW step; loop: as tests/test_lc_loop_gpu.py
TOL = dict(fwd=1e-5, grad=1e-4, out=1e-5, norm=1e-4, param=3e-4, loss=1e-4, loop_norm=1e-3, epoch=5e-4, delta=3e-2)


def _err(got, want):
    got = np.asarray(got.detach().cpu() if torch.is_tensor(got) else got, np.float64)
    want = np.asarray(want.detach().cpu() if torch.is_tensor(want) else want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-30))


# ---- operators ---------------------------------------------------------------------------------------------------------
VARIANTS = [("plain", 7, 37, True), ("skip", 75, 24, False), ("resid", 37, 37, True), ("fp", 146, 75, True), ("tanh", 37, 7, False)]


@pytest.mark.parametrize("B", [1, 5, 64, 257])
@pytest.mark.parametrize("variant,K,O,use_mask", VARIANTS)
def test_dense_layer_forward_backward_matches_float64(B, variant, K, O, use_mask):
    gen = torch.Generator().manual_seed(1000 * B + K)
    r = lambda *s, scale=1.0, off=0.0: (off + scale * torch.randn(*s, generator=gen, dtype=torch.float64)).requires_grad_(True)
    x, W, b = r(B, K), r(O, K, scale=K ** -0.5), r(O, scale=0.1)
    g, beta = r(O, scale=0.1, off=1.0), r(O, scale=0.1)
    leaves = dict(x=x, W=W, b=b, g=g, beta=beta)
    skip = post = mask = None
    p = 0.3
    if variant in ("skip", "fp"):
        Ws, bs, gs, betas = r(O, K, scale=K ** -0.5), r(O, scale=0.1), r(O, scale=0.1, off=1.0), r(O, scale=0.1)
        skip = (x, Ws, bs, gs, betas)
        leaves.update(Ws=Ws, bs=bs, gs=gs, betas=betas)
    if variant == "fp":
        gc, bc = r(O, scale=0.1, off=1.0), r(O, scale=0.1)
        post = (gc, bc)
        leaves.update(gc=gc, bc=bc)
    if use_mask:
        mask = (torch.rand(B, O, generator=gen) >= p).double()
    y = dense_reference(x, W, b, g, beta, mask=mask, p=p, tanh=variant == "tanh", skip=skip, resid=x if variant == "resid" else None, post=post)
    dy = torch.randn(B, O, generator=gen, dtype=torch.float64)
    (y * dy).sum().backward()
    c = lambda t: t.detach().float().cuda().contiguous()
    dev = {k: c(v) for k, v in leaves.items()}
    grads = {k: torch.empty_like(v) for k, v in dev.items()}
    if variant == "tanh":
        z, = ops.mlp_gemm_fwd([dict(x=dev["x"], W=dev["W"], bias=dev["b"])], B, tanh_out=True)
        out = z
        ops.mlp_gemm_bwd([dict(dz=c(dy), y_tanh=z, x=dev["x"], W=dev["W"], dx=grads["x"], dW=grads["W"], db=grads["b"])], B, dx_sum=True)
        checked = ("x", "W", "b")
    else:
        probs = [dict(x=dev["x"], W=dev["W"], bias=dev["b"])]
        if skip is not None:
            probs.append(dict(x=dev["x"], W=dev["Ws"], bias=dev["bs"]))
        zs = ops.mlp_gemm_fwd(probs, B)
        row = dict(za=zs[0], ga=dev["g"], ba=dev["beta"], gelu=True)
        if skip is not None:
            row.update(zb=zs[1], gb=dev["gs"], bb=dev["betas"])
        if variant == "resid":
            row["r"] = dev["x"]
        if post is not None:
            row.update(gc=dev["gc"], bc=dev["bc"])
        if mask is not None:
            row.update(mask=c(mask), mask_thr=0.5, mask_scale=1.0 / (1.0 - p))
        (out, row["stats"]), = ops.mlp_rows_fwd([row], B)
        rb, = ops.mlp_rows_bwd([dict(row, dout=c(dy), need_dr=variant == "resid")], B)
        part = rb["part"]
        pb = [dict(dz=rb["dza"], x=dev["x"], W=dev["W"], dx=grads["x"], dW=grads["W"], db=grads["b"])]
        sums = [(part[0], grads["g"]), (part[1], grads["beta"])]
        if skip is not None:
            pb.append(dict(dz=rb["dzb"], x=dev["x"], W=dev["Ws"], dW=grads["Ws"], db=grads["bs"]))
            sums += [(part[2], grads["gs"]), (part[1], grads["betas"])]
        if post is not None:
            sums += [(part[3], grads["gc"]), (part[4], grads["bc"])]
        ops.mlp_gemm_bwd(pb, B, dx_sum=True, dx_addend=rb["dr"], colsums=sums)
        checked = tuple(leaves)
    torch.cuda.synchronize()
    e = _err(out, y)
    assert e <= TOL["fwd"], f"forward: {e:.2e}"
    for k in checked:
        e = _err(grads[k], leaves[k].grad)
        assert e <= TOL["grad"], f"d{k}: {e:.2e}"


def test_bad_arguments_raise_with_message():
    x = torch.zeros(4, 8, device="cuda")
    with pytest.raises(ops.SgvError, match="sgv_op_mlp_gemm_fwd"):
        ops.mlp_gemm_fwd([dict(x=x, W=torch.zeros(0, 8, device="cuda"))], 4)
    with pytest.raises(ops.SgvError, match="sgv_op_mlp_rows"):
        ops.mlp_rows_fwd([dict(za=x, ga=None, ba=None)], 4)
    with pytest.raises(ops.SgvError, match="dx_addend needs dx_sum"):
        ops.mlp_gemm_bwd([dict(dz=x, x=x, W=torch.zeros(8, 8, device="cuda"), dW=torch.empty(8, 8, device="cuda"))], 4, dx_addend=x)


# ---- the model -----------------------------------------------------------------------------------------------------------
def _meta(g):
    latent_end, latent, size2, input_shape, B = (int(v) for v in g["meta"][:5])
    return [int(v) for v in g["filters"]], latent_end, input_shape, latent, size2, B


def _state(filters, latent_end, input_shape, latent, size2, seed):
    st = lc_init_state(dict(param_spec(filters, latent_end, input_shape, latent, size2)), seed)
    return {k: torch.from_numpy(v) for k, v in st.items()}


def _from_fixture(g):
    filters, latent_end, input_shape, latent, size2, B = _meta(g)
    m = LatentConditioner(filters, latent_end, input_shape, latent, size2, dropout_rate=0.3)
    m.load_state_dict(_state(filters, latent_end, input_shape, latent, size2, int(g["meta"][5])))
    return m


def _check_tensor(g, prefix, name, got, tol):
    got = got.detach().double().cpu().numpy().reshape(-1)
    if prefix + name in g:
        e = _err(got, g[prefix + name].reshape(-1))
    else:
        want = g[prefix + "samp." + name]
        e = max(_err(got[sample_positions(name, got.size)], want),
                abs(np.linalg.norm(got) - float(g[prefix + "norm." + name])) / float(g[prefix + "norm." + name]))
    assert e <= tol, f"{prefix}{name}: {e:.2e}"
    return e


@pytest.mark.parametrize("fixture", ["mlp_lc_small", "mlp_lc_preset"])
def test_single_step_matches_reference(fixture):
    g = np.load(os.path.join(GOLD, fixture + ".npz"))
    m = _from_fixture(g)
    x, y1, y2 = (torch.from_numpy(g[k]).cuda() for k in ("x", "y1", "y2"))
    m.eval()
    e1, e2 = m(x)
    errs = dict(eval_main=_err(e1, g["eval_main"]), eval_xs=_err(e2, g["eval_xs"]))
    m.train()
    masks = [torch.from_numpy(g[f"mask{i}"].astype(np.float32)) for i in range(int(g["n_masks"][0]))]
    p1, p2 = m(x, masks)
    errs.update(train_main=_err(p1, g["train_main"]), train_xs=_err(p2, g["train_xs"]))
    assert max(errs.values()) <= TOL["out"], errs
    loss, A, Bv = m.loss_backward(x, y1, y2, preds=(p1, p2))
    e = _err([loss, A, Bv], g["loss"])
    assert e <= TOL["out"], f"loss terms {e:.2e}"
    worst = max(_check_tensor(g, "g.", n, m.grads[n], TOL["grad"]) for n, _ in m.named_parameters())
    opt = L.LCOptimizer(m, 1e-3, 1e-4)
    tn = opt.clip_and_step(max_norm=10.0, lr=1e-3)
    e = abs(tn - float(g["total_norm"][0])) / float(g["total_norm"][0])
    assert e <= TOL["norm"], f"total norm {tn} vs {float(g['total_norm'][0])}: {e:.2e}"
    pw = max(_check_tensor(g, "s1.", n, t, TOL["param"]) for n, t in m.state_dict().items())
    print(fixture, errs, "worst gradient", worst, "norm", e, "worst parameter", pw)


def test_training_step_replays_bitwise():
    filters, B, input_shape = [32, 64, 128, 256, 512, 1024], 64, 16
    m = LatentConditioner(filters, 32, input_shape, 8, 3)
    gen = torch.Generator().manual_seed(5)
    x = torch.rand(B, input_shape, generator=gen).cuda()
    y1, y2 = torch.randn(B, 32, generator=gen).cuda(), torch.randn(B, 3, 8, generator=gen).cuda()
    masks = [(torch.rand(B, w, generator=gen) >= p).float() for _, w, p in dropout_sites(filters, 32, input_shape, 0.3)]
    runs = []
    for _ in range(2):
        p1, p2 = m(x, masks)
        m.loss_backward(x, y1, y2, preds=(p1, p2))
        runs.append((p1.clone(), p2.clone(), m._garena.clone()))
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    assert float(runs[0][2].abs().sum()) > 0


@pytest.mark.parametrize("input_shape", [7, 13, 600, 603])
def test_fused_parameter_path_at_any_csv_width(input_shape):
    m = LatentConditioner([32, 64, 64], 32, input_shape, 8, 3)
    assert m._fused() and len(m.pset.entries) == len(param_spec([32, 64, 64], 32, input_shape, 8, 3))
    for e in m.pset.entries:
        assert e["p"].numel() % 4 == 0 and e["p"].data_ptr() % 16 == 0 and e["g"].data_ptr() % 16 == 0
    B = 5
    x, y1, y2 = torch.rand(B, input_shape).cuda(), torch.rand(B, 32).cuda(), torch.rand(B, 3, 8).cuda()
    before = m._parena.clone()
    m.loss_backward(x, y1, y2)
    tn = L.LCOptimizer(m, 1e-3, 1e-4).clip_and_step(10.0, lr=1e-3)
    assert np.isfinite(tn) and tn > 0
    pad = torch.ones_like(m._parena, dtype=torch.bool)
    for _, shape, off, _ in m._slots:
        pad[off:off + int(np.prod(shape))] = False
    assert bool(pad.any()) == (input_shape % 4 != 0)
    assert torch.equal(m._parena[pad], torch.zeros_like(m._parena[pad]))      # padding stays zero through AdamW
    assert not torch.equal(m._parena[~pad], before[~pad])


# ---- the training loop ------------------------------------------------------------------------------------------------------
def sample_positions64(name, numel, n=64):
    seed = int.from_bytes(name.encode()[-8:].rjust(8, b"\0"), "little") % (2 ** 31)
    rng = np.random.Generator(np.random.Philox(key=[977, seed]))
    return rng.integers(0, numel, size=min(n, numel))


def test_plain_loop_matches_reference_run(tmp_path, monkeypatch, capsys):
    g = np.load(os.path.join(GOLD, "loop_mlp_lc.npz"))
    latent_end, latent, size2, input_shape, B, p_train, p_val, epochs, state_seed, data_seed = (int(v) for v in g["meta"])
    filters = [int(v) for v in g["filters"]]
    lc = LatentConditioner(filters, latent_end, input_shape, latent, size2)
    state = _state(filters, latent_end, input_shape, latent, size2, state_seed)
    monkeypatch.setattr(LatentConditioner, "apply", lambda self, fn: self.load_state_dict(state))
    real_masks = LatentConditioner._masks

    def keep_all(self, n, dropout_masks):
        sites = [w for _, w, p in dropout_sites(self.latent_conditioner_filter, self.latent_dim_end, self.input_shape, self.dropout_rate) if p > 0]
        return real_masks(self, n, [torch.ones(n, w) for w in sites] if self.training else None)
    monkeypatch.setattr(LatentConditioner, "_masks", keep_all)
    x, y1, y2 = lc_csv_synthetic(data_seed, p_train + p_val, input_shape, latent_end, size2, latent)
    batches = lambda lo, hi: [tuple(torch.from_numpy(a[i:min(i + B, hi)]) for a in (x, y1, y2)) for i in range(lo, hi, B)]
    rec = {"mse": [], "norm": []}
    real_mse, real_clip = ops.mse, L.LCOptimizer.clip_and_step

    def mse(*a, **k):
        out = real_mse(*a, **k)
        rec["mse"].append(float(out[0]))
        return out

    def clip(self, *a, **k):
        n = real_clip(self, *a, **k)
        rec["norm"].append(float(n))
        return n
    monkeypatch.setattr(ops, "mse", mse)
    monkeypatch.setattr(L.LCOptimizer, "clip_and_step", clip)
    monkeypatch.chdir(tmp_path)

    class NoAugment:
        def random(self):
            return 0.99
    L.train_latent_conditioner(epochs, batches(0, p_train), batches(p_train, p_train + p_val), lc, float(g["lr0"]), weight_decay=float(g["wd"]),
                               is_image_data=False, rng=NoAugment())
    out = capsys.readouterr().out
    rows = np.array([[float(v) for v in m.groups()] for m in re.finditer(
        r"Train: ([0-9.E+-]+) \(y1:([0-9.E+-]+), y2:([0-9.E+-]+)\), Val: ([0-9.E+-]+) \(y1:([0-9.E+-]+), y2:([0-9.E+-]+)\), LR: ([0-9.E+-]+)", out)])
    print("mse", np.array(rec["mse"]), "\nref", g["mse"], "\nnorms", rec["norm"], g["grad_norms"], "\n", rows, "\n", g["epochs"])
    np.testing.assert_allclose(rec["mse"], g["mse"], rtol=TOL["loss"])
    np.testing.assert_allclose(rec["norm"], g["grad_norms"], rtol=TOL["loop_norm"])
    np.testing.assert_allclose(rows, g["epochs"], rtol=TOL["epoch"])
    worst = 0.0
    for k, v in lc.state_dict().items():
        a = v.double().numpy().reshape(-1)
        pos = sample_positions64(k, a.size)
        init = state[k].double().numpy().reshape(-1)[pos]
        want, got = g["fsamp." + k] - init, a[pos] - init
        d = np.mean(np.abs(got - want)) / max(np.mean(np.abs(want)), 1e-30)
        assert d < TOL["delta"], (k, d)
        assert abs(np.linalg.norm(a) - float(g["fnorm." + k])) <= 1e-4 * float(g["fnorm." + k]) + 1e-9, k
        worst = max(worst, d)
    print("worst state-change deviation", worst)
    assert os.path.exists("checkpoints/latent_conditioner.pth") and os.path.exists("model_save/LatentConditioner")


# ---- the csv branch of SimulGen-VAE.py -----------------------------------------------------------------------------------------
def test_csv_branch_reader_model_loop_and_evaluator(tmp_path, monkeypatch, capsys):
    """SimulGen-VAE.py:369-372,421-423,466-472 and the evaluation after it, on synthetic data: a headerless CSV of 13
    simulation parameters per case, latents of a G1-sized VAE, 2 epochs, then ReconstructionEvaluator on one sample."""
    import pickle
    monkeypatch.chdir(tmp_path)
    os.makedirs("model_save", exist_ok=True)
    os.makedirs("checkpoints", exist_ok=True)
    cfg = make_cfg(G1)
    P, n_param, size2 = 12, 13, len(cfg.num_filter_dec) - 1
    rng = np.random.default_rng(11)
    np.savetxt("params.csv", rng.uniform(0.0, 5.0, (P, n_param)), delimiter=",")
    raw = L.read_latent_conditioner_dataset("params.csv", ".csv")
    assert raw.shape == (P, n_param)
    x, _ = latent_conditioner_scaler(raw, "./model_save/latent_conditioner_input_scaler.pkl")
    y1, sc1 = latent_conditioner_scaler(rng.standard_normal((P, cfg.latent_dim)), "./model_save/latent_vectors_scaler.pkl")
    y2, sc2 = latent_conditioner_scaler(rng.standard_normal((P, size2, cfg.hierarchical_dim)), "./model_save/xs_scaler.pkl")
    ds = U.LatentConditionerDataset(x.astype(np.float32), y1.astype(np.float32), y2.astype(np.float32))
    train = torch.utils.data.DataLoader(torch.utils.data.Subset(ds, range(8)), batch_size=4, shuffle=True)
    val = torch.utils.data.DataLoader(torch.utils.data.Subset(ds, range(8, P)), batch_size=4, shuffle=False)
    lc = LatentConditioner([32, 64, 64], cfg.latent_dim, n_param, cfg.hierarchical_dim, size2, dropout_rate=0.3)
    torch.manual_seed(2)
    ret = L.train_latent_conditioner(2, train, val, lc, 1e-3, weight_decay=1e-4, is_image_data=False)
    assert np.isfinite(ret) and ret > 0
    with open("model_save/LatentConditioner", "rb") as f:
        back = pickle.load(f)
    for k, v in lc.state_dict().items():
        assert torch.equal(back.state_dict()[k], v), k
    vae = VAE(cfg.latent_dim, cfg.hierarchical_dim, cfg.num_filter_enc, cfg.num_filter_dec, cfg.num_node, cfg.num_time,
              lossfun="MSE", batch_size=1, small=True, compute_dtype="f32")
    vae.load_state_dict({k: torch.from_numpy(v) for k, v in init_state(cfg, 7).items()})
    vae.eval()
    original = synthetic_samples(5, range(P), cfg.num_node, cfg.num_time)
    ev = ReconstructionEvaluator(vae, "cuda", cfg.num_time, debug_mode=1)
    capsys.readouterr()
    ev.evaluate_reconstruction_comparison(back, torch.utils.data.Subset(ds, [0]), original[:1], sc1, sc2)
    out = capsys.readouterr().out
    assert "Evaluating 1 samples..." in out and "Sample 0 Reconstruction Stats:" in out
    assert os.path.getsize("checkpoints/reconstruction_dual_view_0.png") > 10000
    p1, p2 = back(ds[0][0][None])
    assert p1.shape == (1, cfg.latent_dim) and p2.shape == (1, size2, cfg.hierarchical_dim)
    assert float(p1.abs().max()) <= 1.0 and bool(torch.isfinite(p2).all())
