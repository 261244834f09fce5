"""Golden vectors for the parametric (CSV) latent conditioner, recorded from the REFERENCE on CPU (fp32):
modules.latent_conditioner_model_parametric.LatentConditioner and modules.latent_conditioner.train_latent_conditioner,
both imported unmodified.

Run only in the build container (needs the reference checkout):

    python tests/golden/gen_mlp_lc_fixtures.py

Weights come from simulgen_vae_amd.init.lc_init_state (numpy Philox, keyed by state_dict name) and inputs from seeded
generators, so the fixtures carry no weights.
  mlp_lc_small.npz   filters [48, 600, 600] (a width-changing and an identity ResidualBlock), input_shape 600, B = 5:
                     head widths 75 / 37;
  mlp_lc_preset.npz  the default preset widths [32, 64, 128, 256, 512, 1024], input_shape 16, B = 8.
Each holds: one eval forward, one training forward with the Dropout masks captured (F.dropout wrapped), the loss of the
training loop (latent_conditioner.py:293-296: 10*MSE(y1) + MSE(y2)) and its two terms, every gradient, the total norm of
clip_grad_norm_(10) and the parameters after one AdamW(1e-3, weight_decay 1e-4) step.  Tensors of more than FULL_MAX
elements are stored as their norm and SAMPLES entries at name-seeded positions (sample_positions), the rest in full.
  loop_mlp_lc.npz    train_latent_conditioner(..., is_image_data=False) for 3 epochs on filters [32, 64, 64],
                     input_shape 7 (not a multiple of 4), batches of 4 (8 training rows, 3 validation rows: a ragged batch),
                     the model's state loaded where the loop re-initialises it, Dropout keeping everything (scaled by
                     1/(1-p)), the mixup / noise coin flips pinned to "no" (torch.rand(1) returns 0.99).  Recorded as
                     loop_lc.npz is: every MSE value in call order, every step's gradient norm, the per-epoch log numbers
                     and norm + 64 sampled entries of every final state tensor."""
import os
import sys

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_lc_loop_fixtures as gl  # noqa: E402  (stand-ins, reference import path, Recorder, run_in_tmp, parse)
from simulgen_vae_amd.init import lc_csv_synthetic, lc_init_state  # noqa: E402
from tests.mlp_lc_torch import sample_positions  # noqa: E402

import modules.latent_conditioner as ref_lc  # noqa: E402
from modules.latent_conditioner_model_parametric import LatentConditioner as RefMLP  # noqa: E402

LATENT_END, LATENT, SIZE2 = 32, 8, 3
FULL_MAX, SAMPLES = 4096, 256
CONFIGS = {
    "mlp_lc_small": dict(filters=[48, 600, 600], input_shape=600, B=5, state_seed=41, data_seed=5),
    "mlp_lc_preset": dict(filters=[32, 64, 128, 256, 512, 1024], input_shape=16, B=8, state_seed=43, data_seed=6),
}
LOOP = dict(filters=[32, 64, 64], input_shape=7, B=4, p_train=8, p_val=3, epochs=3, state_seed=47, data_seed=77)


def put(out, key, name, t):
    a = t.detach().double().numpy().reshape(-1)
    if a.size <= FULL_MAX:
        out[key + name] = t.detach().numpy()
    else:
        out[key + "norm." + name] = np.array(np.linalg.norm(a))
        out[key + "samp." + name] = a[sample_positions(name, a.size, SAMPLES)]


def csv_data(seed, P, input_shape):
    return lc_csv_synthetic(seed, P, input_shape, LATENT_END, SIZE2, LATENT)


def make_model(filters, input_shape, state_seed, dropout_rate=0.3):
    torch.manual_seed(1)
    m = RefMLP(filters, LATENT_END, input_shape, LATENT, SIZE2, dropout_rate=dropout_rate)
    state = lc_init_state({k: tuple(v.shape) for k, v in m.state_dict().items()}, state_seed)
    return m, {k: torch.from_numpy(v.copy()) for k, v in state.items()}


def single_step(name, cfg):
    m, state = make_model(cfg["filters"], cfg["input_shape"], cfg["state_seed"])
    m.load_state_dict(state)
    B = cfg["B"]
    x, y1, y2 = (torch.from_numpy(a) for a in csv_data(cfg["data_seed"], B, cfg["input_shape"]))
    out = {"meta": np.array([LATENT_END, LATENT, SIZE2, cfg["input_shape"], B, cfg["state_seed"], cfg["data_seed"]], dtype=np.int64),
           "filters": np.array(cfg["filters"]), "keys": np.array(list(m.state_dict().keys())),
           "shapes": np.array([str(tuple(v.shape)) for v in m.state_dict().values()])}
    m.eval()
    with torch.no_grad():
        e1, e2 = m(x)
    out.update(eval_main=e1.numpy(), eval_xs=e2.numpy())
    m.train()
    g = torch.Generator().manual_seed(cfg["data_seed"] + 100)
    masks = []
    orig = F.dropout

    def rec_dropout(inp, p=0.5, training=True, inplace=False):
        if not training or p == 0.0:
            return inp
        mask = (torch.rand(inp.shape, generator=g) >= p).float()
        masks.append(mask)
        return inp * mask / (1.0 - p)
    F.dropout = rec_dropout
    try:
        p1, p2 = m(x)
    finally:
        F.dropout = orig
    A = nn.MSELoss()(p1, y1)
    Bl = nn.MSELoss()(p2, y2)
    loss = A * 10 + Bl
    opt = torch.optim.AdamW(m.parameters(), lr=1e-3, weight_decay=1e-4)
    opt.zero_grad(set_to_none=True)
    loss.backward()
    grads = {n: p.grad.detach().clone() for n, p in m.named_parameters()}
    total_norm = torch.nn.utils.clip_grad_norm_(m.parameters(), max_norm=10.0)
    opt.step()
    out.update(x=x.numpy(), y1=y1.numpy(), y2=y2.numpy(), train_main=p1.detach().numpy(), train_xs=p2.detach().numpy(),
               loss=np.array([loss.item(), A.item(), Bl.item()]), total_norm=np.array([float(total_norm)]), n_masks=np.array([len(masks)]))
    for i, mk in enumerate(masks):
        out[f"mask{i}"] = mk.numpy().astype(np.uint8)
    for n, gr in grads.items():
        put(out, "g.", n, gr)
    for k, v in m.state_dict().items():
        put(out, "s1.", k, v)
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **out)
    print(name, ":", len(grads), "tensors,", len(masks), "masks, loss", loss.item(), "norm", float(total_norm), os.path.getsize(path), "bytes")


def loop():
    c = LOOP
    m, state = make_model(c["filters"], c["input_shape"], c["state_seed"])
    x, y1, y2 = csv_data(c["data_seed"], c["p_train"] + c["p_val"], c["input_shape"])
    B = c["B"]
    batches = lambda lo, hi: [tuple(torch.from_numpy(a[i:min(i + B, hi)]) for a in (x, y1, y2)) for i in range(lo, hi, B)]
    train, val = batches(0, c["p_train"]), batches(c["p_train"], c["p_train"] + c["p_val"])
    real_he, real_rand, real_clip, real_drop = ref_lc.safe_initialize_weights_He, torch.rand, torch.nn.utils.clip_grad_norm_, F.dropout
    norms = []

    def he_then_load(mod):
        real_he(mod)
        if isinstance(mod, RefMLP):
            mod.load_state_dict(state)

    def clip(params, max_norm, *a, **k):
        n = real_clip(params, max_norm, *a, **k)
        norms.append(float(n))
        return n
    ref_lc.safe_initialize_weights_He = he_then_load
    torch.rand = lambda *a, **k: torch.tensor([0.99]) if a == (1,) else real_rand(*a, **k)
    torch.nn.utils.clip_grad_norm_ = clip
    F.dropout = gl.keep_all_dropout
    try:
        with gl.Recorder("MSELoss") as rec:
            _, lines = gl.run_in_tmp(lambda: ref_lc.train_latent_conditioner(c["epochs"], train, val, m, 1e-3, weight_decay=1e-4, is_image_data=False))
    finally:
        ref_lc.safe_initialize_weights_He, torch.rand, torch.nn.utils.clip_grad_norm_, F.dropout = real_he, real_rand, real_clip, real_drop
    epochs = gl.parse(lines, r"Train: ([0-9.E+-]+) \(y1:([0-9.E+-]+), y2:([0-9.E+-]+)\), Val: ([0-9.E+-]+) \(y1:([0-9.E+-]+), y2:([0-9.E+-]+)\), LR: ([0-9.E+-]+)")
    assert len(epochs) == c["epochs"], lines
    out = dict(meta=np.array([LATENT_END, LATENT, SIZE2, c["input_shape"], B, c["p_train"], c["p_val"], c["epochs"], c["state_seed"], c["data_seed"]],
                             dtype=np.int64),
               filters=np.array(c["filters"]), lr0=np.array(1e-3), wd=np.array(1e-4), mse=np.array([v for _, v in rec.values]),
               grad_norms=np.array(norms), epochs=epochs)
    gl.final_state(m, out)
    np.savez_compressed(os.path.join(HERE, "loop_mlp_lc.npz"), **out)
    print("loop_mlp_lc: mse calls", len(rec.values), "norms", norms, "\n", epochs)


if __name__ == "__main__":
    torch.set_num_threads(8)
    for name, cfg in CONFIGS.items():
        single_step(name, cfg)
    loop()
