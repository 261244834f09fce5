"""Training-step time of the parametric (CSV) latent conditioner at batch 64 with the default preset widths
(32 64 128 256 512 1024), for 16 and 600 input columns: forward, 10*MSE(y1) + MSE(y2), backward, clip_grad_norm_(10) and
AdamW -- the HIP path (modules/latent_conditioner_model_parametric.py on csrc/mlp.hip) and, beside it, the same model in
PyTorch eager on the same GPU (the restatement in tests/mlp_lc_torch.py, torch.optim.AdamW).  Warm-up steps first, then
hipEvents around the timed steps; one JSON line on stdout.

    python tests/micro/mlp_lc_bench.py [--steps 200] [--warmup 20] [--inputs 16 600] [--hip-only]

--hip-only skips the eager baseline (for a kernel trace of the HIP path alone: rocprofv3 --kernel-trace --stats -- python ...)."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import simulgen_vae_amd  # noqa: E402
from simulgen_vae_amd.modules import latent_conditioner as L  # noqa: E402
from simulgen_vae_amd.modules.latent_conditioner_model_parametric import LatentConditioner  # noqa: E402
from tests.mlp_lc_torch import TorchMLPConditioner  # noqa: E402

FILTERS = [32, 64, 128, 256, 512, 1024]
B, LATENT_END, LATENT, SIZE2, LR, WD = 64, 32, 8, 3, 1e-3, 1e-4


def timed(step, warmup, steps):
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        step()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def hip_step_ms(n_in, data, warmup, steps):
    x, y1, y2 = data
    m = LatentConditioner(FILTERS, LATENT_END, n_in, LATENT, SIZE2)
    m.apply(None)
    assert m._fused()

    def step():
        m.loss_backward(x, y1, y2, sync=False)
        m.pset.step(LR, WD, 10.0, want_norm=False)
    return timed(step, warmup, steps)


def torch_step_ms(n_in, data, warmup, steps):
    x, y1, y2 = data
    m = TorchMLPConditioner(FILTERS, LATENT_END, n_in, LATENT, SIZE2).cuda().train()
    opt = torch.optim.AdamW(m.parameters(), lr=LR, weight_decay=WD)
    mse = torch.nn.MSELoss()

    def step():
        opt.zero_grad(set_to_none=True)
        p1, p2 = m(x)
        loss = 10 * mse(p1, y1) + mse(p2, y2)
        loss.backward()
        torch.nn.utils.clip_grad_norm_(m.parameters(), max_norm=10.0)
        opt.step()
    return timed(step, warmup, steps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--inputs", type=int, nargs="+", default=[16, 600])
    ap.add_argument("--hip-only", action="store_true")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    res = {"workload": "mlp_lc_train_step", "batch": B, "filters": FILTERS, "steps": a.steps, "warmup": a.warmup}
    for n_in in a.inputs:
        g = torch.Generator().manual_seed(n_in)
        data = (torch.rand(B, n_in, generator=g).cuda() * 1.4 - 0.7, torch.randn(B, LATENT_END, generator=g).cuda() * 0.5,
                torch.randn(B, SIZE2, LATENT, generator=g).cuda() * 0.5)
        r = {"hip_step_ms": round(hip_step_ms(n_in, data, a.warmup, a.steps), 4)}
        r["hip_samples_per_s"] = round(B / r["hip_step_ms"] * 1e3, 1)
        if not a.hip_only:
            r["torch_eager_step_ms"] = round(torch_step_ms(n_in, data, a.warmup, a.steps), 4)
            r["torch_eager_samples_per_s"] = round(B / r["torch_eager_step_ms"] * 1e3, 1)
        res[f"inputs_{n_in}"] = r
    print(json.dumps(res))


if __name__ == "__main__":
    main()
