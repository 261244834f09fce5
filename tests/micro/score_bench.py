"""What the error pass of surrogate scoring costs at preset-1 `small` (N = 95 008, T = 200), batch 16, bf16, random weights,
latents and truth.  Recorded, not asserted.

  kernel times: the engine's own timers (sgv_kernel_time) around the output pass of sgv_generate ("recon_phys": recon_phys_tn_kernel)
      and around the error pass of sgv_score ("recon_score": recon_score_kernel + the frame finalize, whichever the outputs asked
      for need), mean over --batches calls, with the bytes each must move and the rate that comes to;
  whole calls: hipEvents on the engine stream, the variants alternating: Engine.generate, Engine.generate followed by the torch
      reductions that give the same outputs from the stored field and the truth, Engine.score.

Prints one JSON line.  Usage: python tests/micro/score_bench.py [--batches 10] [--blocks 3] [--small-net]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import simulgen_vae_amd  # noqa: E402,F401
from simulgen_vae_amd.modules.VAE_network import VAE  # noqa: E402

ENC = [1024, 512, 256, 128]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=10, help="calls per timed block")
    ap.add_argument("--blocks", type=int, default=3, help="alternations of the variants")
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--small-net", action="store_true", help="N = 4096, T = 32: a quick functional run of this script")
    args = ap.parse_args()
    N, T = (4096, 32) if args.small_net else (95008, 200)
    B, nb = args.batch, args.batches
    vae = VAE(32, 8, ENC, ENC[::-1], N, T, lossfun="MSE", batch_size=B, small=True, compute_dtype=args.dtype).eval()
    eng = vae._eng(B)
    stream = torch.cuda.ExternalStream(eng.stream) if eng.stream else torch.cuda.current_stream()
    gen = torch.Generator(device="cuda").manual_seed(1)
    z = torch.randn((B, 32), generator=gen, device="cuda")
    xs = torch.randn((3, B, 8), generator=gen, device="cuda") * 0.5
    rng = np.random.default_rng(2)
    scale = np.exp(rng.uniform(np.log(1e-3), np.log(50.0), N)).astype(np.float32)
    scale = torch.from_numpy(np.where(rng.random(N) < 0.25, -scale, scale).astype(np.float32)).cuda()
    mn = torch.from_numpy(rng.standard_normal(N).astype(np.float32)).cuda()
    field = torch.empty((B, T, N), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    bufs = {}

    with torch.cuda.stream(stream):
        eng.generate(z, xs, scale, mn, out=field)
        truth = field * (1 + 0.1 * torch.randn(field.shape, generator=gen, device="cuda")) + 0.05 / scale.abs()

        def score(want):
            bufs.update(eng.score(z, xs, scale, mn, truth, want=want, out=bufs))

        def reduce_afterwards():
            eng.generate(z, xs, scale, mn, out=field)
            e = field - truth
            a, sq = e.abs(), e * e
            return a.max(dim=1), e.mean(dim=1), sq.mean(dim=1), a.max(dim=2), sq.mean(dim=2), (truth * truth).mean(dim=2)

        el = 2 if args.dtype == "bf16" else 4
        read = B * T * N * el + B * T * N * 4
        frame_part = B * T * ((N // 8 + 63) // 64) * 16
        bytes_ = {"recon_phys": B * T * N * el + B * T * N * 4,
                  "node": read + B * 4 * N * 4,
                  "frame": read + 2 * frame_part + B * T * 16,
                  "node+frame": read + B * 4 * N * 4 + 2 * frame_part + B * T * 16}
        out = {"config": f"preset-1 small, N={N}, T={T}, batch {B}, {args.dtype}, {nb} calls per block", "bytes": bytes_}

        # ---- kernel times from the engine's timers ----
        passes = {"recon_phys": lambda: eng.generate(z, xs, scale, mn, out=field), "node": lambda: score(("node",)),
                  "frame": lambda: score(("frame",)), "node+frame": lambda: score(("node", "frame"))}
        for fn in passes.values():
            fn()
        torch.cuda.synchronize()
        kern = {k: [] for k in passes}
        for _ in range(args.blocks):
            for k, fn in passes.items():
                eng.kernel_time_reset(True)
                for _ in range(nb):
                    fn()
                ms, n = eng.kernel_time("recon_phys" if k == "recon_phys" else "recon_score")
                assert n == nb, (k, n)
                kern[k].append(ms / n)
        eng.kernel_time_reset(False)
        for k, v in kern.items():
            out[k + "_kernel_ms_blocks"] = [round(t, 4) for t in v]
            out[k + "_kernel_ms"] = round(statistics.mean(v), 4)
            out[k + "_tb_per_s"] = round(bytes_[k] / (statistics.mean(v) * 1e-3) / 1e12, 3)

        # ---- whole calls ----
        def timed(fn, n):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record(stream)
            for _ in range(n):
                fn()
            b.record(stream)
            torch.cuda.synchronize()
            return a.elapsed_time(b) / n

        calls = {"generate": passes["recon_phys"], "generate_then_torch_reduce": reduce_afterwards, "score": passes["node+frame"]}
        for fn in calls.values():
            timed(fn, 2)
        res = {k: [] for k in calls}
        for _ in range(args.blocks):
            for k, fn in calls.items():
                res[k].append(timed(fn, nb))
        for k, v in res.items():
            out[k + "_call_ms_blocks"] = [round(t, 3) for t in v]
            out[k + "_call_ms"] = round(statistics.mean(v), 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
