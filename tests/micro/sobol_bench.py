"""What the Sobol pass costs at preset-1 `small` (N = 95 008, T = 200), batch 16, bf16, random weights and latents, for d = 2 and
d = 6 parameters.  Recorded, not asserted.

  kernel times: the engine's own timers (sgv_kernel_time) around the output pass of sgv_generate ("recon_phys":
      recon_phys_tn_kernel) and around the Sobol pass of sgv_sobol ("recon_sobol": recon_sobol_kernel) with both parts and with
      each alone, on a continuing batch (blocks_before > 0: the state is read and written) and, for both parts, on the first
      batch (written only), mean over --batches calls, with the bytes each must move and the rate that comes to;
  whole studies of n = 64 base samples: hipEvents on the engine stream, the variants alternating: n (d + 2) / batch' calls of
      Engine.sobol (batch' = the whole blocks that fit the batch), against as many calls of Engine.generate into a batch buffer
      followed by the torch reductions that give the same outputs -- sum and sum of squares of the A and B fields (mean and
      variance), and the two sums of squared differences per parameter -- accumulated over the batches.

Prints one JSON line.  Usage: python tests/micro/sobol_bench.py [--batches 10] [--blocks 3] [--samples 64] [--small-net]"""
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
PARTS = {"first+total": ("first_sq", "total_sq"), "first": ("first_sq",), "total": ("total_sq",)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=10, help="calls per timed block of the kernel timers")
    ap.add_argument("--blocks", type=int, default=3, help="alternations of the variants")
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--samples", type=int, default=64, help="n: base samples of one study")
    ap.add_argument("--params", type=int, nargs="+", default=[2, 6], help="d: parameters")
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--small-net", action="store_true", help="N = 4096, T = 32: a quick functional run of this script")
    args = ap.parse_args()
    N, T = (4096, 32) if args.small_net else (95008, 200)
    B, nb, n = args.batch, args.batches, args.samples
    vae = VAE(32, 8, ENC, ENC[::-1], N, T, lossfun="MSE", batch_size=B, small=True, compute_dtype=args.dtype).eval()
    eng = vae._eng(B)
    stream = torch.cuda.ExternalStream(eng.stream) if eng.stream else torch.cuda.current_stream()
    gen = torch.Generator(device="cuda").manual_seed(1)
    rng = np.random.default_rng(2)
    scale = np.exp(rng.uniform(np.log(1e-3), np.log(50.0), N)).astype(np.float32)
    scale = torch.from_numpy(np.where(rng.random(N) < 0.25, -scale, scale).astype(np.float32)).cuda()
    mn = torch.from_numpy(rng.standard_normal(N).astype(np.float32)).cuda()
    fields = torch.empty((B, T, N), dtype=torch.float32, device="cuda")
    el = 2 if args.dtype == "bf16" else 4
    out = {"config": f"preset-1 small, N={N}, T={T}, batch {B}, {args.dtype}, n={n}, {nb} calls per block"}
    torch.cuda.synchronize()

    def timed(fn, reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record(stream)
        for _ in range(reps):
            fn()
        b.record(stream)
        torch.cuda.synchronize()
        return a.elapsed_time(b) / reps

    with torch.cuda.stream(stream):
        for d in args.params:
            S = d + 2
            per = B // S                                   # whole blocks per batch
            assert per >= 1 and n % per == 0
            M = per * S
            z = torch.randn((n * S, 32), generator=gen, device="cuda")
            xs = torch.randn((3, n * S, 8), generator=gen, device="cuda") * 0.5
            zb = [z[lo:lo + M].contiguous() for lo in range(0, n * S, M)]
            xb = [xs[:, lo:lo + M].contiguous() for lo in range(0, n * S, M)]
            state = {k: torch.zeros((T, N), device="cuda") for k in ("mean", "m2")}
            state.update({k: torch.zeros((d, T, N), device="cuda") for k in ("first_sq", "total_sq")})
            acc = dict(s1=torch.zeros((T, N), device="cuda"), s2=torch.zeros((T, N), device="cuda"),
                       first=torch.zeros((d, T, N), device="cuda"), total=torch.zeros((d, T, N), device="cuda"))

            def one(parts, before):
                eng.sobol(zb[0], xb[0], scale, mn, {k: state[k] for k in ("mean", "m2") + parts}, d, before)

            def study():
                for i in range(n // per):
                    eng.sobol(zb[i], xb[i], scale, mn, state, d, i * per)

            def generate_only():
                for i in range(n // per):
                    eng.generate(zb[i], xb[i], scale, mn, out=fields[:M])

            def generate_then_reduce():
                for v in acc.values():
                    v.zero_()
                for i in range(n // per):
                    eng.generate(zb[i], xb[i], scale, mn, out=fields[:M])
                    F = fields[:M].view(per, S, T, N)
                    ab = F[:, :2].reshape(2 * per, T, N)
                    acc["s1"] += ab.sum(dim=0)
                    acc["s2"] += (ab * ab).sum(dim=0)
                    acc["first"] += (F[:, 1:2] - F[:, 2:]).square().sum(dim=0)
                    acc["total"] += (F[:, 0:1] - F[:, 2:]).square().sum(dim=0)
                mean = acc["s1"] / (2 * n)
                return mean, acc["s2"] / (2 * n) - mean * mean

            tag = f"d{d}_"
            bytes_ = {"recon_phys": M * T * N * el + M * T * N * 4}
            for name, parts in PARTS.items():
                bytes_[name] = M * T * N * el + 2 * 4 * T * N * (2 + d * len(parts))
            bytes_["first:first+total"] = M * T * N * el + 4 * T * N * (2 + 2 * d)
            out[tag + "members_per_batch"] = M
            out[tag + "state_bytes"] = (2 + 2 * d) * 4 * T * N
            out[tag + "bytes"] = bytes_

            # ---- kernel times from the engine's timers ----
            passes = {"recon_phys": lambda: eng.generate(zb[0], xb[0], scale, mn, out=fields[:M])}
            for name, parts in PARTS.items():
                passes[name] = lambda parts=parts: one(parts, per)
            passes["first:first+total"] = lambda: one(PARTS["first+total"], 0)
            for fn in passes.values():
                fn()
            torch.cuda.synchronize()
            kern = {k: [] for k in passes}
            for _ in range(args.blocks):
                for k, fn in passes.items():
                    eng.kernel_time_reset(True)
                    for _ in range(nb):
                        fn()
                    ms, cnt = eng.kernel_time("recon_phys" if k == "recon_phys" else "recon_sobol")
                    assert cnt == nb, (k, cnt)
                    kern[k].append(ms / cnt)
            eng.kernel_time_reset(False)
            for k, v in kern.items():
                out[tag + k + "_kernel_ms_blocks"] = [round(t, 4) for t in v]
                out[tag + k + "_kernel_ms"] = round(statistics.mean(v), 4)
                out[tag + k + "_tb_per_s"] = round(bytes_[k] / (statistics.mean(v) * 1e-3) / 1e12, 3)

            # ---- whole studies of n base samples ----
            calls = {"generate_only": generate_only, "generate_then_torch_reduce": generate_then_reduce, "sobol": study}
            for fn in calls.values():
                timed(fn, 1)
            res = {k: [] for k in calls}
            for _ in range(args.blocks):
                for k, fn in calls.items():
                    res[k].append(timed(fn, 1))
            for k, v in res.items():
                out[tag + k + "_study_ms_blocks"] = [round(t, 3) for t in v]
                out[tag + k + "_study_ms"] = round(statistics.mean(v), 3)
            del state, acc, z, xs, zb, xb
    print(json.dumps(out))


if __name__ == "__main__":
    main()
