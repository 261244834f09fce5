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
import json

import torch

import recon_bench_common as RB

PARTS = {"first+total": ("first_sq", "total_sq"), "first": ("first_sq",), "total": ("total_sq",)}


def main():
    ap = RB.parser(batches_help="calls per timed block of the kernel timers")
    ap.add_argument("--samples", type=int, default=64, help="n: base samples of one study")
    ap.add_argument("--params", type=int, nargs="+", default=[2, 6], help="d: parameters")
    args = ap.parse_args()
    env = RB.setup(args)
    N, T, B, nb, n, el, eng, stream, gen, scale, mn = env.N, env.T, env.B, env.nb, args.samples, env.el, env.eng, env.stream, env.gen, env.scale, env.mn
    fields = torch.empty((B, T, N), dtype=torch.float32, device="cuda")
    out = {"config": f"preset-1 small, N={N}, T={T}, batch {B}, {args.dtype}, n={n}, {nb} calls per block"}
    torch.cuda.synchronize()

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
            kern = RB.kernel_blocks(eng, passes, lambda k: "recon_phys" if k == "recon_phys" else "recon_sobol", bytes_, nb, args.blocks)
            out.update({tag + k: v for k, v in kern.items()})

            # ---- whole studies of n base samples ----
            calls = {"generate_only": generate_only, "generate_then_torch_reduce": generate_then_reduce, "sobol": study}
            out.update({tag + k: v for k, v in RB.alternating(stream, calls, 1, 1, args.blocks, "_study_ms").items()})
            del state, acc, z, xs, zb, xb
    print(json.dumps(out))


if __name__ == "__main__":
    main()
