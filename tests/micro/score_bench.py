"""What the error pass of surrogate scoring costs at preset-1 `small` (N = 95 008, T = 200), batch 16, bf16, random weights,
latents and truth.  Recorded, not asserted.

  kernel times: the engine's own timers (sgv_kernel_time) around the output pass of sgv_generate ("recon_phys": recon_phys_tn_kernel)
      and around the error pass of sgv_score ("recon_score": recon_score_kernel + the frame finalize, whichever the outputs asked
      for need), mean over --batches calls, with the bytes each must move and the rate that comes to;
  whole calls: hipEvents on the engine stream, the variants alternating: Engine.generate, Engine.generate followed by the torch
      reductions that give the same outputs from the stored field and the truth, Engine.score.

Prints one JSON line.  Usage: python tests/micro/score_bench.py [--batches 10] [--blocks 3] [--small-net]"""
import json

import torch

import recon_bench_common as RB


def main():
    args = RB.parser().parse_args()
    env = RB.setup(args)
    N, T, B, nb, el, eng, stream, gen, scale, mn = env.N, env.T, env.B, env.nb, env.el, env.eng, env.stream, env.gen, env.scale, env.mn
    z = torch.randn((B, 32), generator=gen, device="cuda")
    xs = torch.randn((3, B, 8), generator=gen, device="cuda") * 0.5
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
        out.update(RB.kernel_blocks(eng, passes, lambda k: "recon_phys" if k == "recon_phys" else "recon_score", bytes_, nb, args.blocks))

        # ---- whole calls ----
        calls = {"generate": passes["recon_phys"], "generate_then_torch_reduce": reduce_afterwards, "score": passes["node+frame"]}
        out.update(RB.alternating(stream, calls, 2, nb, args.blocks, "_call_ms"))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
