"""What the summary pass of a surrogate sweep costs at preset-1 `small` (N = 95 008, T = 200), batch 16, bf16, random weights and
latents.  Recorded, not asserted.

  kernel times: the engine's own timers (sgv_kernel_time) around the output pass of sgv_generate ("recon_phys": recon_phys_tn_kernel)
      and around the summary pass of sgv_summarize ("recon_summary": recon_summary_kernel + the frame finalize + the probe gather,
      whichever the outputs asked for need), mean over --batches calls, with the bytes each must move and the rate that comes to;
  whole calls: hipEvents on the engine stream, the variants alternating: Engine.generate, Engine.generate followed by the torch
      reductions that give the same summaries from the stored field, Engine.summarize.

Prints one JSON line.  Usage: python tests/micro/sweep_bench.py [--batches 10] [--blocks 3] [--probes 64] [--small-net]"""
import json

import numpy as np
import torch

import recon_bench_common as RB


def main():
    ap = RB.parser()
    ap.add_argument("--probes", type=int, default=64)
    args = ap.parse_args()
    env = RB.setup(args)
    N, T, B, nb, K, eng, gen, rng, scale, mn = env.N, env.T, env.B, env.nb, args.probes, env.eng, env.gen, env.rng, env.scale, env.mn
    z = torch.randn((B, 32), generator=gen, device="cuda")
    xs = torch.randn((3, B, 8), generator=gen, device="cuda") * 0.5
    field = torch.empty((B, T, N), dtype=torch.float32, device="cuda")
    probe_list = rng.integers(0, N, K).astype(np.int32)
    eng.set_probes(probe_list)
    nodes = torch.from_numpy(probe_list.astype(np.int64)).cuda()
    bufs = {}

    def summarize(want):
        bufs.update(eng.summarize(z, xs, scale, mn, want=want, out=bufs))

    def reduce_afterwards():
        eng.generate(z, xs, scale, mn, out=field)
        a, b = field.max(dim=1), field.min(dim=1)
        c, d = field.max(dim=2), field.min(dim=2)
        return a, b, field.mean(dim=1), c, d, field[:, :, nodes]

    read = B * T * N * env.el
    frame_part = B * T * ((N // 8 + 63) // 64) * 16
    bytes_ = {"recon_phys": read + B * T * N * 4,
              "node": read + B * 5 * N * 4,
              "frame": read + 2 * frame_part + B * T * 16,
              "node+frame": read + B * 5 * N * 4 + 2 * frame_part + B * T * 16}
    out = {"config": f"preset-1 small, N={N}, T={T}, batch {B}, {args.dtype}, {nb} calls per block, {K} probes", "bytes": bytes_}

    # ---- kernel times from the engine's timers ----
    passes = {"recon_phys": lambda: eng.generate(z, xs, scale, mn, out=field), "node": lambda: summarize(("node",)),
              "frame": lambda: summarize(("frame",)), "node+frame": lambda: summarize(("node", "frame")),
              "node+frame+probes": lambda: summarize(("node", "frame", "probes"))}
    out.update(RB.kernel_blocks(eng, passes, lambda k: "recon_phys" if k == "recon_phys" else "recon_summary", bytes_, nb, args.blocks))

    # ---- whole calls ----
    calls = {"generate": passes["recon_phys"], "generate_then_torch_reduce": reduce_afterwards, "summarize": passes["node+frame+probes"]}
    out.update(RB.alternating(env.stream, calls, 2, nb, args.blocks, "_call_ms"))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
