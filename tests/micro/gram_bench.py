"""What the Gram pass costs at preset-1 `small` (N = 95 008, T = 200), batch 16, bf16, random latents, with node weights and an
offset.  Recorded, not asserted.

  kernel times: the engine's own timers (sgv_kernel_time) around the output pass of sgv_generate ("recon_phys":
      recon_phys_tn_kernel) and around the Gram pass of sgv_gram ("recon_gram": recon_gram_kernel and recon_gram_finish_kernel
      together), the passes alternating, mean over --batches calls, with the MFMA work of the pass -- the tile pairs ti <= tj of the
      T rows padded to tiles of 32, 2 * 1024 flop per pair and channel -- the rate that comes to and the time as a multiple of the
      floor that work has at 64 flop per clock and SIMD (1024 SIMDs at 2.4 GHz: 157 Tflop/s);
  whole studies of P = 64 conditions: hipEvents on the engine stream, the variants alternating: the batch loop of Surrogate.gram on
      given latents -- P / batch calls of Engine.gram, each into its rows of values [P, T, T] -- against as many calls of
      Engine.generate into a batch buffer, each followed by fp32 torch.bmm(field, field.transpose(1, 2)) into the same rows
      (unweighted, no offset: the cheapest form of the alternative), and against generating the fields alone.  (The conditioner in
      front of all of them is the same and left out, as in project_bench.py.)

--lib PATH loads another build of the library.  A process lands in one of two modes about 8 % apart, so builds
are compared through the ratio to recon_phys inside each job.

Prints one JSON line.  Usage: python tests/micro/gram_bench.py [--batches 10] [--blocks 3] [--members 64] [--lib PATH] [--small-net]"""
import json
import sys

import torch

import recon_bench_common as RB
from simulgen_vae_amd import engine as E

PEAK_FLOPS = 64 * 1024 * 2.4e9          # fp32-input MFMA: 64 flop per clock and SIMD, 4 SIMDs on each of 256 CUs, 2.4 GHz


def main():
    ap = RB.parser(batches_help="calls per timed block of the kernel timers")
    ap.add_argument("--members", type=int, default=64, help="P: conditions of one study")
    ap.add_argument("--lib", default=None, help="another build of libsgvae.so")
    args = ap.parse_args()
    if args.lib:
        E.load_library(args.lib)
    env = RB.setup(args)
    N, T, B, nb, P, eng, stream, gen, scale, mn = env.N, env.T, env.B, env.nb, args.members, env.eng, env.stream, env.gen, env.scale, env.mn
    assert P % B == 0 and P >= 2 * B
    z = torch.randn((P, 32), generator=gen, device="cuda")
    xs = torch.randn((3, P, 8), generator=gen, device="cuda") * 0.5
    fields = torch.empty((B, T, N), dtype=torch.float32, device="cuda")
    nt = (T + 31) // 32
    flop = B * (nt * (nt + 1) // 2) * 2 * 1024 * N
    out = {"config": f"preset-1 small, N={N}, T={T}, batch {B}, {args.dtype}, P={P}, {nb} calls per block", "lib": args.lib or "the tree's",
           "workspace_bytes": eng.memory_info()["workspaces"], "mfma_gflop_per_pass": round(flop / 1e9, 2),
           "mfma_floor_ms": round(flop / PEAK_FLOPS * 1e3, 4)}
    torch.cuda.synchronize()

    with torch.cuda.stream(stream):
        zb = [z[lo:lo + B].contiguous() for lo in range(0, P, B)]
        xb = [xs[:, lo:lo + B].contiguous() for lo in range(0, P, B)]
        w = torch.rand(N, generator=gen, device="cuda") + 0.5
        m = torch.randn(N, generator=gen, device="cuda") * 0.1
        values = torch.empty((P, T, T), dtype=torch.float32, device="cuda")
        plain = torch.empty((P, T, T), dtype=torch.float32, device="cuda")

        # ---- kernel times from the engine's timers ----
        passes = {"recon_phys": lambda: eng.generate(zb[1], xb[1], scale, mn, out=fields),
                  "gram": lambda: eng.gram(zb[1], xb[1], scale, mn, node_weights=w, offset=m, out=values[B:2 * B]),
                  "gram_plain": lambda: eng.gram(zb[1], xb[1], scale, mn, out=plain[B:2 * B])}
        out.update(RB.kernel_blocks(eng, passes, lambda k: "recon_phys" if k == "recon_phys" else "recon_gram", {}, nb, args.blocks))
        for k in ("gram", "gram_plain"):
            out[f"{k}_over_recon_phys"] = round(out[f"{k}_kernel_ms"] / out["recon_phys_kernel_ms"], 3)
            out[f"{k}_tflops"] = round(flop / (out[f"{k}_kernel_ms"] * 1e-3) / 1e12, 2)
            out[f"{k}_over_mfma_floor"] = round(out[f"{k}_kernel_ms"] / out["mfma_floor_ms"], 3)

        # ---- whole studies of P conditions ----
        def generate_only():
            for i in range(P // B):
                eng.generate(zb[i], xb[i], scale, mn, out=fields)

        def study():
            for i in range(P // B):
                eng.gram(zb[i], xb[i], scale, mn, node_weights=w, offset=m, out=values[i * B:(i + 1) * B])

        def generate_then_bmm():
            for i in range(P // B):
                eng.generate(zb[i], xb[i], scale, mn, out=fields)
                torch.bmm(fields, fields.transpose(1, 2), out=plain[i * B:(i + 1) * B])

        out.update(RB.alternating(stream, {"generate_only": generate_only, "gram": study, "generate_then_bmm": generate_then_bmm}, 1, 1,
                                  args.blocks, "_study_ms"))
    print(json.dumps(out))
    sys.stdout.flush()


if __name__ == "__main__":
    main()
