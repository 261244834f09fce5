"""What the temporal pass costs at preset-1 `small` (N = 95 008, T = 200), batch 16, bf16, random weights and latents, for R = 1, 8
and 32 functionals.  Recorded, not asserted.

  kernel times: the engine's own timers (sgv_kernel_time) around the output pass of sgv_generate ("recon_phys":
      recon_phys_tn_kernel) and around the temporal pass of sgv_temporal ("recon_temporal": recon_temporal_weights_kernel and
      recon_temporal_kernel together) for every R, the passes alternating, mean over --batches calls, with the bytes each must
      move -- y once and the field written, or y once and R rows of N values written per sample -- and the rate that comes to;
  whole studies of P = 64 conditions for every R: hipEvents on the engine stream, the variants alternating: the batch loop of
      Surrogate.temporal on given latents -- the upload of the host weights, P / batch calls of Engine.temporal, each into its rows
      of values [P, R, N] -- against as many calls of Engine.generate into a batch buffer, each followed by
      torch.einsum("rt,btn->brn", W, field) into the same rows, and against generating the fields alone.  (The conditioner in front
      of both is the same and left out, as in project_bench.py.)

--lib PATH loads another build of the library, e.g. one with another number of steps in flight (tp_flight, csrc/recon_out.hip).  A
process lands in one of two modes about 8 % apart, so builds are compared through the ratio to recon_phys
inside each job.

Prints one JSON line.  Usage: python tests/micro/temporal_bench.py [--batches 10] [--blocks 3] [--members 64] [--functionals 1 8 32]
[--lib PATH] [--small-net]"""
import json
import sys

import torch

import recon_bench_common as RB
from simulgen_vae_amd import engine as E


def main():
    ap = RB.parser(batches_help="calls per timed block of the kernel timers")
    ap.add_argument("--members", type=int, default=64, help="P: conditions of one study")
    ap.add_argument("--functionals", type=int, nargs="+", default=[1, 8, 32], help="R: weight rows")
    ap.add_argument("--lib", default=None, help="another build of libsgvae.so")
    args = ap.parse_args()
    if args.lib:
        E.load_library(args.lib)
    env = RB.setup(args)
    N, T, B, nb, P, el, eng, stream, gen, scale, mn = env.N, env.T, env.B, env.nb, args.members, env.el, env.eng, env.stream, env.gen, env.scale, env.mn
    assert P % B == 0 and P >= 2 * B
    z = torch.randn((P, 32), generator=gen, device="cuda")
    xs = torch.randn((3, P, 8), generator=gen, device="cuda") * 0.5
    fields = torch.empty((B, T, N), dtype=torch.float32, device="cuda")
    out = {"config": f"preset-1 small, N={N}, T={T}, batch {B}, {args.dtype}, P={P}, {nb} calls per block", "lib": args.lib or "the tree's",
           "workspace_bytes": eng.memory_info()["workspaces"]}
    torch.cuda.synchronize()

    with torch.cuda.stream(stream):
        zb = [z[lo:lo + B].contiguous() for lo in range(0, P, B)]
        xb = [xs[:, lo:lo + B].contiguous() for lo in range(0, P, B)]
        Wh = {R: env.rng.standard_normal((R, T)).astype("float32") for R in args.functionals}
        W = {R: torch.from_numpy(Wh[R]).cuda() for R in args.functionals}
        values = {R: torch.empty((P, R, N), dtype=torch.float32, device="cuda") for R in args.functionals}

        # ---- kernel times from the engine's timers ----
        bytes_ = {"recon_phys": B * T * N * el + B * T * N * 4}
        passes = {"recon_phys": lambda: eng.generate(zb[1], xb[1], scale, mn, out=fields)}
        for R in args.functionals:
            bytes_[f"temporal_R{R}"] = B * T * N * el + B * R * N * 4
            passes[f"temporal_R{R}"] = lambda R=R: eng.temporal(zb[1], xb[1], scale, mn, W[R], out=values[R][B:2 * B])
        out["bytes"] = bytes_
        out.update(RB.kernel_blocks(eng, passes, lambda k: "recon_phys" if k == "recon_phys" else "recon_temporal", bytes_, nb, args.blocks))
        for R in args.functionals:
            out[f"temporal_R{R}_over_recon_phys"] = round(out[f"temporal_R{R}_kernel_ms"] / out["recon_phys_kernel_ms"], 3)

        # ---- whole studies of P conditions ----
        def generate_only():
            for i in range(P // B):
                eng.generate(zb[i], xb[i], scale, mn, out=fields)

        calls = {"generate_only": generate_only}
        for R in args.functionals:
            def study(R=R):
                w = torch.from_numpy(Wh[R]).cuda()
                for i in range(P // B):
                    eng.temporal(zb[i], xb[i], scale, mn, w, out=values[R][i * B:(i + 1) * B])

            def generate_then_einsum(R=R):
                w = torch.from_numpy(Wh[R]).cuda()
                for i in range(P // B):
                    eng.generate(zb[i], xb[i], scale, mn, out=fields)
                    values[R][i * B:(i + 1) * B] = torch.einsum("rt,btn->brn", w, fields)
            calls[f"temporal_R{R}"] = study
            calls[f"generate_then_einsum_R{R}"] = generate_then_einsum
        out.update(RB.alternating(stream, calls, 1, 1, args.blocks, "_study_ms"))
    print(json.dumps(out))
    sys.stdout.flush()


if __name__ == "__main__":
    main()
