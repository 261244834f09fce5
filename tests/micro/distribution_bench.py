"""What the distribution pass costs at preset-1 `small` (N = 95 008, T = 200), batch 16, bf16, random weights and latents, P = 64
members in four batches, for K = 8, 32 and 64 bins.  Recorded, not asserted.

  kernel times: the engine's own timers (sgv_kernel_time) around the output pass of sgv_generate ("recon_phys":
      recon_phys_tn_kernel), around the extrema group of sgv_ensemble ("recon_ensemble": recon_ensemble_kernel) and around the
      distribution pass of sgv_distribution ("recon_hist": recon_hist_kernel) for every K, each on the second batch of the study
      between the envelope of all P members (the state is read and written), mean over --batches calls, with the bytes each must
      move at the most -- the distribution pass skips the rows of the state it has nothing to add to -- and the rate that comes to;
  whole studies: hipEvents on the engine stream, the variants alternating: the extrema pass over the P members, torch.zeros for
      the counts, the distribution pass over the same members and DistributionResult.quantile for P5 / P50 / P95, against P / batch
      calls of Engine.generate into a [P, T, N] buffer followed by torch.sort over dim 0 and the same three order statistics.

Prints one JSON line.  Usage: python tests/micro/distribution_bench.py [--batches 10] [--blocks 3] [--members 64] [--bins 8 32 64] [--small-net]"""
import json

import torch

import recon_bench_common as RB
from simulgen_vae_amd.predict import DistributionResult, quantile_rank

QS = (0.05, 0.5, 0.95)


def main():
    ap = RB.parser(batches_help="calls per timed block of the kernel timers")
    ap.add_argument("--members", type=int, default=64, help="P: members of one study")
    ap.add_argument("--bins", type=int, nargs="+", default=[8, 32, 64], help="K: bins")
    args = ap.parse_args()
    env = RB.setup(args)
    N, T, B, nb, P, el, eng, stream, gen, scale, mn = env.N, env.T, env.B, env.nb, args.members, env.el, env.eng, env.stream, env.gen, env.scale, env.mn
    assert P % B == 0 and P >= 2 * B
    z = torch.randn((P, 32), generator=gen, device="cuda")
    xs = torch.randn((3, P, 8), generator=gen, device="cuda") * 0.5
    fields = torch.empty((P, T, N), dtype=torch.float32, device="cuda")
    ranks = [quantile_rank(q, P) for q in QS]
    torch.cuda.synchronize()

    with torch.cuda.stream(stream):
        zb = [z[lo:lo + B].contiguous() for lo in range(0, P, B)]
        xb = [xs[:, lo:lo + B].contiguous() for lo in range(0, P, B)]
        ext = {k: torch.zeros((T, N), dtype=torch.int32 if k.startswith("arg") else torch.float32, device="cuda") for k in ("max", "min", "arg_max", "arg_min")}
        counts = {K: torch.zeros((K + 2, T, N), dtype=torch.int32, device="cuda") for K in args.bins}

        def extrema():
            for i in range(P // B):
                eng.ensemble(zb[i], xb[i], scale, mn, ext, i * B)

        def state(K, c=None):
            return {"lo": ext["min"], "hi": ext["max"], "counts": counts[K] if c is None else c}

        def study(K):
            extrema()
            st = state(K, torch.zeros((K + 2, T, N), dtype=torch.int32, device="cuda"))
            for i in range(P // B):
                eng.distribution(zb[i], xb[i], scale, mn, st, i * B)
            return DistributionResult(count=P, bins=K, lo=st["lo"], hi=st["hi"], counts=st["counts"]).quantile(QS)

        def generate_then_sort():
            for i in range(P // B):
                eng.generate(zb[i], xb[i], scale, mn, out=fields[i * B:(i + 1) * B])
            s = fields.sort(dim=0).values
            return torch.stack([s[r - 1] for r in ranks])

        extrema()                                   # the envelope of all P members, for the kernel times below
        bytes_ = {"recon_phys": B * T * N * el + B * T * N * 4, "extrema": B * T * N * el + 2 * 4 * T * N * 4}
        for K in args.bins:
            bytes_[f"hist_K{K}"] = B * T * N * el + 2 * 4 * T * N + 2 * 4 * T * N * (K + 2)
        out = {"config": f"preset-1 small, N={N}, T={T}, batch {B}, {args.dtype}, P={P}, {nb} calls per block", "bytes_at_most": bytes_}

        # ---- kernel times from the engine's timers: the second batch of the study ----
        passes = {"recon_phys": lambda: eng.generate(zb[1], xb[1], scale, mn, out=fields[:B]),
                  "extrema": lambda: eng.ensemble(zb[1], xb[1], scale, mn, ext, B)}
        for K in args.bins:
            passes[f"hist_K{K}"] = lambda K=K: eng.distribution(zb[1], xb[1], scale, mn, state(K), B)
        tags = {"recon_phys": "recon_phys", "extrema": "recon_ensemble"}
        out.update(RB.kernel_blocks(eng, passes, lambda k: tags.get(k, "recon_hist"), bytes_, nb, args.blocks))

        # ---- whole studies of P members ----
        calls = {"generate_only": lambda: [eng.generate(zb[i], xb[i], scale, mn, out=fields[i * B:(i + 1) * B]) for i in range(P // B)],
                 "generate_then_torch_sort": generate_then_sort, "extrema_only": extrema}
        for K in args.bins:
            calls[f"extrema_then_distribution_K{K}"] = lambda K=K: study(K)
        out.update(RB.alternating(stream, calls, 1, max(1, nb // 3), args.blocks, "_study_ms"))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
