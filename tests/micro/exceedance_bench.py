"""What the exceedance pass costs at preset-1 `small` (N = 95 008, T = 200), batch 16, bf16, random latents, for L = 1, 2 and 4
levels, both outputs.  Recorded, not asserted.

  levels: per node the mean over one generated batch plus 0, 0.5, 1 and 1.5 of its standard deviation, so that steps do exceed
      and runs do start and end;
  kernel times: the engine's own timers (sgv_kernel_time) around the output pass of sgv_generate ("recon_phys":
      recon_phys_tn_kernel) and around the exceedance pass of sgv_exceedance ("recon_exceed": recon_exceed_kernel) for every L, the
      passes alternating, mean over --batches calls, with the bytes each must move -- y once and the field written, or y once, the
      levels read and 24 L N bytes written per sample -- and the rate that comes to;
  whole studies of P = 64 conditions for every L: hipEvents on the engine stream, the variants alternating: the batch loop of
      Surrogate.exceedance on given latents -- the upload of the host levels, P / batch calls of Engine.exceedance, each into its
      rows of the result -- against as many calls of Engine.generate into a batch buffer, each followed by torch ops that give
      the same six outputs level by level (e = field > level; count = e.sum; first / last = argmax of e and of its flip, -1 where
      count is 0; runs = (e[1:] & ~e[:-1]).sum + e[0]; longest = max of cumsum(e) - cummax(where(~e, cumsum(e), 0)); excess =
      where(e, field - level, 0).sum), and against generating the fields alone.  (The conditioner in front of both is the same
      and left out, as in temporal_bench.py.)

--lib PATH loads another build of the library.  A process lands in one of two modes about 8 % apart, so
builds are compared through the ratio to recon_phys inside each job.

Prints one JSON line.  Usage: python tests/micro/exceedance_bench.py [--batches 10] [--blocks 3] [--members 64] [--levels 1 2 4]
[--lib PATH] [--small-net]"""
import json
import sys

import torch

import recon_bench_common as RB
from simulgen_vae_amd import engine as E


def torch_outputs(field, lv, stats, excess):
    """the six outputs of a batch from the stored field [B, T, N] by torch, level by level, into stats [B, 5, L, N] and excess [B, L, N]"""
    T = field.shape[1]
    for l in range(lv.shape[0]):
        e = field > lv[l]
        ei = e.to(torch.int32)
        count = ei.sum(1)
        none = count == 0
        stats[:, 0, l] = count
        stats[:, 1, l] = ei.argmax(1).masked_fill(none, -1)
        stats[:, 2, l] = (T - 1 - ei.flip(1).argmax(1)).masked_fill(none, -1)
        c = ei.cumsum(1, dtype=torch.int32)
        stats[:, 3, l] = (c - torch.where(e, 0, c).cummax(1).values).amax(1)
        stats[:, 4, l] = (e[:, 1:] & ~e[:, :-1]).sum(1) + ei[:, 0]
        excess[:, l] = torch.where(e, field - lv[l], 0.0).sum(1)


def main():
    ap = RB.parser(batches_help="calls per timed block of the kernel timers")
    ap.add_argument("--members", type=int, default=64, help="P: conditions of one study")
    ap.add_argument("--levels", type=int, nargs="+", default=[1, 2, 4], help="L: levels per node")
    ap.add_argument("--lib", default=None, help="another build of libsgvae.so")
    args = ap.parse_args()
    if args.lib:
        E.load_library(args.lib)
    env = RB.setup(args)
    N, T, B, nb, P, el, eng, stream, gen, scale, mn = env.N, env.T, env.B, env.nb, args.members, env.el, env.eng, env.stream, env.gen, env.scale, env.mn
    assert P % B == 0 and P >= 2 * B and all(1 <= L <= E.MAX_LEVELS for L in args.levels)
    z = torch.randn((P, 32), generator=gen, device="cuda")
    xs = torch.randn((3, P, 8), generator=gen, device="cuda") * 0.5
    fields = torch.empty((B, T, N), dtype=torch.float32, device="cuda")
    out = {"config": f"preset-1 small, N={N}, T={T}, batch {B}, {args.dtype}, P={P}, {nb} calls per block", "lib": args.lib or "the tree's"}
    torch.cuda.synchronize()

    with torch.cuda.stream(stream):
        zb = [z[lo:lo + B].contiguous() for lo in range(0, P, B)]
        xb = [xs[:, lo:lo + B].contiguous() for lo in range(0, P, B)]
        eng.generate(zb[0], xb[0], scale, mn, out=fields)
        flat = fields.reshape(B * T, N)
        mean, std = flat.mean(0), flat.std(0)
        all4 = torch.stack([mean + k * std for k in (0.0, 0.5, 1.0, 1.5)]).contiguous()
        lv = {L: all4[:L].contiguous() for L in args.levels}
        lvh = {L: lv[L].cpu().numpy() for L in args.levels}
        stats = {L: torch.empty((P, 5, L, N), dtype=torch.int32, device="cuda") for L in args.levels}
        excess = {L: torch.empty((P, L, N), dtype=torch.float32, device="cuda") for L in args.levels}
        ref_s = {L: torch.empty((B, 5, L, N), dtype=torch.int32, device="cuda") for L in args.levels}
        ref_e = {L: torch.empty((B, L, N), dtype=torch.float32, device="cuda") for L in args.levels}

        # ---- kernel times from the engine's timers ----
        bytes_ = {"recon_phys": B * T * N * el + B * T * N * 4}
        passes = {"recon_phys": lambda: eng.generate(zb[1], xb[1], scale, mn, out=fields)}
        for L in args.levels:
            bytes_[f"exceed_L{L}"] = B * T * N * el + L * N * 4 + B * 24 * L * N
            passes[f"exceed_L{L}"] = lambda L=L: eng.exceedance(zb[1], xb[1], scale, mn, lv[L], stats=stats[L][B:2 * B], excess=excess[L][B:2 * B])
        out["bytes"] = bytes_
        out.update(RB.kernel_blocks(eng, passes, lambda k: "recon_phys" if k == "recon_phys" else "recon_exceed", bytes_, nb, args.blocks))
        for L in args.levels:
            out[f"exceed_L{L}_over_recon_phys"] = round(out[f"exceed_L{L}_kernel_ms"] / out["recon_phys_kernel_ms"], 3)
        # what the levels do at the largest L: the share of exceeding steps and the mean number of runs per node and level
        Lm = max(args.levels)
        out["exceeding_share"] = [round(float(stats[Lm][B:2 * B, 0, l].float().mean()) / T, 4) for l in range(Lm)]
        out["mean_runs"] = [round(float(stats[Lm][B:2 * B, 4, l].float().mean()), 2) for l in range(Lm)]
        # the integer outputs of the torch comparator are the pass's on the same batch (the noise is drawn per call: re-seeded)
        at = eng.train_state()
        eng.exceedance(zb[1], xb[1], scale, mn, lv[Lm], stats=stats[Lm][B:2 * B], excess=excess[Lm][B:2 * B])
        eng.set_train_state(at["step"], at["seed"], at["draw"])
        eng.generate(zb[1], xb[1], scale, mn, out=fields)
        torch_outputs(fields, lv[Lm], ref_s[Lm], ref_e[Lm])
        out["torch_comparator_stats_equal"] = bool(torch.equal(ref_s[Lm], stats[Lm][B:2 * B]))

        # ---- whole studies of P conditions ----
        def generate_only():
            for i in range(P // B):
                eng.generate(zb[i], xb[i], scale, mn, out=fields)

        calls = {"generate_only": generate_only}
        for L in args.levels:
            def study(L=L):
                w = torch.from_numpy(lvh[L]).cuda()
                for i in range(P // B):
                    eng.exceedance(zb[i], xb[i], scale, mn, w, stats=stats[L][i * B:(i + 1) * B], excess=excess[L][i * B:(i + 1) * B])

            def generate_then_torch(L=L):
                w = torch.from_numpy(lvh[L]).cuda()
                for i in range(P // B):
                    eng.generate(zb[i], xb[i], scale, mn, out=fields)
                    torch_outputs(fields, w, stats[L][i * B:(i + 1) * B], excess[L][i * B:(i + 1) * B])
            calls[f"exceed_L{L}"] = study
            calls[f"generate_then_torch_L{L}"] = generate_then_torch
        out.update(RB.alternating(stream, calls, 1, 1, args.blocks, "_study_ms"))
    print(json.dumps(out))
    sys.stdout.flush()


if __name__ == "__main__":
    main()
