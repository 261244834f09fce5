"""What the regression pass costs at preset-1 `small` (N = 95 008, T = 200), batch 16, bf16, random weights and latents, for K = 2,
6 and 16 covariates.  Recorded, not asserted.

  kernel times: the engine's own timers (sgv_kernel_time) around the output pass of sgv_generate ("recon_phys":
      recon_phys_tn_kernel), around the moments of sgv_ensemble ("recon_ensemble") and around the regression pass of sgv_regress
      ("recon_regress": recon_regress_kernel) for every K, on a continuing batch (count_before > 0: the state is read and written),
      mean over --batches calls, with the bytes each must move -- y once, and the (2 + K) state arrays read and written once per
      launch of --members-per-launch members -- and the rate that comes to;
  whole studies of P = 64 members at K = --study-k: hipEvents on the engine stream, the variants alternating: regression_weights on
      the host, the upload of the weights, P / batch calls of Engine.regress and RegressionResult.coefficients() and r2(), against
      as many calls of Engine.generate into a batch buffer followed by the torch reductions that give the same outputs (sums of x,
      x^2 and x w_i accumulated over the batches, then the same coefficients and R^2), against generating the fields alone, and
      against the Sobol study of n = 64 base samples at d = --study-k parameters (Engine.sobol, whole blocks per batch).

--lib PATH loads another build of the library, e.g. one with another members-per-launch constant (rg_members, csrc/recon_out.hip);
--members-per-launch only enters the byte model.  A process lands in one of two modes about 8 % apart, so
builds are compared through the ratio to recon_phys inside each job.

Prints one JSON line.  Usage: python tests/micro/regress_bench.py [--batches 10] [--blocks 3] [--members 64] [--covariates 2 6 16]
[--study-k 6] [--members-per-launch 16] [--lib PATH] [--small-net]"""
import json
import sys

import numpy as np
import torch

import recon_bench_common as RB
from simulgen_vae_amd import engine as E
from simulgen_vae_amd.predict import RegressionResult, regression_weights


def main():
    ap = RB.parser(batches_help="calls per timed block of the kernel timers")
    ap.add_argument("--members", type=int, default=64, help="P: members of one study")
    ap.add_argument("--covariates", type=int, nargs="+", default=[2, 6, 16], help="K: covariates of the kernel times")
    ap.add_argument("--study-k", type=int, default=6, help="K of the whole study, and d of the Sobol study it is compared with")
    ap.add_argument("--members-per-launch", type=int, default=16, help="what the library under test was built with (byte model only)")
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
    launches = -(-B // args.members_per_launch)
    out = {"config": f"preset-1 small, N={N}, T={T}, batch {B}, {args.dtype}, P={P}, {nb} calls per block, {args.members_per_launch} members per launch",
           "lib": args.lib or "the tree's"}
    torch.cuda.synchronize()

    with torch.cuda.stream(stream):
        zb = [z[lo:lo + B].contiguous() for lo in range(0, P, B)]
        xb = [xs[:, lo:lo + B].contiguous() for lo in range(0, P, B)]
        Ks = sorted(set(args.covariates) | {args.study_k})
        Y = {K: env.rng.uniform(-1.0, 1.0, (P, K)) for K in Ks}
        W = {K: torch.from_numpy(regression_weights(Y[K])[0]).cuda() for K in Ks}
        state = {K: {"mean": torch.zeros((T, N), device="cuda"), "m2": torch.zeros((T, N), device="cuda"),
                     "comoment": torch.zeros((K, T, N), device="cuda")} for K in Ks}
        mom = {k: torch.zeros((T, N), device="cuda") for k in ("mean", "m2")}

        # ---- kernel times from the engine's timers: the second batch of the study ----
        bytes_ = {"recon_phys": B * T * N * el + B * T * N * 4, "moments": B * T * N * el + 2 * 2 * 4 * T * N}
        passes = {"recon_phys": lambda: eng.generate(zb[1], xb[1], scale, mn, out=fields),
                  "moments": lambda: eng.ensemble(zb[1], xb[1], scale, mn, mom, B)}
        for K in args.covariates:
            bytes_[f"regress_K{K}"] = B * T * N * el + launches * (2 + K) * 2 * 4 * T * N
            passes[f"regress_K{K}"] = lambda K=K: eng.regress(zb[1], xb[1], scale, mn, state[K], W[K][B:2 * B], B)
        tags = {"recon_phys": "recon_phys", "moments": "recon_ensemble"}
        out["bytes"] = bytes_
        out.update(RB.kernel_blocks(eng, passes, lambda k: tags.get(k, "recon_regress"), bytes_, nb, args.blocks))
        for K in args.covariates:
            out[f"regress_K{K}_over_recon_phys"] = round(out[f"regress_K{K}_kernel_ms"] / out["recon_phys_kernel_ms"], 3)

        # ---- whole studies of P members ----
        K = d = args.study_k
        acc = dict(s1=torch.zeros((T, N), device="cuda"), s2=torch.zeros((T, N), device="cuda"), sw=torch.zeros((K, T, N), device="cuda"))

        def derived(res):
            return res.coefficients(), res.r2()

        def study():
            w, ybar, gram = regression_weights(Y[K])
            w = torch.from_numpy(w).cuda()
            for i in range(P // B):
                eng.regress(zb[i], xb[i], scale, mn, state[K], w[i * B:(i + 1) * B], i * B)
            st = state[K]
            return derived(RegressionResult(count=P, mean=st["mean"], m2=st["m2"], comoment=st["comoment"], cov_mean=ybar, cov_gram=gram))

        def generate_only():
            for i in range(P // B):
                eng.generate(zb[i], xb[i], scale, mn, out=fields)

        def generate_then_reduce():
            Yc = Y[K] - Y[K].mean(0)
            gram = Yc.T @ Yc
            wc = torch.from_numpy(Yc.astype(np.float32)).cuda()
            for v in acc.values():
                v.zero_()
            for i in range(P // B):
                eng.generate(zb[i], xb[i], scale, mn, out=fields)
                acc["s1"] += fields.sum(dim=0)
                acc["s2"] += (fields * fields).sum(dim=0)
                acc["sw"] += (wc[i * B:(i + 1) * B].t() @ fields.view(B, T * N)).view(K, T, N)          # sum x (y - ybar) = the co-moment
            mean = acc["s1"] / P
            return derived(RegressionResult(count=P, mean=mean, m2=acc["s2"] - P * mean * mean, comoment=acc["sw"], cov_mean=Y[K].mean(0), cov_gram=gram))

        calls = {"generate_only": generate_only, "generate_then_torch_reduce": generate_then_reduce, "regress": study}
        S = d + 2
        per = B // S
        if per >= 1 and P % per == 0:
            M = per * S
            zs = torch.randn((P * S, 32), generator=gen, device="cuda")
            xss = torch.randn((3, P * S, 8), generator=gen, device="cuda") * 0.5
            zsb = [zs[lo:lo + M].contiguous() for lo in range(0, P * S, M)]
            xsb = [xss[:, lo:lo + M].contiguous() for lo in range(0, P * S, M)]
            sob = {k: torch.zeros((T, N), device="cuda") for k in ("mean", "m2")}
            sob.update({k: torch.zeros((d, T, N), device="cuda") for k in ("first_sq", "total_sq")})

            def sobol():
                for i in range(P // per):
                    eng.sobol(zsb[i], xsb[i], scale, mn, sob, d, i * per)
            calls["sobol"] = sobol
        out.update({f"K{K}_" + k: v for k, v in RB.alternating(stream, calls, 1, 1, args.blocks, "_study_ms").items()})
    print(json.dumps(out))
    sys.stdout.flush()


if __name__ == "__main__":
    main()
