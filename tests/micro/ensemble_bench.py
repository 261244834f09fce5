"""What the ensemble pass costs at preset-1 `small` (N = 95 008, T = 200), batch 16, bf16, random weights and latents, P = 64
members in four batches.  Recorded, not asserted.

  kernel times: the engine's own timers (sgv_kernel_time) around the output pass of sgv_generate ("recon_phys":
      recon_phys_tn_kernel) and around the ensemble pass of sgv_ensemble ("recon_ensemble": recon_ensemble_kernel) for every
      subset of the three groups, on a continuing batch (count_before = 16: the state is read and written) and, for all groups,
      on the first batch (count_before = 0: written only), mean over --batches calls, with the bytes each must move and the
      rate that comes to;
  whole studies: hipEvents on the engine stream, the variants alternating: P / batch calls of Engine.ensemble with all groups,
      against as many calls of Engine.generate into a [P, T, N] buffer followed by torch max / min (values and indices), mean,
      var and (F > limit).sum over dim 0.

Prints one JSON line.  Usage: python tests/micro/ensemble_bench.py [--batches 10] [--blocks 3] [--members 64] [--small-net]"""
import itertools
import json

import torch

import recon_bench_common as RB
from simulgen_vae_amd.engine import ENSEMBLE_GROUPS

STATE_ARRAYS = {"moments": 2, "extrema": 4, "exceed": 1}          # [T, N] arrays of 4 bytes a group reads and writes


def main():
    ap = RB.parser(batches_help="calls per timed block of the kernel timers")
    ap.add_argument("--members", type=int, default=64, help="P: members of one study")
    args = ap.parse_args()
    env = RB.setup(args)
    N, T, B, nb, P, el, eng, stream, gen, scale, mn = env.N, env.T, env.B, env.nb, args.members, env.el, env.eng, env.stream, env.gen, env.scale, env.mn
    assert P % B == 0
    z = torch.randn((P, 32), generator=gen, device="cuda")
    xs = torch.randn((3, P, 8), generator=gen, device="cuda") * 0.5
    fields = torch.empty((P, T, N), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()

    with torch.cuda.stream(stream):
        eng.generate(z[:B], xs[:, :B].contiguous(), scale, mn, out=fields[:B])
        limit = fields[:B].reshape(B * T, N).median(dim=0).values.contiguous()
        state = {}
        for g, names in ENSEMBLE_GROUPS.items():
            for k in names:
                state[k] = limit if k == "limit" else torch.zeros((T, N), dtype=torch.int32 if k in ("arg_max", "arg_min", "exceed") else torch.float32, device="cuda")
        zb = [z[lo:lo + B].contiguous() for lo in range(0, P, B)]
        xb = [xs[:, lo:lo + B].contiguous() for lo in range(0, P, B)]

        def one(groups, count_before):
            eng.ensemble(zb[0], xb[0], scale, mn, {k: state[k] for g in groups for k in ENSEMBLE_GROUPS[g]}, count_before)

        def study():
            for i in range(P // B):
                eng.ensemble(zb[i], xb[i], scale, mn, state, i * B)

        def generate_then_reduce():
            for i in range(P // B):
                eng.generate(zb[i], xb[i], scale, mn, out=fields[i * B:(i + 1) * B])
            return fields.max(dim=0), fields.min(dim=0), fields.mean(dim=0), fields.var(dim=0, unbiased=False), (fields > limit).sum(dim=0)

        subsets = [s for r in (1, 2, 3) for s in itertools.combinations(ENSEMBLE_GROUPS, r)]
        bytes_ = {"recon_phys": B * T * N * el + B * T * N * 4}
        for s in subsets:
            bytes_["+".join(s)] = B * T * N * el + 2 * 4 * T * N * sum(STATE_ARRAYS[g] for g in s)
        bytes_["first:" + "+".join(ENSEMBLE_GROUPS)] = B * T * N * el + 4 * T * N * sum(STATE_ARRAYS.values())
        out = {"config": f"preset-1 small, N={N}, T={T}, batch {B}, {args.dtype}, P={P}, {nb} calls per block", "bytes": bytes_}

        # ---- kernel times from the engine's timers ----
        passes = {"recon_phys": lambda: eng.generate(zb[0], xb[0], scale, mn, out=fields[:B])}
        for s in subsets:
            passes["+".join(s)] = lambda s=s: one(s, B)
        passes["first:" + "+".join(ENSEMBLE_GROUPS)] = lambda: one(tuple(ENSEMBLE_GROUPS), 0)
        out.update(RB.kernel_blocks(eng, passes, lambda k: "recon_phys" if k == "recon_phys" else "recon_ensemble", bytes_, nb, args.blocks))

        # ---- whole studies of P members ----
        calls = {"generate_only": lambda: [eng.generate(zb[i], xb[i], scale, mn, out=fields[i * B:(i + 1) * B]) for i in range(P // B)],
                 "generate_then_torch_reduce": generate_then_reduce, "ensemble": study}
        out.update(RB.alternating(stream, calls, 1, max(1, nb // 3), args.blocks, "_study_ms"))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
