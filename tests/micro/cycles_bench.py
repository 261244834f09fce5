"""What the cycles pass costs at preset-1 `small` (N = 95 008, T = 200), batch 16, bf16, random latents, for the turns, the rates and
both groups.  Recorded, not asserted.

  gate: per node a tenth of the standard deviation over one generated batch, so that reversals are both counted and filtered;
      exponent 3;
  kernel times: the engine's own timers (sgv_kernel_time) around the output pass of sgv_generate ("recon_phys":
      recon_phys_tn_kernel) and around the cycles pass of sgv_cycles ("recon_cycles": recon_cycles_kernel) for every choice of
      groups, the passes alternating, mean over --batches calls, with the bytes each must move -- y once and the field written, or
      y once, the gate read and 20 N bytes per group written per sample -- and the rate that comes to;
  whole studies of P = 64 conditions: hipEvents on the engine stream, the variants alternating: the batch loop of Surrogate.cycles
      on given latents -- the upload of the host gate, P / batch calls of Engine.cycles, each into its rows of the result -- against
      as many calls of Engine.generate into a batch buffer, each followed by the torch equivalent (the rates from one difference of
      the field; the turns by the state machine step by step over t with torch.where on [B, N] tensors, the only way torch has),
      and against generating the fields alone.  (The conditioner in front of both is the same and left out, as in
      temporal_bench.py.)

--lib PATH loads another build of the library.  A process lands in one of two modes about 8 % apart, so
builds are compared through the ratio to recon_phys inside each job.

Prints one JSON line.  Usage: python tests/micro/cycles_bench.py [--batches 10] [--blocks 3] [--members 64] [--lib PATH] [--small-net]"""
import json
import sys

import torch

import recon_bench_common as RB
from simulgen_vae_amd import engine as E

GROUPS = {"turns": (True, False), "rates": (False, True), "both": (True, True)}


def torch_rates(field, rate_when, rates):
    r = field[:, 1:] - field[:, :-1]
    rates[:, 0], rates[:, 1], rates[:, 2] = r.amax(1), r.amin(1), r.abs().sum(1)
    rate_when[:, 0], rate_when[:, 1] = r.argmax(1) + 1, r.argmin(1) + 1


def torch_turns(field, gate, m, reversals, ranges):
    """the state machine of the contract over t, torch.where on [B, N] tensors"""
    x0 = field[:, 0]
    a, b = x0.clone(), x0.clone()
    d = torch.zeros_like(x0, dtype=torch.int32)
    rev = torch.zeros_like(d)
    rsum, rmax, dmg = torch.zeros_like(x0), torch.zeros_like(x0), torch.zeros_like(x0)
    for t in range(1, field.shape[1]):
        x = field[:, t]
        z, p, n = d == 0, d == 1, d == -1
        up0 = z & (x - b > gate)
        dn0 = z & ~up0 & (a - x > gate)
        ext = (p & (x > a)) | (n & (x < a))
        peak = p & ~ext & (a - x > gate)
        vall = n & ~ext & (x - a > gate)
        trig = peak | vall
        R = torch.where(trig, (a - b).abs(), 0.0)
        rsum, rmax, dmg = rsum + R, torch.maximum(rmax, R), dmg + R ** m
        turn = up0 | dn0 | trig
        b = torch.where(up0, b, torch.where(dn0 | trig, a, torch.where(z, torch.minimum(b, x), b)))
        a = torch.where(turn | ext, x, torch.where(z, torch.maximum(a, x), a))
        d = torch.where(up0 | vall, 1, torch.where(dn0 | peak, -1, d))
        rev = rev + turn
    reversals.copy_(rev)
    ranges[:, 0], ranges[:, 1], ranges[:, 2], ranges[:, 3] = rsum, rmax, dmg, (a - b).abs()


def main():
    ap = RB.parser(batches_help="calls per timed block of the kernel timers")
    ap.add_argument("--members", type=int, default=64, help="P: conditions of one study")
    ap.add_argument("--lib", default=None, help="another build of libsgvae.so")
    args = ap.parse_args()
    if args.lib:
        E.load_library(args.lib)
    env = RB.setup(args)
    N, T, B, nb, P, el, eng, stream, gen, scale, mn = env.N, env.T, env.B, env.nb, args.members, env.el, env.eng, env.stream, env.gen, env.scale, env.mn
    assert P % B == 0 and P >= 2 * B
    m = 3
    z = torch.randn((P, 32), generator=gen, device="cuda")
    xs = torch.randn((3, P, 8), generator=gen, device="cuda") * 0.5
    fields = torch.empty((B, T, N), dtype=torch.float32, device="cuda")
    out = {"config": f"preset-1 small, N={N}, T={T}, batch {B}, {args.dtype}, P={P}, exponent {m}, {nb} calls per block", "lib": args.lib or "the tree's"}
    torch.cuda.synchronize()

    with torch.cuda.stream(stream):
        zb = [z[lo:lo + B].contiguous() for lo in range(0, P, B)]
        xb = [xs[:, lo:lo + B].contiguous() for lo in range(0, P, B)]
        eng.generate(zb[0], xb[0], scale, mn, out=fields)
        gate = (0.1 * fields.reshape(B * T, N).std(0)).contiguous()
        gh = gate.cpu().numpy()
        res = {"reversals": torch.empty((P, N), dtype=torch.int32, device="cuda"), "ranges": torch.empty((P, 4, N), device="cuda"),
               "rate_when": torch.empty((P, 2, N), dtype=torch.int32, device="cuda"), "rates": torch.empty((P, 3, N), device="cuda")}

        def cycles(i, g, turns, rates):
            s = slice(i * B, (i + 1) * B)
            eng.cycles(zb[i], xb[i], scale, mn, g, exponent=m, turns=(res["reversals"][s], res["ranges"][s]) if turns else False,
                       rates=(res["rate_when"][s], res["rates"][s]) if rates else False)

        # ---- kernel times from the engine's timers ----
        bytes_ = {"recon_phys": B * T * N * el + B * T * N * 4}
        passes = {"recon_phys": lambda: eng.generate(zb[1], xb[1], scale, mn, out=fields)}
        for name, (tu, ra) in GROUPS.items():
            bytes_[f"cycles_{name}"] = B * T * N * el + N * 4 + B * 20 * N * (tu + ra)
            passes[f"cycles_{name}"] = lambda tu=tu, ra=ra: cycles(1, gate, tu, ra)
        out["bytes"] = bytes_
        out.update(RB.kernel_blocks(eng, passes, lambda k: "recon_phys" if k == "recon_phys" else "recon_cycles", bytes_, nb, args.blocks))
        for name in GROUPS:
            out[f"cycles_{name}_over_recon_phys"] = round(out[f"cycles_{name}_kernel_ms"] / out["recon_phys_kernel_ms"], 3)
        # what the gate does: the mean number of reversals per node with it and without it
        s1 = slice(B, 2 * B)
        out["mean_reversals"] = round(float(res["reversals"][s1].float().mean()), 2)
        cycles(1, torch.zeros_like(gate), True, False)
        out["mean_reversals_gate_0"] = round(float(res["reversals"][s1].float().mean()), 2)
        # the integer outputs of the torch comparator are the pass's on the same batch (the noise is drawn per call: re-seeded)
        at = eng.train_state()
        cycles(1, gate, True, True)
        eng.set_train_state(at["step"], at["seed"], at["draw"])
        eng.generate(zb[1], xb[1], scale, mn, out=fields)
        ref = {k: torch.empty_like(v[:B]) for k, v in res.items()}
        torch_turns(fields, gate, m, ref["reversals"], ref["ranges"])
        torch_rates(fields, ref["rate_when"], ref["rates"])
        out["torch_comparator_reversals_equal"] = bool(torch.equal(ref["reversals"], res["reversals"][s1]))
        out["torch_comparator_rise_fall_equal"] = bool(torch.equal(ref["rates"][:, :2], res["rates"][s1][:, :2]))

        # ---- whole studies of P conditions ----
        def generate_only():
            for i in range(P // B):
                eng.generate(zb[i], xb[i], scale, mn, out=fields)

        calls = {"generate_only": generate_only}
        for name, (tu, ra) in GROUPS.items():
            def study(tu=tu, ra=ra):
                g = torch.from_numpy(gh).cuda()
                for i in range(P // B):
                    cycles(i, g, tu, ra)

            def generate_then_torch(tu=tu, ra=ra):
                g = torch.from_numpy(gh).cuda()
                for i in range(P // B):
                    s = slice(i * B, (i + 1) * B)
                    eng.generate(zb[i], xb[i], scale, mn, out=fields)
                    if tu:
                        torch_turns(fields, g, m, res["reversals"][s], res["ranges"][s])
                    if ra:
                        torch_rates(fields, res["rate_when"][s], res["rates"][s])
            calls[f"cycles_{name}"] = study
            calls[f"generate_then_torch_{name}"] = generate_then_torch
        out.update(RB.alternating(stream, calls, 1, 1, args.blocks, "_study_ms"))
    print(json.dumps(out))
    sys.stdout.flush()


if __name__ == "__main__":
    main()
