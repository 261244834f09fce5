"""What surrogate prediction costs at preset-1 `small` (N = 95 008, T = 200), batch 16, bf16, random weights and latents
(DESIGN.md section 16).  Recorded, not asserted.  hipEvents on the engine stream, the variants alternating in one process; every
time is the mean over --batches batches after a warm-up, per block, and the blocks' means are listed.

  (a) the old way: sgv_decode(fix) (eval loss pass, bf16 x_hat) -> sgv_get_xhat (transpose to [B, N, T] fp32) -> a torch device
      expression for the inverse scaling into [B, T, N]; a_sync is the same through Engine.decode, which waits for the scalars;
  (b) Engine.generate(..., layout="TN"); b_nt the same with layout="NT";
  (c) the new kernel alone: not separable with events from inside the engine, so it is a kernel time -- profile this script with
      `rocprofv3 --kernel-trace --stats -- python tests/micro/predict_bench.py --only ab --blocks 1` and read recon_phys_tn_kernel
      against gn_bwd_reduce_kernel + transpose_kernel + the torch kernels of (a); bytes the kernel must move: 2 B read + 4 B
      written per element (printed as c_bytes);
  (d) Surrogate.predict per batch with the image conditioner at 256 x 256;
  (e) Surrogate.predict_to_host per batch, with the device-to-host rate that comes to.

Prints one JSON line.  Usage: python tests/micro/predict_bench.py [--batches 20] [--blocks 3] [--host-batches 6] [--only ab] [--small-net]"""
import ctypes as C
import json
import statistics
import time
import types

import numpy as np
import torch

import recon_bench_common as RB
from simulgen_vae_amd.modules.latent_conditioner_model_cnn import LatentConditionerImg
from simulgen_vae_amd.predict import Surrogate

LC_FILTERS = [32, 64, 128, 256, 512, 1024]          # tests/micro/e2e_bench.py


def main():
    ap = RB.parser(batches=20, batches_help="batches per timed block", small_net_help="N = 4096, T = 32, 64 x 64 images: a quick functional run of this script")
    ap.add_argument("--host-batches", type=int, default=6, help="batches per block of (e): its pinned result is batches x 1.2 GB")
    ap.add_argument("--only", default="abde", help="which of a, b, d, e to run")
    args = ap.parse_args()
    side = 64 if args.small_net else 256
    env = RB.setup(args, signed=False)
    n_node, n_time, B, nb, vae, eng, gen, scale, mn = env.N, env.T, env.B, env.nb, env.vae, env.eng, env.gen, env.scale, env.mn
    z = torch.randn((B, 32), generator=gen, device="cuda")
    xs = torch.randn((3, B, 8), generator=gen, device="cuda") * 0.5
    out_tn = torch.empty((B, n_time, n_node), dtype=torch.float32, device="cuda")
    out_nt = torch.empty((B, n_node, n_time), dtype=torch.float32, device="cuda")
    lib, vp = eng.lib, C.c_void_p

    def old(sync):
        if sync:
            eng.decode(z, list(xs), fix=True)
        else:
            rc = lib.sgv_decode(eng.h, vp(z.data_ptr()), vp(xs.data_ptr()), B, 1, None)
            assert rc == 0, lib.sgv_last_error().decode()
            eng.batch = B
        xh = eng.xhat()
        torch.div(torch.sub(xh, mn[None, :, None]).transpose(1, 2), scale[None, None, :], out=out_tn)

    variants = {"a": lambda: old(False), "a_sync": lambda: old(True),
                "b": lambda: eng.generate(z, xs, scale, mn, out=out_tn, layout="TN"),
                "b_nt": lambda: eng.generate(z, xs, scale, mn, out=out_nt, layout="NT")}
    if "a" not in args.only:
        variants.pop("a"), variants.pop("a_sync")
    if "b" not in args.only:
        variants.pop("b"), variants.pop("b_nt")
    sur = cond = None
    if "d" in args.only or "e" in args.only:
        lc = LatentConditionerImg(LC_FILTERS, 32, (1, side, side), 8, 3, (side, side), dropout_rate=0.2, compute_dtype=args.dtype)
        ns = lambda n: types.SimpleNamespace(scale_=np.linspace(0.5, 2.0, n), min_=np.linspace(-0.5, 0.5, n))
        sur = Surrogate(vae, lc, ns(32), ns(24), types.SimpleNamespace(scale_=scale.cpu().numpy(), min_=mn.cpu().numpy()), batch=B)
        cond = torch.rand((B * nb, side * side), generator=gen, device="cuda")
        out_dev = torch.empty((B * nb, n_time, n_node), dtype=torch.float32, device="cuda") if "d" in args.only else None
        nh = min(nb, args.host_batches)
        out_host = torch.empty((B * nh, n_time, n_node), dtype=torch.float32, pin_memory=True) if "e" in args.only else None

    out = {"config": f"preset-1 small, N={n_node}, T={n_time}, batch {B}, {args.dtype}, {nb} batches per block",
           "c_bytes": B * n_time * n_node * (env.el + 4)}
    out.update(RB.alternating(env.stream, variants, 3, nb, args.blocks, "_ms"))
    if "d" in args.only:
        sur.predict(cond[:2 * B], out=out_dev[:2 * B])
        d = [RB.timed(env.stream, lambda: sur.predict(cond, out=out_dev), 1) / nb for _ in range(args.blocks)]
        out["d_predict_ms_per_batch_blocks"], out["d_predict_ms_per_batch"] = [round(t, 3) for t in d], round(statistics.mean(d), 3)
    if "e" in args.only:
        sur.predict_to_host(cond[:2 * B], out=out_host[:2 * B])
        e = []
        for _ in range(args.blocks):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            sur.predict_to_host(cond[:B * nh], out=out_host)          # returns after its one host wait
            e.append((time.perf_counter() - t0) * 1e3 / nh)
        out["e_to_host_ms_per_batch_blocks"], out["e_to_host_ms_per_batch"] = [round(t, 3) for t in e], round(statistics.mean(e), 3)
        out["e_d2h_gb_per_s"] = round(B * n_time * n_node * 4 / (statistics.mean(e) * 1e-3) / 1e9, 1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
