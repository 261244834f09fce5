"""What the micro-benchmarks of the surrogate's output passes share (predict_bench.py, sweep_bench.py, score_bench.py,
ensemble_bench.py, sobol_bench.py): the common command line, the preset-1 `small` VAE with its engine and node scaler, hipEvent
timing on the engine stream, the engine's kernel timers read block by block, and the alternation of whole calls.  Byte models,
variants and reference reductions are each script's own."""
import argparse
import os
import statistics
import sys
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import simulgen_vae_amd  # noqa: E402,F401
from simulgen_vae_amd.modules.VAE_network import VAE  # noqa: E402

ENC = [1024, 512, 256, 128]


def parser(batches=10, batches_help="calls per timed block", small_net_help="N = 4096, T = 32: a quick functional run of this script"):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=batches, help=batches_help)
    ap.add_argument("--blocks", type=int, default=3, help="alternations of the variants")
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--small-net", action="store_true", help=small_net_help)
    return ap


def setup(args, signed=True):
    """N, T, B (batch), nb (batches per block), el (bytes of a stored x_hat element); the VAE, its engine and the engine stream as a
    torch stream; gen and rng, the device and host generators the script goes on drawing from; scale and mn [N] on the device,
    with `signed` a quarter of the scales negative"""
    N, T = (4096, 32) if args.small_net else (95008, 200)
    B = args.batch
    vae = VAE(32, 8, ENC, ENC[::-1], N, T, lossfun="MSE", batch_size=B, small=True, compute_dtype=args.dtype).eval()
    eng = vae._eng(B)
    stream = torch.cuda.ExternalStream(eng.stream) if eng.stream else torch.cuda.current_stream()
    rng = np.random.default_rng(2)
    scale = np.exp(rng.uniform(np.log(1e-3), np.log(50.0), N)).astype(np.float32)
    if signed:
        scale = np.where(rng.random(N) < 0.25, -scale, scale).astype(np.float32)
    mn = torch.from_numpy(rng.standard_normal(N).astype(np.float32)).cuda()
    torch.cuda.synchronize()
    return types.SimpleNamespace(N=N, T=T, B=B, nb=args.batches, el=2 if args.dtype == "bf16" else 4, vae=vae, eng=eng, stream=stream,
                                 gen=torch.Generator(device="cuda").manual_seed(1), rng=rng, scale=torch.from_numpy(scale).cuda(), mn=mn)


def timed(stream, fn, reps):
    """ms per call of fn over reps calls, between hipEvents on `stream`"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record(stream)
    for _ in range(reps):
        fn()
    b.record(stream)
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def kernel_blocks(eng, passes, tag_of, bytes_, nb, blocks):
    """Kernel times from the engine's timers: every pass of `passes` (name -> call) runs once to warm up, then nb times per block,
    the passes alternating; tag_of(name) is the timer it is read from.  Returns name_kernel_ms_blocks, name_kernel_ms and, where
    bytes_ has the name, name_tb_per_s."""
    for fn in passes.values():
        fn()
    torch.cuda.synchronize()
    kern = {k: [] for k in passes}
    for _ in range(blocks):
        for k, fn in passes.items():
            eng.kernel_time_reset(True)
            for _ in range(nb):
                fn()
            ms, n = eng.kernel_time(tag_of(k))
            assert n == nb, (k, n)
            kern[k].append(ms / n)
    eng.kernel_time_reset(False)
    out = {}
    for k, v in kern.items():
        out[k + "_kernel_ms_blocks"] = [round(t, 4) for t in v]
        out[k + "_kernel_ms"] = round(statistics.mean(v), 4)
        if k in bytes_:
            out[k + "_tb_per_s"] = round(bytes_[k] / (statistics.mean(v) * 1e-3) / 1e12, 3)
    return out


def alternating(stream, calls, warm, reps, blocks, suffix):
    """Whole calls between hipEvents: every call of `calls` (name -> call) runs `warm` times, then `reps` times per block, the
    calls alternating.  Returns name + suffix + "_blocks" and name + suffix (the mean of the blocks)."""
    for fn in calls.values():
        timed(stream, fn, warm)
    res = {k: [] for k in calls}
    for _ in range(blocks):
        for k, fn in calls.items():
            res[k].append(timed(stream, fn, reps))
    out = {}
    for k, v in res.items():
        out[k + suffix + "_blocks"] = [round(t, 3) for t in v]
        out[k + suffix] = round(statistics.mean(v), 3)
    return out
