"""What a checkpoint costs at preset-1 `small`, batch 16, bf16.  Recorded, not asserted.

  (a) the per-tensor way: wall time of Engine.state_dict() plus Engine.adam_state() over every trainable key (one synchronous
      hipMemcpy and one host permutation per tensor);
  (b) how long Engine.snapshot_begin() holds its caller (the first call also allocates the staging buffer and builds the tables);
  (c) the time of the permute kernels on the engine stream (events around the call);
  (d) the mean step time of the steps that run while the device-to-host copy is in flight against undisturbed steps of the same
      process, in alternating blocks (event-timed on the engine stream, the permute kernels excluded).

Prints one JSON line.  Usage: python tests/micro/checkpoint_bench.py [--steps 8] [--blocks 5] [--small-net]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import simulgen_vae_amd  # noqa: E402,F401
from simulgen_vae_amd import engine as E  # noqa: E402
from simulgen_vae_amd.init import init_state  # noqa: E402
from simulgen_vae_amd.spec import VAEConfig  # noqa: E402

ENC = [1024, 512, 256, 128]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=8, help="steps per block")
    ap.add_argument("--blocks", type=int, default=5, help="alternations of (undisturbed, copy in flight)")
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--small-net", action="store_true", help="N = 4096, T = 32: a quick functional run of this script")
    ap.add_argument("--skip-per-tensor", action="store_true", help="leave (a) out")
    args = ap.parse_args()
    n_node, n_time = (4096, 32) if args.small_net else (95008, 200)
    cfg = VAEConfig(32, 8, ENC, ENC[::-1], n_node, n_time, "MSE", True)
    B = args.batch
    eng = E.Engine(cfg, max_batch=B, compute_dtype=args.dtype)
    eng.load_state(init_state(cfg, 7, reference_init=True))
    eng.set_option("write_xhat", 0)
    if args.dtype == "bf16":
        eng.set_option("grad_bf16", 1)
    gen = torch.Generator(device="cuda").manual_seed(1)
    x = torch.rand((B, n_node, n_time), generator=gen, device="cuda") * 1.4 - 0.7
    eng.set_input(x)
    stream = torch.cuda.current_stream()

    def steps(n):
        for _ in range(n):
            eng.forward(train=True, sync=False)
            eng.backward_step(1e6, 1e-4, 1e-4)

    def timed_steps(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        steps(n)
        b.record(stream)
        return a, b

    steps(5)
    torch.cuda.synchronize()
    total = eng.snapshot_floats()
    out = {"config": f"preset-1 small, N={n_node}, T={n_time}, batch {B}, {args.dtype}", "state_floats": total,
           "state_gb": round(total * 4 / 1e9, 3)}

    # (a) the per-tensor way
    if not args.skip_per_tensor:
        t0 = time.perf_counter()
        sd = eng.state_dict()
        for name, _shape, _kind, has_grad in eng.param_info():
            if has_grad:
                eng.adam_state(name)
        out["a_per_tensor_export_s"] = round(time.perf_counter() - t0, 3)
        del sd

    buf = torch.empty(total, dtype=torch.float32).pin_memory()
    # (b) / (c): first call (allocation, tables, stream probe), then steady state
    hold, kern, copy = [], [], []
    for i in range(4):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record(stream)
        eng.snapshot_begin(buf)
        b.record(stream)
        t1 = time.perf_counter()
        eng.snapshot_wait()
        t2 = time.perf_counter()
        torch.cuda.synchronize()
        hold.append((t1 - t0) * 1e3)
        kern.append(a.elapsed_time(b))
        copy.append((t2 - t0) * 1e3)
    out["b_begin_holds_caller_ms_first"] = round(hold[0], 3)
    out["b_begin_holds_caller_ms"] = round(statistics.median(hold[1:]), 3)
    out["c_permute_kernels_ms"] = round(statistics.median(kern[1:]), 3)
    out["begin_to_wait_ms"] = round(statistics.median(copy[1:]), 1)

    # (d) alternating blocks
    plain, busy, in_flight = [], [], []
    for _ in range(args.blocks):
        torch.cuda.synchronize()
        a, b = timed_steps(args.steps)
        torch.cuda.synchronize()
        plain.append(a.elapsed_time(b) / args.steps)
        eng.snapshot_begin(buf)
        t0 = time.perf_counter()
        a, b = timed_steps(args.steps)
        stream.synchronize()
        t1 = time.perf_counter()
        eng.snapshot_wait()
        t2 = time.perf_counter()
        busy.append(a.elapsed_time(b) / args.steps)
        in_flight.append(t2 - t1 > 1e-4)           # the copy outlasted the block: every timed step ran beside it
    out["d_step_ms_undisturbed"] = [round(v, 3) for v in plain]
    out["d_step_ms_copy_in_flight"] = [round(v, 3) for v in busy]
    out["d_copy_outlasted_block"] = in_flight
    out["d_mean_undisturbed_ms"] = round(statistics.mean(plain), 3)
    out["d_mean_copy_in_flight_ms"] = round(statistics.mean(busy), 3)
    out["d_spread_undisturbed_ms"] = round(max(plain) - min(plain), 3)
    print(json.dumps(out))
    eng.close()


if __name__ == "__main__":
    main()
