#!/usr/bin/env python3
"""Assemble profiles/r01_summary.md (+ the raw files it cites) from one tools/profile_round.sh output directory:
  python tools/write_round_summary.py gpurun_out/r01e [tn_sq.txt]
expects <dir>/stats, <dir>/stats_serial, <dir>/fetch, <dir>/write, <dir>/sq_*, <dir>/bench_line.json, <dir>/layers.log."""
import csv, glob, io, json, os, shutil, subprocess, sys, collections

O = sys.argv[1]
tn_sq = open(sys.argv[2]).read().strip() if len(sys.argv) > 2 and os.path.exists(sys.argv[2]) else None
here = os.path.dirname(os.path.abspath(__file__))
run = lambda *a: subprocess.run([sys.executable, os.path.join(here, "summarize_profile.py"), *a], capture_output=True, text=True, check=True).stdout
one = lambda pat: glob.glob(os.path.join(O, pat))[0]
serial = run("stats", one("stats_serial/runc/*_kernel_stats.csv"), "0")
overl = run("stats", one("stats/runc/*_kernel_stats.csv"), "0")
fetch = run("pmc", one("fetch/runc/*_counter_collection.csv"))
write = run("pmc", one("write/runc/*_counter_collection.csv"))
traffic = json.loads(run("traffic", one("fetch/runc/*_counter_collection.csv"), one("write/runc/*_counter_collection.csv")))
overlap = subprocess.run([sys.executable, os.path.join(here, "trace_overlap.py"), one("stats/runc/*_kernel_trace.csv")], capture_output=True, text=True).stdout.strip()
bench = open(os.path.join(O, "bench_line.json")).read().strip().splitlines()[-1]
b = json.loads(bench)
layers = [l[:170] for l in open(os.path.join(O, "layers.log")).read().splitlines() if " us " in l and "TF/s" in l][:40]
agg = collections.defaultdict(list)
for f in glob.glob(os.path.join(O, "sq_*/**/*counter_collection.csv"), recursive=True):
    for r in csv.DictReader(open(f)):
        if "gemm_nt_wide64p" in r["Kernel_Name"]:
            agg[r["Counter_Name"]].append(float(r["Counter_Value"]))
sq = "\n".join(f"{k:28s} {sorted(v)[len(v) // 2]:.3e}" for k, v in sorted(agg.items()))
dur = []
for f in glob.glob(os.path.join(O, "sq_SQ_WAVE_CYCLES/**/*kernel_trace.csv"), recursive=True):
    dur += [int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in csv.DictReader(open(f)) if "gemm_nt_wide64p" in r["Kernel_Name"]]
dur_us = sorted(dur)[len(dur) // 2] / 1e3 if dur else float("nan")
P = os.path.join(os.path.dirname(here), "profiles")
open(os.path.join(P, "r01_bench_line.json"), "w").write(bench + "\n")
shutil.copy(one("stats_serial/runc/*_kernel_stats.csv"), os.path.join(P, "r01_bench_kernel_stats.csv"))
shutil.copy(one("stats/runc/*_kernel_stats.csv"), os.path.join(P, "r01_bench_kernel_stats_overlapped.csv"))
json.dump(traffic, open(os.path.join(P, "r01_traffic.json"), "w"), indent=1)
mf = agg.get("SQ_VALU_MFMA_BUSY_CYCLES", [0])[0] / (1024 * dur_us * 1e-6 * 2.4e9) * 100 if dur else 0
doc = f"""# Round 1 — rocprofv3 summaries (MI355X, bf16, batch 16, preset-1 small)

Collected by `tools/profile_round.sh` (one gpurun call, separate rocprofv3 processes per pass) plus one serial-mode
kernel-stats pass, assembled by `tools/write_round_summary.py` (tables by `tools/summarize_profile.py`).  Code state: the
commit this file belongs to.  Un-profiled bench of the same build on the same box (`profiles/r01_bench_line.json`):
{b["value"]:.0f} samples/s, {b["ms_per_step"]:.2f} ms/step (first GPU measurement of the round: 196 samples/s); box-to-box spread is
about ±3 %.  The GPU runs at ≈2.2 GHz / 1.13-1.16 kW under this load (rocm-smi during a 600-step run), 8 % below the
2.4 GHz the peak figures assume; under rocprofv3 the same bench reads 5-15 % lower.

## Kernel time per training step, one stream (comparable with bench.py's roofline numbers)

Command: `SGV_DW_SIDE=0 rocprofv3 --kernel-trace --stats --output-format csv -- python3 bench.py --full --steps 10 --warmup 3 --cpu-baseline skip`
(raw: `profiles/r01_bench_kernel_stats.csv`).  bench.py's kernel-timing pass also runs on one stream, so its `avg_launch_ms`
(hipEvents; {b["roofline"]["avg_launch_ms"] * 1e3:.0f} µs for gemm_nt_wide64p, {b["roofline_gemm_tn"]["avg_launch_ms"] * 1e3:.0f} µs for the weight-gradient class in the
un-profiled run) is to be compared with the averages below (the profiled run is slower by the tool's clock effect; the events
also see the launch gap).  The weight-gradient class is `gemm_tn_w2_kernel` (27 launches) + `gemm_tn_kernel` (5 launches on
layers with < 256 input channels).

{serial}
## Kernel time per training step, default mode (second stream active)

Command: `rocprofv3 --kernel-trace --stats --output-format csv -- python3 bench.py --full --steps 10 --warmup 3 --cpu-baseline skip`
(raw: `profiles/r01_bench_kernel_stats_overlapped.csv`).  Small weight-gradient GEMMs and the AdamW of finished buckets
run on a second stream, so per-kernel durations stretch and their sum exceeds the step time.

{overl}
Timeline of one step of that run (`tools/trace_overlap.py`):

```
{overlap}
```

## HBM-side traffic (separate `--pmc FETCH_SIZE` and `--pmc WRITE_SIZE` passes, bench.py --steps 2 --warmup 1)

{fetch}
{write}
Machine-readable per-GEMM-kernel bytes: `profiles/r01_traffic.json` (read by bench.py for `roofline.traffic`; the two
weight-gradient kernels are summed under `gemm_tn_w2_kernel`).
Algorithmic minimum for comparison: AdamW 28 B x 401.6 M = 11.2 GB (measured 12.6 GB incl. the two bf16 weight copies it writes);
GEMM operands+outputs if every tensor were touched once: ~6.5 GB/step (measured ≈18 GB fetch + 3.6 GB write: tiles are re-read
from HBM/MALL 2-3x, mainly the K=95008 / N=95008 layers whose operands do not fit the 4 MiB per-XCD L2).  The 128x256
weight-gradient tiles cut that kernel class from 10.9 to 9.2 GB/step.

## SQ counters on M=3200, 5120 x 5120, 5 taps (tests/micro/gemm_bench.py {{nt,tn}} 3200 5120 5120 5)

Three `--pmc` passes (3 counters each), median over 4 launches.  `gemm_nt_wide64p_kernel` ({dur_us:.0f} µs under the tool):

```
{sq}
```
MFMA pipe busy = SQ_VALU_MFMA_BUSY_CYCLES / (1024 SIMDs x duration x 2.4 GHz) = {mf:.0f} %; LDS bank conflicts: none (XOR-swizzled
LDS-DMA layout); waves are issue-stalled (SQ_WAIT_INST_ANY) ≈55 % of their cycles, i.e. waiting on the LDS-DMA ring / LDS reads,
not on the MFMA pipe.  The same kernel before software pipelining sat at 931 TFLOP/s on this shape, the 128x128 register-staged
kernel at 33 % MFMA busy with a 33 % LDS bank-conflict rate (round start).
"""
if tn_sq:
    doc += f"""
`gemm_tn_w2_kernel` on the same shape (`tests/micro/pmc_sq.sh`, same FLOPs; un-profiled 807 µs = 1039 TFLOP/s against 1047 µs for
the 128x128 `gemm_tn_kernel` on the same box):

```
{tn_sq}
```
SQ_BUSY_CYCLES 4.01e7 against 4.97e7 for the NT kernel under the same tool: two waves per SIMD hide the stage hand-off; no
LDS bank conflicts with the chunk ^ ((row & 3) << 2) swizzle for `ds_read_b64_tr_b16`; twice the LDS instructions (64-bit
transposed reads) for the same bytes.
"""
doc += f"""
Negative results of the round (5120^2 k5, same box, wide64p = 932-942 TFLOP/s): an NT kernel in the w2 form (K-step 32, two
blocks per CU, 64-byte source rows) 791-820; an 8-wave NT kernel with two K-groups half a stage out of phase 878; two rows per
round with all loads issued first in the recon-head loss/reduce pass: 459.9 -> 459.8 µs (the pass was VALU-bound, ≈54 lane-ops per
element; what fixed it later was the instruction count: loss kind as a template parameter and `v_rcp_f32` instead of the IEEE
divide sequence, 467 -> 252 µs, now HBM-bound at 5 TB/s); L2 prefetch touches in the wide NT kernel for the K = 95 008 layers
(1014 -> 1026-1210 µs: vector-memory returns are in order); one zeroing kernel per site instead of 14 memsets (no change); four
rows per round in the bf16 `W v` pass (217 -> 243 µs); the library (hipBLASLt) on the K = 95 008 layers (1028 vs 832 µs) and on
the conditioner's weight gradients (734 vs 1095 samples/s).  All removed.  Kept from the same series of per-kernel A/B runs
(a per-kernel A/B script, removed; see git history): the library for plain one-tap GEMMs with K <= 8192 (+2.6 %), bf16 weight copy in the `W v` pass
(+1.1 %), GroupNorm statistics in the 128x128 GEMM epilogue (own-kernel path), the 16-byte split-K combine passes.

## Per-layer GEMM table (bench.py --layer-times, hipEvents, one step; top 40 by time)

```
[bench] per-layer GEMM times (one step, hipEvents incl. split-K combine passes):
{chr(10).join(layers)}
```
"""
open(os.path.join(P, "r01_summary.md"), "w").write(doc)
print("wrote profiles/r01_summary.md:", len(doc.splitlines()), "lines;", f"{b['value']:.0f} samples/s")
