#!/usr/bin/env python3
"""bench_pyramid_filter.py -- cost of the binomial-filtered gray pyramid of a sensor-depth batch (dvo_batch_set_pyramid_filter,
DESIGN.md §39).

ms per push at bench.py's shape -- resident raw 640x480 sensor-depth sequences (dvo_batch_push_raw_device), 16 384 of them unless
--batch says otherwise -- for two builds, alternated round by round in one process (one batch alive at a time): plain (the setter
never called: the bench.py path, which splits its build at this size) and filtered (DVO_PYRAMID_FILTER_BINOMIAL3:
k_pyramid_filter_top and one k_pyramid_filter_down per lower level, never split).  Device events on the handle's stream around the
timed pushes, after a warm-up.  The two estimators see different gray, so with bench.py's stop tests they stop at different
iterations; --fixed-iterations N makes every level run N iterations of every sequence, the like-for-like comparison of the builds.

--trace also runs each build once in a child process under `rocprofv3 --kernel-trace --stats` (nothing else traced) and reports
every pyramid-build kernel of the run: calls, total and average time per launch, and for the kernels that read the input the bytes
they have to read per launch -- every source byte and depth word for the filter, every 2^culls-th row and column's 32-byte sectors
for the decimating kernels, stated as whole kept rows -- with the rate that makes.  No cost is promised: the figures are against
the plain build of the same process, and the spread of the plain rounds stands beside them.  Prints one JSON line.

    python tools/bench_pyramid_filter.py --steps 8 --warmup 3 --rounds 3 --trace [--fixed-iterations 4]
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "direct-visual-odometry_amd"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import numpy as np
import torch

import dvo_amd as dvo
from dvo_amd import synth

F, W, H, LEVELS, CULLS = 3, 640, 480, 4, 1
MODES = ["plain", "filtered"]


def frames(B, U, dev):
    g8 = torch.empty((F, U, H, W), dtype=torch.uint8, device=dev)
    d16 = torch.empty((F, U, H, W), dtype=torch.int16, device=dev)
    for u0 in range(0, U, 16):
        u1 = min(U, u0 + 16)
        Ts = np.stack([synth.trajectory(F, seed=42 + u)[f] for u in range(u0, u1) for f in range(F)])
        g, d = synth.render_batch(Ts, synth.K_640, W, H, device=dev, newton_iters=6)
        g8[:, u0:u1] = torch.clamp(torch.round(g * 255.0), 0, 255).to(torch.uint8).reshape(u1 - u0, F, H, W).permute(1, 0, 2, 3)
        d16[:, u0:u1] = torch.clamp(torch.round(d * 5000.0), 0, 65535).to(torch.int32).to(torch.int16).reshape(u1 - u0, F, H, W).permute(1, 0, 2, 3)
    idx = torch.arange(B, device=dev) % U
    return g8.index_select(1, idx).contiguous(), d16.index_select(1, idx).contiguous()


def run(mode, a, B, g8, d16, stream):
    h = dvo.Batch(B, synth.K_640, W, H, LEVELS, CULLS, cfg=dvo.default_config(stream=stream, fixed_iterations=a.fixed_iterations))
    if mode == "filtered":
        h.set_pyramid_filter(dvo.PYRAMID_FILTER_BINOMIAL3)
    ev = []
    for k in range(1 + a.warmup + a.steps):
        f = k % F
        timed = k > a.warmup
        if timed:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
        h.push_raw_device(g8[f].data_ptr(), 1, d16[f].data_ptr())
        if timed:
            e1.record()
            ev.append((e0, e1))
    torch.cuda.synchronize()
    ms = sum(e0.elapsed_time(e1) for e0, e1 in ev) / a.steps
    h.close()
    return ms


def input_bytes(kernel, B):
    """the bytes of the input one launch has to read (u8 gray + u16 depth), or None for a kernel that reads no input"""
    if kernel.startswith("k_pyramid_filter_top"):
        return B * W * H * 3                       # every source pixel
    if kernel.startswith("k_pyramid_filter_down"):
        return None
    if kernel.startswith("k_pyramid_raw4_coarse"):
        return B * W * (H >> (CULLS + 1)) * 3      # the rows level top - 1 keeps, whole (the kept columns share their sectors with the dropped)
    if kernel.startswith("k_pyramid"):
        return B * W * (H >> CULLS) * 3            # the rows the top level keeps, whole
    return None


def kernel_rows(stats_csv, pushes, B):
    out = []
    for r in csv.DictReader(open(stats_csv)):
        if "dvo::k_pyramid" not in r["Name"]:
            continue
        name = r["Name"].split("dvo::", 1)[1].split("(", 1)[0]
        row = {"kernel": name, "calls": int(r["Calls"]), "total_ms": round(float(r["TotalDurationNs"]) * 1e-6, 3),
               "average_us": round(float(r["AverageNs"]) * 1e-3, 2), "ms_per_push": round(float(r["TotalDurationNs"]) * 1e-6 / pushes, 3)}
        nb = input_bytes(name, B)
        if nb is not None:
            row["input_bytes_per_launch"] = nb
            row["input_GB_per_s"] = round(nb / float(r["AverageNs"]), 1)
        out.append(row)
    return sorted(out, key=lambda x: -x["total_ms"])


def trace(mode, a):
    """one build in a fresh child process under rocprofv3 --kernel-trace --stats; the pyramid kernels' rows of its statistics"""
    with tempfile.TemporaryDirectory() as td:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", td, "--", sys.executable, os.path.abspath(__file__),
               "--child", mode, "--batch", str(a.batch), "--unique", str(a.unique), "--steps", str(a.steps), "--warmup", str(a.warmup),
               "--fixed-iterations", str(a.fixed_iterations)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("traced child failed (%d): %s" % (r.returncode, r.stderr[-2000:]))
        files = glob.glob(os.path.join(td, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            raise RuntimeError("rocprofv3 wrote no kernel statistics")
        return kernel_rows(files[0], 1 + a.warmup + a.steps, a.batch)   # (every push builds, the first one too)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16384, help="sequences held resident; lower it where the frames do not fit")
    ap.add_argument("--unique", type=int, default=64)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--fixed-iterations", type=int, default=0,
                    help="N > 0: every level runs N iterations of every sequence, so both builds are followed by the same launches; "
                         "0: bench.py's stop tests")
    ap.add_argument("--trace", action="store_true", help="also one traced child run per build (rocprofv3 --kernel-trace --stats)")
    ap.add_argument("--child", default="", help=argparse.SUPPRESS)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    g8, d16 = frames(a.batch, a.unique, dev)
    torch.cuda.synchronize()
    if a.child:
        run(a.child, a, a.batch, g8, d16, stream)
        return 0
    res = {m: [] for m in MODES}
    for _ in range(a.rounds):
        for m in MODES:
            res[m].append(run(m, a, a.batch, g8, d16, stream))
    med = {m: float(np.median(res[m])) for m in MODES}
    out = {"batch": a.batch, "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds, "fixed_iterations": a.fixed_iterations,
           "ms_per_push": {m: round(med[m], 3) for m in MODES},
           "all_rounds": {m: [round(x, 3) for x in res[m]] for m in MODES},
           "plain_spread_ms": round(max(res["plain"]) - min(res["plain"]), 3),
           "vs_plain": {"filtered": round(med["filtered"] / med["plain"], 4)}}
    del g8, d16
    torch.cuda.empty_cache()
    if a.trace:
        out["kernels"] = {m: trace(m, a) for m in MODES}
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
