#!/usr/bin/env python3
"""bench_robust.py -- cost of robust residual weights (dvo_batch_set_robust_weights).

ms per push at bench.py's shape -- 16 384 resident raw 640x480 sensor-depth sequences (dvo_batch_push_raw_device) -- for three
estimators, alternated round by round in one process (one batch alive at a time): plain (weights never set: the bench.py path),
huber (k = 1.345) and student_t (nu = 5), both with the adaptive scale.  Device events on the handle's stream around the timed
pushes, after a warm-up.  With bench.py's stop tests the estimators stop at different iterations (the min_residual test sees the
weighted mean square), so a push does not run the same launches in each; --fixed-iterations N makes every level run N iterations of
every sequence, which is the like-for-like comparison.

--trace also runs each estimator once in a child process under `rocprofv3 --kernel-trace --stats` (nothing else traced) and reports
the finest level's kernel -- k_track_gn<4, 2, false, true> against k_track_gn_rw<4, 2, true> -- and the solve (k_gn_solve against
k_gn_solve_rw): calls, total and average time per launch.  No cost is promised: the figures are against the plain kernel of the same
build, and the spread of the plain rounds stands beside them.  Prints one JSON line.

--median adds a fourth series, huber_median: Huber with the median (MAD) scale (dvo_batch_set_robust_median), whose
finest-level kernel is k_track_gn_md<4, 2, true> and whose solve is k_gn_solve_md; its push also holds the priming pair.  The
series' figures stand against huber's (k_track_gn_rw / k_gn_solve_rw of the same build), and the spread of the huber rounds is
reported beside them.  Without the flag the tool runs what it always ran.

    python tools/bench_robust.py --steps 8 --warmup 3 --rounds 3 --trace [--fixed-iterations 4] [--median]
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

F, W, H = 3, 640, 480
MODES = ["plain", "huber", "student_t"]
ROBUST = {"huber": (dvo.ROBUST_HUBER, 1.345), "student_t": (dvo.ROBUST_STUDENT_T, 5.0), "huber_median": (dvo.ROBUST_HUBER, 1.345)}
MEDIAN = "huber_median"
FINEST = {"plain": "dvo::k_track_gn<4, 2, false, true>(", "huber": "dvo::k_track_gn_rw<4, 2, true>(", "student_t": "dvo::k_track_gn_rw<4, 2, true>("}
FINEST[MEDIAN] = "dvo::k_track_gn_md<4, 2, true>("
SOLVE = {"plain": "dvo::k_gn_solve(", "huber": "dvo::k_gn_solve_rw(", "student_t": "dvo::k_gn_solve_rw("}


SOLVE[MEDIAN] = "dvo::k_gn_solve_md("


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
    h = dvo.Batch(B, synth.K_640, W, H, 4, 1, cfg=dvo.default_config(stream=stream, fixed_iterations=a.fixed_iterations))
    if mode == MEDIAN:
        h.set_robust_median(ROBUST[mode][0], ROBUST[mode][1], a.scale_floor)
    elif mode != "plain":
        kind, param = ROBUST[mode]
        h.set_robust_weights(kind, param, dvo.ROBUST_SCALE_ADAPTIVE, a.scale_floor)
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


def kernel_rows(stats_csv, mode, pushes):
    out = {}
    for r in csv.DictReader(open(stats_csv)):
        for key, pat in (("finest_level", FINEST[mode]), ("solve", SOLVE[mode])):
            if pat in r["Name"]:
                out[key] = {"kernel": r["Name"].split("dvo::", 1)[1].split("(", 1)[0], "calls": int(r["Calls"]),
                            "total_ms": round(float(r["TotalDurationNs"]) * 1e-6, 3), "average_us": round(float(r["AverageNs"]) * 1e-3, 2),
                            "ms_per_push": round(float(r["TotalDurationNs"]) * 1e-6 / pushes, 3)}
    return out


def trace(mode, a):
    """one estimator in a fresh child process under rocprofv3 --kernel-trace --stats; the kernel rows of its statistics"""
    with tempfile.TemporaryDirectory() as td:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", td, "--", sys.executable, os.path.abspath(__file__),
               "--child", mode, "--batch", str(a.batch), "--unique", str(a.unique), "--steps", str(a.steps), "--warmup", str(a.warmup),
               "--scale-floor", str(a.scale_floor), "--fixed-iterations", str(a.fixed_iterations)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("traced child failed (%d): %s" % (r.returncode, r.stderr[-2000:]))
        files = glob.glob(os.path.join(td, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            raise RuntimeError("rocprofv3 wrote no kernel statistics")
        return kernel_rows(files[0], mode, a.warmup + a.steps)   # (the first push tracks nothing)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16384)
    ap.add_argument("--unique", type=int, default=64)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--scale-floor", type=float, default=1e-3)
    ap.add_argument("--fixed-iterations", type=int, default=0,
                    help="N > 0: every level runs N iterations of every sequence, so the three estimators run the same launches on the same "
                         "number of sequences and the per-launch times compare like for like; 0: bench.py's stop tests")
    ap.add_argument("--trace", action="store_true", help="also one traced child run per estimator (rocprofv3 --kernel-trace --stats)")
    ap.add_argument("--median", action="store_true", help="a fourth series: Huber with the median (MAD) scale (dvo_batch_set_robust_median)")
    ap.add_argument("--child", default="", help=argparse.SUPPRESS)
    a = ap.parse_args()
    modes = MODES + ([MEDIAN] if a.median else [])
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    g8, d16 = frames(a.batch, a.unique, dev)
    torch.cuda.synchronize()
    if a.child:
        run(a.child, a, a.batch, g8, d16, stream)
        return 0
    res = {m: [] for m in modes}
    for _ in range(a.rounds):
        for m in modes:
            res[m].append(run(m, a, a.batch, g8, d16, stream))
    med = {m: float(np.median(res[m])) for m in modes}
    out = {"batch": a.batch, "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds, "fixed_iterations": a.fixed_iterations,
           "ms_per_push": {m: round(med[m], 3) for m in modes},
           "all_rounds": {m: [round(x, 3) for x in res[m]] for m in modes},
           "plain_spread_ms": round(max(res["plain"]) - min(res["plain"]), 3),
           "vs_plain": {m: round(med[m] / med["plain"], 4) for m in modes[1:]}}
    if a.median:
        out["huber_spread_ms"] = round(max(res["huber"]) - min(res["huber"]), 3)
        out["median_vs_huber"] = round(med[MEDIAN] / med["huber"], 4)
    del g8, d16
    torch.cuda.empty_cache()
    if a.trace:
        out["kernels"] = {m: trace(m, a) for m in modes}
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
