#!/usr/bin/env python3
"""bench_points.py -- what dvo_batch_export_points costs.

A mono batch and a sensor-depth keyframe batch of --batch resident raw 640x480 sequences (bench_lifecycle.frames), three frames
each; then the export at the top level and at level 0, --rounds rounds of --reps calls in one process, microseconds per call from device
events on the handle's stream (the median of the rounds).  Bytes moved per call: the planes both passes read (depth twice; gray, and
for mono sigma, once for every exported point, counted as whole planes when every pixel is exported) plus the points written
(16 B, + 4 B src, + 4 B sigma), plus the chunk counts.  The yardstick is a device-to-device hipMemcpyAsync of the same byte count
(read + write = that count), timed in the same run with the same events.

    python tools/bench_points.py [--batch 4096] [--rounds 5] [--reps 10]            one JSON line"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "direct-visual-odometry_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np
import torch

import dvo_amd as dvo
from dvo_amd import synth
from bench_lifecycle import F, H, W, frames


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def measure(bt, mono, level, plane, a, copy_src, copy_dst):
    B = bt.n_seq
    off = torch.empty(B + 1, dtype=torch.int32, device="cuda")
    cfg = dvo.points_config(level=level)
    torch.cuda.synchronize()
    bt.export_points(cfg, 0, 0, 0, 0, off.data_ptr())
    total = int(bt.last_points()[-1])
    xyzg = torch.empty((max(total, 1), 4), dtype=torch.float32, device="cuda")
    src = torch.empty(max(total, 1), dtype=torch.int32, device="cuda")
    sig = torch.empty(max(total, 1), dtype=torch.float32, device="cuda") if mono else None
    torch.cuda.synchronize()
    full = lambda: bt.export_points(cfg, total, xyzg.data_ptr(), src.data_ptr(), sig.data_ptr() if mono else 0, off.data_ptr())
    count = lambda: bt.export_points(cfg, 0, 0, 0, 0, off.data_ptr())
    pixels = B * plane
    frac = total / pixels
    chunks = B * ((plane + 1023) // 1024)
    read = pixels * 4 * 2 + int(pixels * 4 * frac) * (2 if mono else 1) + chunks * 4 * 2
    written = total * (16 + 4 + (4 if mono else 0)) + chunks * 4
    moved = read + written
    n_copy = min(moved // 2, copy_src.numel())
    copy = lambda: copy_dst[:n_copy].copy_(copy_src[:n_copy], non_blocking=True)
    for fn in (full, count, copy):      # warm
        timed(fn, 2)
    us = {"export": [], "count_only": [], "copy": []}
    for _ in range(a.rounds):
        us["export"].append(timed(full, a.reps))
        us["count_only"].append(timed(count, a.reps))
        us["copy"].append(timed(copy, a.reps))
    med = {k: float(np.median(v)) for k, v in us.items()}
    return {"level": level, "plane_pixels": plane, "points": total, "exported_fraction": round(frac, 4), "bytes_moved": moved,
            "copy_bytes_moved": int(n_copy) * 2,
            "us_export": round(med["export"], 1), "us_count_only": round(med["count_only"], 1), "us_copy": round(med["copy"], 1),
            "gbps_export": round(moved / med["export"] / 1e3, 1), "gbps_copy": round(n_copy * 2 / med["copy"] / 1e3, 1),
            "fraction_of_copy": round((moved / med["export"]) / (n_copy * 2 / med["copy"]), 3),
            "us_export_rounds": [round(x, 1) for x in us["export"]]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--unique", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream     # (one stream: the events above bracket the handle's work)
    g8, d16 = frames(a.batch, a.unique, dev)
    B = a.batch
    out = {"batch": B, "rounds": a.rounds, "reps": a.reps, "mono": [], "sensor": []}
    biggest = B * (W // 2) * (H // 2) * 32     # (the sensor-depth top level with every pixel exported: 32 B per pixel)
    copy_src = torch.empty(biggest // 2, dtype=torch.uint8, device=dev)
    copy_dst = torch.empty(biggest // 2, dtype=torch.uint8, device=dev)
    mb = dvo.MonoBatch(B, synth.K_640, W, H, cfg=dvo.default_config(stream=stream))
    for f in range(F):
        mb.odometrize_raw_device(g8[f].data_ptr(), 1)
    torch.cuda.synchronize()
    for level, sh in ((2, 0), (0, 2)):
        out["mono"].append(measure(mb, True, level, ((W // 4) >> sh) * ((H // 4) >> sh), a, copy_src, copy_dst))
    mb.close()
    bt = dvo.Batch(B, synth.K_640, W, H, 4, 1, cfg=dvo.default_config(stream=stream))
    bt.set_keyframe_tracking(True)
    for f in range(F):
        bt.push_raw_device(g8[f].data_ptr(), 1, d16[f].data_ptr())
    torch.cuda.synchronize()
    for level, sh in ((3, 0), (0, 3)):
        out["sensor"].append(measure(bt, False, level, ((W // 2) >> sh) * ((H // 2) >> sh), a, copy_src, copy_dst))
    bt.close()
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
