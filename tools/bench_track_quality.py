#!/usr/bin/env python3
"""bench_track_quality.py -- cost of the per-sequence tracking-quality records (dvo_batch_set_track_quality).

ms per push at bench.py's shapes -- 16 384 resident raw 640x480 sensor-depth sequences (dvo_batch_push_raw_device) and 8 192 mono
sequences (dvo_batch_odometrize_raw_device, ring 8) -- in three modes, alternated round by round in one process (one batch alive at a
time): plain (quality never enabled: the bench.py path), quality (records kept, never read), quality_copy (records kept and copied to
a device buffer after every push: one k_track_quality launch per push).  Device events on the handle's stream around the timed
pushes, after a warm-up.  Prints one JSON line.

    python tools/bench_track_quality.py --steps 12 --warmup 3 --rounds 3
"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "direct-visual-odometry_amd"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import numpy as np
import torch

import dvo_amd as dvo
from dvo_amd import synth

F, W, H = 3, 640, 480
MODES = ["plain", "quality", "quality_copy"]


def frames(B, U, dev, depth):
    g8 = torch.empty((F, U, H, W), dtype=torch.uint8, device=dev)
    d16 = torch.empty((F, U, H, W), dtype=torch.int16, device=dev) if depth else None
    for u0 in range(0, U, 16):
        u1 = min(U, u0 + 16)
        Ts = np.stack([synth.trajectory(F, seed=42 + u)[f] for u in range(u0, u1) for f in range(F)])
        g, d = synth.render_batch(Ts, synth.K_640, W, H, device=dev, newton_iters=6)
        g8[:, u0:u1] = torch.clamp(torch.round(g * 255.0), 0, 255).to(torch.uint8).reshape(u1 - u0, F, H, W).permute(1, 0, 2, 3)
        if depth:
            d16[:, u0:u1] = torch.clamp(torch.round(d * 5000.0), 0, 65535).to(torch.int32).to(torch.int16).reshape(u1 - u0, F, H, W).permute(1, 0, 2, 3)
    idx = torch.arange(B, device=dev) % U
    return g8.index_select(1, idx).contiguous(), (d16.index_select(1, idx).contiguous() if depth else None)


def run(kind, mode, a, B, g8, d16, stream):
    if kind == "sensor":
        h = dvo.Batch(B, synth.K_640, W, H, 4, 1, cfg=dvo.default_config(stream=stream))
    else:
        h = dvo.MonoBatch(B, synth.K_640, W, H, ring_keyframes=8, cfg=dvo.default_config(stream=stream, rng_seed=1))
    if mode != "plain":
        h.set_track_quality(True)
    rec = torch.empty(B * C.sizeof(dvo.TrackQuality), dtype=torch.uint8, device="cuda")
    ev = []
    for k in range(1 + a.warmup + a.steps):
        f = k % F
        timed = k > a.warmup
        if timed:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
        if kind == "sensor":
            h.push_raw_device(g8[f].data_ptr(), 1, d16[f].data_ptr())
        else:
            h.odometrize_raw_device(g8[f].data_ptr(), 1)
        if mode == "quality_copy":
            h.copy_track_quality_device(rec.data_ptr())
        if timed:
            e1.record()
            ev.append((e0, e1))
    torch.cuda.synchronize()
    ms = sum(e0.elapsed_time(e1) for e0, e1 in ev) / a.steps
    h.close()
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16384)
    ap.add_argument("--mono-batch", type=int, default=8192)
    ap.add_argument("--unique", type=int, default=64)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    out = {"steps": a.steps, "warmup": a.warmup, "rounds": a.rounds}
    for kind, B in (("sensor", a.batch), ("mono", a.mono_batch)):
        g8, d16 = frames(B, a.unique, dev, kind == "sensor")
        torch.cuda.synchronize()
        res = {m: [] for m in MODES}
        for _ in range(a.rounds):
            for m in MODES:
                res[m].append(run(kind, m, a, B, g8, d16, stream))
        med = {m: float(np.median(res[m])) for m in MODES}
        out[kind] = {"batch": B, "ms_per_push": {m: round(med[m], 3) for m in MODES},
                     "all_rounds": {m: [round(x, 3) for x in res[m]] for m in MODES},
                     "vs_plain": {m: round(med[m] / med["plain"], 4) for m in MODES[1:]}}
        del g8, d16
        torch.cuda.empty_cache()
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
