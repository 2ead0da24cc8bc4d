#!/usr/bin/env python3
"""bench_cameras.py -- cost of per-sequence camera intrinsics (dvo_batch_set_intrinsics) on the headline batch shape.

16 384 resident raw 640x480 sequences (u8 gray + u16 depth in HBM, as bench.py), pushed in three modes, alternated round by round in
one process (one batch alive at a time):
  plain      dvo_batch_push_raw_device, no intrinsics table (the bench.py path: k_track_gn)
  uniform    a per-sequence table equal to the creation K for every sequence (the per-sequence path: k_plan, k_track_gn_cam)
  four       four distinct cameras (synth.K_640, TUM fr1, TUM fr3, fx = fy = 400), sequence q on camera q % 4
The frames are rendered with synth.K_640 in every mode: the table changes what the kernels compute, not how much.  ms per push and
tracked frames/s come from device events on the handle's stream around the timed pushes (after a warm-up).  Pose check: the
uniform mode's poses of the last pushes must equal the plain mode's bit for bit.  Prints one JSON line.

    python tools/bench_cameras.py --batch 16384 --steps 12 --warmup 3 --rounds 2
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "direct-visual-odometry_amd"))

import numpy as np
import torch

import dvo_amd as dvo
from dvo_amd import synth

F, W, H = 3, 640, 480
CAMS = [synth.K_640,
        np.array([[517.3, 0, 318.6], [0, 516.5, 255.3], [0, 0, 1]], np.float32),
        np.array([[535.4, 0, 320.1], [0, 539.2, 247.6], [0, 0, 1]], np.float32),
        np.array([[400.0, 0, 300.0], [0, 400.0, 260.0], [0, 0, 1]], np.float32)]


def frames(B, U, dev):
    """U distinct synthetic sequences of F frames, tiled over B slots: u8 gray [F][B][H][W], u16 depth (as int16) [F][B][H][W]"""
    g8 = torch.empty((F, U, H, W), dtype=torch.uint8, device=dev)
    d16 = torch.empty((F, U, H, W), dtype=torch.int16, device=dev)
    for u0 in range(0, U, 16):
        u1 = min(U, u0 + 16)
        trajs = [synth.trajectory(F, seed=42 + u) for u in range(u0, u1)]
        Ts = np.stack([p[f] for p in trajs for f in range(F)])
        g, d = synth.render_batch(Ts, synth.K_640, W, H, device=dev, newton_iters=6)
        g8[:, u0:u1] = torch.clamp(torch.round(g * 255.0), 0, 255).to(torch.uint8).reshape(u1 - u0, F, H, W).permute(1, 0, 2, 3)
        d16[:, u0:u1] = torch.clamp(torch.round(d * 5000.0), 0, 65535).to(torch.int32).to(torch.int16).reshape(u1 - u0, F, H, W).permute(1, 0, 2, 3)
    idx = torch.arange(B, device=dev) % U
    return g8.index_select(1, idx).contiguous(), d16.index_select(1, idx).contiguous()


def run(mode, a, g8, d16, stream):
    B = a.batch
    bt = dvo.Batch(B, synth.K_640, W, H, 4, 1, cfg=dvo.default_config(stream=stream))
    if mode == "uniform":
        bt.set_intrinsics(np.broadcast_to(synth.K_640, (B, 3, 3)))
    elif mode == "four":
        bt.set_intrinsics(np.stack([CAMS[q % 4] for q in range(B)]))
    ev = []
    checks = []
    n = 1 + a.warmup + a.steps
    for k in range(n):
        f = k % F
        timed = k > a.warmup
        if timed:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
        bt.push_raw_device(g8[f].data_ptr(), 1, d16[f].data_ptr())
        if timed:
            e1.record()
            ev.append((e0, e1))
        if k >= n - F:   # the last F pushes: poses for the cross-mode check (outside the timed pushes' events)
            checks.append((k, bt.last_poses()[0].copy()))
    torch.cuda.synchronize()
    ms = sum(e0.elapsed_time(e1) for e0, e1 in ev)
    bt.close()
    return {"ms_per_push": ms / a.steps, "tracked_frames_per_s": B * a.steps / (ms / 1e3)}, checks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16384)
    ap.add_argument("--unique", type=int, default=64, help="distinct synthetic sequences tiled over the batch")
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--modes", default="plain,uniform,four", help="comma-separated subset of plain, uniform, four")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    g8, d16 = frames(a.batch, a.unique, dev)
    torch.cuda.synchronize()
    modes = a.modes.split(",")
    res = {m: [] for m in modes}
    plain_xi = {}
    mismatches, compared = 0, 0
    for r in range(a.rounds):
        for m in modes:
            out, checks = run(m, a, g8, d16, stream)
            res[m].append(out)
            for k, xi in checks:
                if m == "plain":
                    plain_xi[k] = xi
                elif m == "uniform" and k in plain_xi:
                    mismatches += int((~np.all(xi == plain_xi[k], axis=1)).sum()); compared += xi.shape[0]
    summary = {}
    for m in modes:
        ms = sorted(x["ms_per_push"] for x in res[m])
        summary[m] = {"ms_per_push": round(ms[len(ms) // 2], 3), "ms_per_push_all_rounds": [round(x["ms_per_push"], 3) for x in res[m]],
                      "tracked_frames_per_s": round(float(np.median([x["tracked_frames_per_s"] for x in res[m]])), 1)}
    if "plain" in summary:
        for m in modes:
            if m != "plain":
                summary[m]["vs_plain"] = round(summary[m]["ms_per_push"] / summary["plain"]["ms_per_push"], 4)
    print(json.dumps({"batch": a.batch, "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds, "modes": summary,
                      "pose_check_uniform_vs_plain": {"compared": compared, "mismatches": mismatches}}))
    return 0 if mismatches == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
