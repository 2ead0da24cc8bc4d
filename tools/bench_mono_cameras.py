#!/usr/bin/env python3
"""bench_mono_cameras.py -- cost of per-sequence camera intrinsics on a mono batch (dvo_batch_create_mono_cameras).

8 192 resident raw 640x480 mono sequences (u8 gray in HBM, as bench.py's mono leg), run in three modes, alternated round by round in
one process (one batch alive at a time):
  plain      dvo_batch_create_mono with synth.K_640 (the bench.py path: k_track_gn, k_propagate_owner, k_depth_update)
  uniform    dvo_batch_create_mono_cameras with K_640 for every sequence (the per-camera kernels: k_track_gn_cam,
             k_propagate_owner_cam, k_depth_update_cam)
  four       four distinct cameras (synth.K_640, TUM fr1, TUM fr3, fx = fy = 400), sequence q on camera q % 4
The frames are rendered with synth.K_640 in every mode: the table changes what the kernels compute, not how much.  ms per frame
comes from device events on the handle's stream around the timed frames (after a warm-up).  Pose check: the uniform mode's world
poses of every timed frame must equal the plain mode's bit for bit.  Prints one JSON line.

    python tools/bench_mono_cameras.py --batch 8192 --steps 12 --warmup 3 --rounds 2
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

F, W, H = 6, 640, 480
CAMS = [synth.K_640,
        np.array([[517.3, 0, 318.6], [0, 516.5, 255.3], [0, 0, 1]], np.float32),
        np.array([[535.4, 0, 320.1], [0, 539.2, 247.6], [0, 0, 1]], np.float32),
        np.array([[400.0, 0, 300.0], [0, 400.0, 260.0], [0, 0, 1]], np.float32)]


def frames(B, U, dev):
    """U distinct synthetic sequences of F frames, tiled over B slots: u8 gray [F][B][H][W]"""
    g8 = torch.empty((F, U, H, W), dtype=torch.uint8, device=dev)
    for u0 in range(0, U, 16):
        u1 = min(U, u0 + 16)
        Ts = np.stack([synth.trajectory(F, seed=42 + u)[f] for u in range(u0, u1) for f in range(F)])
        g, _ = synth.render_batch(Ts, synth.K_640, W, H, device=dev, newton_iters=6)
        g8[:, u0:u1] = torch.clamp(torch.round(g * 255.0), 0, 255).to(torch.uint8).reshape(u1 - u0, F, H, W).permute(1, 0, 2, 3)
    idx = torch.arange(B, device=dev) % U
    return g8.index_select(1, idx).contiguous()


def run(mode, a, g8, stream):
    B = a.batch
    cfg = dvo.default_config(stream=stream, rng_seed=1)
    if mode == "plain":
        mb = dvo.MonoBatch(B, synth.K_640, W, H, cfg=cfg)
    elif mode == "uniform":
        mb = dvo.MonoBatch(B, np.broadcast_to(synth.K_640, (B, 3, 3)), W, H, cfg=cfg, per_sequence_K=True)
    else:
        mb = dvo.MonoBatch(B, np.stack([CAMS[q % 4] for q in range(B)]), W, H, cfg=cfg, per_sequence_K=True)
    ev, poses = [], []
    n = 1 + a.warmup + a.steps
    xi_dev = torch.zeros((a.steps, B, 6), dtype=torch.float32, device="cuda")
    for k in range(n):
        timed = k > a.warmup
        if timed:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
        mb.odometrize_raw_device(g8[k % F].data_ptr(), 1)
        if timed:
            e1.record()
            ev.append((e0, e1))
            mb.copy_world_poses_device(xi_dev[k - a.warmup - 1].data_ptr())   # (after the frame's end event)
    torch.cuda.synchronize()
    ms = sum(e0.elapsed_time(e1) for e0, e1 in ev)
    mb.close()
    return {"ms_per_frame": ms / a.steps, "frames_per_s": B * a.steps / (ms / 1e3)}, xi_dev.cpu().numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--unique", type=int, default=64, help="distinct synthetic sequences tiled over the batch")
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--modes", default="plain,uniform,four", help="comma-separated subset of plain, uniform, four")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    g8 = frames(a.batch, a.unique, dev)
    torch.cuda.synchronize()
    modes = a.modes.split(",")
    res = {m: [] for m in modes}
    plain_xi = None
    mismatches, compared = 0, 0
    for r in range(a.rounds):
        for m in modes:
            out, xi = run(m, a, g8, stream)
            res[m].append(out)
            if m == "plain":
                plain_xi = xi
            elif m == "uniform" and plain_xi is not None:
                mismatches += int((~np.all(xi == plain_xi, axis=2)).sum()); compared += xi.shape[0] * xi.shape[1]
    summary = {}
    for m in modes:
        ms = sorted(x["ms_per_frame"] for x in res[m])
        summary[m] = {"ms_per_frame": round(ms[len(ms) // 2], 3), "ms_per_frame_all_rounds": [round(x["ms_per_frame"], 3) for x in res[m]],
                      "frames_per_s": round(float(np.median([x["frames_per_s"] for x in res[m]])), 1)}
    if "plain" in summary:
        for m in modes:
            if m != "plain":
                summary[m]["vs_plain"] = round(summary[m]["ms_per_frame"] / summary["plain"]["ms_per_frame"], 4)
    print(json.dumps({"batch": a.batch, "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds, "modes": summary,
                      "pose_check_uniform_vs_plain": {"compared": compared, "mismatches": mismatches}}))
    return 0 if mismatches == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
