#!/usr/bin/env python3
"""bench_mono_lifecycle.py -- cost of per-sequence skip / restart on a mono batch (dvo_batch_set_mono_actions), bench.py's mono shape.

8 192 resident raw 640x480 sequences (u8 gray in HBM, as bench.py's mono leg: dvo_batch_create_mono, ring 8, rng_seed 1), run in four
modes, alternated round by round in one process (one batch alive at a time):
  plain      dvo_batch_odometrize_raw_device, no actions (the bench.py path)
  track      every call with all-TRACK actions (k_plan, the plan kernels of the mapping)
  skip0.1    10 % of the sequences skipped per call, 1 % restarted, the rest tracked
  skip0.5    50 % skipped, 1 % restarted
ms per call and consumed frames/s (tracked + started) come from device events on the handle's stream around the timed calls (after
a warm-up).  The world poses of the all-TRACK mode are checked bit for bit against the plain mode at every timed call.  Prints one
JSON line.

    python tools/bench_mono_lifecycle.py --batch 8192 --steps 12 --warmup 3 --rounds 2
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


def actions(rng, B, skip, restart):
    r = rng.uniform(size=B)
    a = np.full(B, dvo.SEQ_TRACK, np.uint8)
    a[r < skip] = dvo.SEQ_SKIP
    a[(r >= skip) & (r < skip + restart)] = dvo.SEQ_RESTART
    return a


def run(mode, a, g8, stream, seed):
    B = a.batch
    skip = {"plain": None, "track": 0.0, "skip0.1": 0.1, "skip0.5": 0.5}[mode]
    rng = np.random.RandomState(seed)
    mb = dvo.MonoBatch(B, synth.K_640, W, H, ring_keyframes=8, cfg=dvo.default_config(stream=stream, rng_seed=1))
    ev, poses = [], []
    consumed = 0
    n = 1 + a.warmup + a.steps
    for k in range(n):
        f = k % F
        acts = None
        if skip is not None:
            acts = actions(rng, B, skip, 0.01 if skip > 0 else 0.0) if k > 0 else np.full(B, dvo.SEQ_TRACK, np.uint8)
        timed = k > a.warmup
        if timed:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
        if acts is not None:
            mb.set_actions(acts)
        mb.odometrize_raw_device(g8[f].data_ptr(), 1)
        if timed:
            e1.record()
            ev.append((e0, e1))
            consumed += B if acts is None else int(((acts == dvo.SEQ_TRACK) | (acts == dvo.SEQ_RESTART)).sum())
            T = mb.world_poses()[1]   # (synchronises, in every mode alike: outside the events of the next call)
            if mode in ("plain", "track"):
                poses.append(T.copy())
    torch.cuda.synchronize()
    ms = sum(e0.elapsed_time(e1) for e0, e1 in ev)
    mb.close()
    return {"ms_per_call": ms / a.steps, "consumed_frames_per_s": consumed / (ms / 1e3), "consumed_per_call": consumed / a.steps}, poses


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--unique", type=int, default=64, help="distinct synthetic sequences tiled over the batch")
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    g8 = frames(a.batch, a.unique, dev)
    torch.cuda.synchronize()
    modes = ["plain", "track", "skip0.1", "skip0.5"]
    res = {m: [] for m in modes}
    mismatches, compared = 0, 0
    for r in range(a.rounds):
        plain = None
        for m in modes:
            out, poses = run(m, a, g8, stream, seed=100 * r + modes.index(m))
            res[m].append(out)
            if m == "plain":
                plain = poses
            elif m == "track":
                for x, y in zip(plain, poses):
                    same = np.all((x == y).reshape(a.batch, -1), axis=1)
                    mismatches += int((~same).sum()); compared += a.batch
    summary = {}
    for m in modes:
        ms = sorted(x["ms_per_call"] for x in res[m])
        summary[m] = {"ms_per_call": round(ms[len(ms) // 2], 3), "ms_per_call_all_rounds": [round(x["ms_per_call"], 3) for x in res[m]],
                      "consumed_frames_per_s": round(float(np.median([x["consumed_frames_per_s"] for x in res[m]])), 1),
                      "consumed_per_call": res[m][0]["consumed_per_call"]}
    base = summary["plain"]["ms_per_call"]
    for m in modes[1:]:
        summary[m]["vs_plain"] = round(summary[m]["ms_per_call"] / base, 4)
    print(json.dumps({"batch": a.batch, "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds, "modes": summary,
                      "pose_check": {"compared": compared, "mismatches": mismatches}}))
    return 0 if mismatches == 0 and compared > 0 else 1


if __name__ == "__main__":
    sys.exit(main())
