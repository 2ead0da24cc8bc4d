#!/usr/bin/env python3
"""bench_keyframes.py -- cost of keyframe tracking (dvo_batch_set_keyframe_tracking) on the headline batch shape.

16 384 resident raw 640x480 sequences (u8 gray + u16 depth in HBM, as bench.py and tools/bench_lifecycle.py), pushed in three modes,
alternated round by round in one process (one batch alive at a time):
  plain      dvo_batch_push_raw_device, frame-to-frame tracking (the bench.py path)
  kf         keyframe tracking with the default rule (keyframe_min_translation 0.02, keyframe_max_frames 6)
  kf1        keyframe tracking with keyframe_max_frames = 1 (every tracked frame is promoted: the copy at its most)
for two workloads: bench.py's default constants, and the converging constants (step literals halved, min_residual 0; the raw
conversion keeps sigma 0.1).  ms per push and tracked frames/s come from device events on the handle's stream around the timed pushes
(after a warm-up); the promoted fraction is the mean of is_keyframe over the timed pushes, copied on the device after each push.
Every sequence tracks at every push after the first.  Prints one JSON line.
--fusion adds two modes to the alternation (without the flag the tool runs what it always ran):
  kf_long    keyframe tracking with long-lived keyframes (keyframe_min_translation 1.0, keyframe_max_frames 8)
  kf_fused   the same with keyframe depth fusion on (dvo_batch_set_keyframe_fusion): vs_kf_long is its cost
--carry (with --fusion) adds one more:
  kf_carry   kf_fused with the keyframe carry on (dvo_batch_set_keyframe_carry): vs_kf_fused is its cost; the
             carry kernels run on the promoting pushes only (one in eight here), carried_fraction is n_carried / n_candidates of the
             last promoting push (read after the push's closing event: not timed)

    python tools/bench_keyframes.py --batch 16384 --steps 12 --warmup 3 --rounds 2 [--fusion [--carry]]
"""
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

WORKLOADS = {"default": {}, "converging": dict(step_default=1.0, step_level1=0.75, step_level2=0.5, min_residual=0.0)}
MODES = {"plain": None, "kf": {}, "kf1": dict(keyframe_max_frames=1)}
LONG = dict(keyframe_min_translation=1.0, keyframe_max_frames=8)
FUSION_MODES = {"kf_long": dict(LONG), "kf_fused": dict(LONG)}
CARRY_MODES = {"kf_carry": dict(LONG)}


def run(workload, mode, a, g8, d16, stream):
    B = a.batch
    kw = dict(WORKLOADS[workload])
    kf = MODES[mode]
    if kf is not None:
        kw.update(kf)
    bt = dvo.Batch(B, synth.K_640, W, H, 4, 1, cfg=dvo.default_config(stream=stream, **kw))
    if kf is not None:
        bt.set_keyframe_tracking(True)
    if mode in ("kf_fused", "kf_carry"):
        bt.set_keyframe_fusion()
    if mode == "kf_carry":
        bt.set_keyframe_carry()
    carried = None
    key = torch.zeros((a.steps, B), dtype=torch.int32, device="cuda")
    ev = []
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
            if kf is not None:   # (after the event: the copy is not timed)
                bt.copy_world_poses_device(0, 0, key[k - a.warmup - 1].data_ptr())
            if mode == "kf_carry":
                rec = bt.last_keyframe_carry()
                if rec["n_candidates"].any():
                    carried = float(rec["n_carried"].sum()) / float(rec["n_candidates"].sum())
    torch.cuda.synchronize()
    ms = sum(e0.elapsed_time(e1) for e0, e1 in ev)
    xi, _ = bt.last_poses()
    fused = None
    if mode == "kf_fused":   # (of the last push)
        rec = bt.last_keyframe_fusion()
        fused = float(rec["n_fused"].sum()) / max(float(rec["n_candidates"].sum()), 1.0)
    bt.close()
    assert np.all(np.isfinite(xi)), "non-finite poses"
    return {"ms_per_push": ms / a.steps, "tracked_frames_per_s": B * a.steps / (ms / 1e3),
            "promoted_fraction": float(key.float().mean().item()) if kf is not None else None, "fused_fraction_last_push": fused,
            "carried_fraction": carried}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16384)
    ap.add_argument("--unique", type=int, default=64, help="distinct synthetic sequences tiled over the batch")
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--workloads", default="default,converging")
    ap.add_argument("--fusion", action="store_true", help="also alternate kf_long and kf_fused (keyframe depth fusion)")
    ap.add_argument("--carry", action="store_true", help="with --fusion: also alternate kf_carry (keyframe carry)")
    a = ap.parse_args()
    if a.carry and not a.fusion:
        ap.error("--carry needs --fusion")
    if a.fusion:
        MODES.update(FUSION_MODES)
    if a.carry:
        MODES.update(CARRY_MODES)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    g8, d16 = frames(a.batch, a.unique, dev)
    torch.cuda.synchronize()
    wls = a.workloads.split(",")
    res = {(w, m): [] for w in wls for m in MODES}
    for r in range(a.rounds):
        for w in wls:
            for m in MODES:
                res[(w, m)].append(run(w, m, a, g8, d16, stream))
    summary = {}
    for w in wls:
        summary[w] = {}
        for m in MODES:
            rs = res[(w, m)]
            ms = sorted(x["ms_per_push"] for x in rs)
            s = {"ms_per_push": round(ms[len(ms) // 2], 3), "ms_per_push_all_rounds": [round(x["ms_per_push"], 3) for x in rs],
                 "tracked_frames_per_s": round(float(np.median([x["tracked_frames_per_s"] for x in rs])), 1)}
            if rs[0]["promoted_fraction"] is not None:
                s["promoted_fraction"] = round(float(np.median([x["promoted_fraction"] for x in rs])), 4)
            summary[w][m] = s
        base = summary[w]["plain"]["ms_per_push"]
        for m in ("kf", "kf1"):
            summary[w][m]["vs_plain"] = round(summary[w][m]["ms_per_push"] / base, 4)
        if a.fusion:
            for m in FUSION_MODES:
                summary[w][m]["vs_plain"] = round(summary[w][m]["ms_per_push"] / base, 4)
            summary[w]["kf_fused"]["vs_kf_long"] = round(summary[w]["kf_fused"]["ms_per_push"] / summary[w]["kf_long"]["ms_per_push"], 4)
            summary[w]["kf_fused"]["fused_fraction_last_push"] = res[(w, "kf_fused")][-1]["fused_fraction_last_push"]
        if a.carry:
            summary[w]["kf_carry"]["vs_plain"] = round(summary[w]["kf_carry"]["ms_per_push"] / base, 4)
            summary[w]["kf_carry"]["vs_kf_fused"] = round(summary[w]["kf_carry"]["ms_per_push"] / summary[w]["kf_fused"]["ms_per_push"], 4)
            summary[w]["kf_carry"]["carried_fraction"] = res[(w, "kf_carry")][-1]["carried_fraction"]
    print(json.dumps({"batch": a.batch, "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds, "frames_per_sequence": F,
                      "workloads": summary}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
