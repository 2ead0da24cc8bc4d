#!/usr/bin/env python3
"""bench_lm.py -- cost of step control (dvo_batch_set_step_control).

ms per push at bench.py's shape -- 16 384 resident raw 640x480 sensor-depth sequences (dvo_batch_push_raw_device, sigma 0.1, the
reference's step constants) -- for two estimators, alternated round by round in one process (one batch alive at a time): plain
(step control never set: the bench.py path) and step_control (the defaults of dvo_lm_config_default).  Device events on the handle's
stream around the timed pushes, after a warm-up.

Two things change at once under step control: the solve's time per launch (k_gn_solve_lm against k_gn_solve) and the number of
launches (a rejected step costs an evaluation, a damped sequence converges instead of running to the cap).  --fixed-iterations N makes
every level run N evaluations of every sequence in both estimators, which isolates the first; 0 (bench.py's stop tests, free-running)
shows both.  After the timed rounds each estimator runs once more with cfg.profile = 1 and reports its tile launches and
sequence-iterations per push, and step control its accepted and rejected steps per sequence and push.  No speed is promised: the
figures are against the plain path of the same build, and the spread of the plain rounds stands beside them.  Prints one JSON line.

    python tools/bench_lm.py --steps 8 --warmup 3 --rounds 3 [--fixed-iterations 4]
"""
import argparse
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
MODES = ["plain", "step_control"]


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


def run(mode, a, B, g8, d16, stream, profile=False):
    """ms per timed push; with profile: (tile launches, sequence-iterations, accepted, rejected) per push instead"""
    h = dvo.Batch(B, synth.K_640, W, H, 4, 1, cfg=dvo.default_config(stream=stream, fixed_iterations=a.fixed_iterations, profile=1 if profile else 0))
    if mode == "step_control":
        h.set_step_control()
    ev = []
    acc = rej = 0
    for k in range(1 + a.warmup + a.steps):
        f = k % F
        timed = k > a.warmup
        if timed and profile and k == a.warmup + 1:
            h.synchronize()
            h.profile(reset=True)
        if timed and not profile:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
        h.push_raw_device(g8[f].data_ptr(), 1, d16[f].data_ptr())
        if timed and not profile:
            e1.record()
            ev.append((e0, e1))
        if timed and profile and mode == "step_control":
            rec = h.last_step_control()
            acc += int(rec["n_accepted"].sum()); rej += int(rec["n_rejected"].sum())
    torch.cuda.synchronize()
    if profile:
        p = h.profile()
        h.close()
        return dict(tile_launches_per_push=round(p["gn_launches"] / a.steps, 2), sequence_iterations_per_push=round(p["gn_iterations"] / a.steps, 1),
                    accepted_per_sequence=round(acc / a.steps / B, 3), rejected_per_sequence=round(rej / a.steps / B, 3))
    ms = sum(e0.elapsed_time(e1) for e0, e1 in ev) / a.steps
    h.close()
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16384)
    ap.add_argument("--unique", type=int, default=64)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--fixed-iterations", type=int, default=0,
                    help="N > 0: every level runs N evaluations of every sequence, so both estimators run the same launches on the same number "
                         "of sequences and the solve's per-launch time compares like for like; 0: bench.py's stop tests (free-running)")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    g8, d16 = frames(a.batch, a.unique, dev)
    torch.cuda.synchronize()
    res = {m: [] for m in MODES}
    for _ in range(a.rounds):
        for m in MODES:
            res[m].append(run(m, a, a.batch, g8, d16, stream))
    med = {m: float(np.median(res[m])) for m in MODES}
    out = {"batch": a.batch, "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds, "fixed_iterations": a.fixed_iterations,
           "ms_per_push": {m: round(med[m], 3) for m in MODES},
           "all_rounds": {m: [round(x, 3) for x in res[m]] for m in MODES},
           "plain_spread_ms": round(max(res["plain"]) - min(res["plain"]), 3),
           "vs_plain": round(med["step_control"] / med["plain"], 4),
           "launches": {m: run(m, a, a.batch, g8, d16, stream, profile=True) for m in MODES}}
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
