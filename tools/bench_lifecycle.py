#!/usr/bin/env python3
"""bench_lifecycle.py -- cost of per-sequence skip / restart (dvo_batch_set_actions) on the headline batch shape.

16 384 resident raw 640x480 sequences (u8 gray + u16 depth in HBM, as bench.py), pushed in four modes, alternated round by round in
one process (one batch alive at a time):
  plain      dvo_batch_push_raw_device, no actions (the bench.py path)
  track      every push with all-TRACK actions (k_plan + the plan's lists on each level's first iteration)
  skip0.1    10 % of the sequences skipped per push, 1 % restarted, the rest tracked
  skip0.5    50 % skipped, 1 % restarted
ms per push and tracked frames/s come from device events on the handle's stream around the timed pushes (after a warm-up).  The
tracked sequences' poses of the action modes are checked against the plain run wherever their (frame, reference) pair is the pair
the plain run tracked at the same step.  Prints one JSON line.

    python tools/bench_lifecycle.py --batch 16384 --steps 12 --warmup 3 --rounds 2
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


def actions(rng, B, skip, restart):
    r = rng.uniform(size=B)
    a = np.full(B, dvo.SEQ_TRACK, np.uint8)
    a[r < skip] = dvo.SEQ_SKIP
    a[(r >= skip) & (r < skip + restart)] = dvo.SEQ_RESTART
    return a


def run(mode, a, g8, d16, stream, seed):
    B = a.batch
    skip = {"plain": None, "track": 0.0, "skip0.1": 0.1, "skip0.5": 0.5}[mode]
    rng = np.random.RandomState(seed)
    bt = dvo.Batch(B, synth.K_640, W, H, 4, 1, cfg=dvo.default_config(stream=stream))
    ref = np.full(B, -1)                     # reference frame of every sequence (host model of the actions)
    ev = []
    tracked = 0
    checks = []
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
            bt.set_actions(acts)
        bt.push_raw_device(g8[f].data_ptr(), 1, d16[f].data_ptr())
        if timed:
            e1.record()
            ev.append((e0, e1))
        if acts is None:
            trk = np.ones(B, bool) if k > 0 else np.zeros(B, bool)
            pair_ok = trk
            ref[:] = f
        else:
            on = (acts == dvo.SEQ_TRACK) | (acts == dvo.SEQ_RESTART)
            trk = (acts == dvo.SEQ_TRACK) & (ref >= 0)
            pair_ok = trk & (ref == (k - 1) % F)
            ref[on] = f
        if timed:
            tracked += int(trk.sum())
        if k >= n - F:   # the last F pushes: poses for the cross-mode check (outside the timed pushes' events)
            checks.append((k, bt.last_poses()[0].copy(), pair_ok.copy(), bt.last_status() if acts is not None else None, trk.copy()))
    torch.cuda.synchronize()
    ms = sum(e0.elapsed_time(e1) for e0, e1 in ev)
    bt.close()
    return {"ms_per_push": ms / a.steps, "tracked_frames_per_s": tracked / (ms / 1e3), "tracked_per_push": tracked / a.steps}, checks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16384)
    ap.add_argument("--unique", type=int, default=64, help="distinct synthetic sequences tiled over the batch")
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    g8, d16 = frames(a.batch, a.unique, dev)
    torch.cuda.synchronize()
    modes = ["plain", "track", "skip0.1", "skip0.5"]
    res = {m: [] for m in modes}
    plain_xi = {}
    mismatches, compared = 0, 0
    for r in range(a.rounds):
        for m in modes:
            out, checks = run(m, a, g8, d16, stream, seed=100 * r + modes.index(m))
            res[m].append(out)
            for k, xi, ok, st, trk in checks:
                if m == "plain":
                    plain_xi[k] = xi
                elif k in plain_xi:
                    assert st is not None and np.array_equal(st == dvo.SEQ_TRACKED, trk), "status disagrees with the host model"
                    same = np.all(xi[ok] == plain_xi[k][ok], axis=1)
                    mismatches += int((~same).sum()); compared += int(ok.sum())
    summary = {}
    for m in modes:
        ms = sorted(x["ms_per_push"] for x in res[m])
        summary[m] = {"ms_per_push": round(ms[len(ms) // 2], 3), "ms_per_push_all_rounds": [round(x["ms_per_push"], 3) for x in res[m]],
                      "tracked_frames_per_s": round(float(np.median([x["tracked_frames_per_s"] for x in res[m]])), 1),
                      "tracked_per_push": res[m][0]["tracked_per_push"]}
    base = summary["plain"]["ms_per_push"]
    for m in modes[1:]:
        summary[m]["vs_plain"] = round(summary[m]["ms_per_push"] / base, 4)
    print(json.dumps({"batch": a.batch, "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds, "modes": summary,
                      "pose_check": {"compared": compared, "mismatches": mismatches}}))
    return 0 if mismatches == 0 and compared > 0 else 1


if __name__ == "__main__":
    sys.exit(main())
