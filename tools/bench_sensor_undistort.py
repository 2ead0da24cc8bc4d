#!/usr/bin/env python3
"""bench_sensor_undistort.py -- cost of the lens undistortion fused into the sensor-depth batch (dvo_batch_set_sensor_distortion).

16 384 resident raw 640x480 sequences (u8 gray + u16 depth in HBM, bench.py's headline shape), run in six modes, alternated round by
round in one process (one batch alive at a time):
  plain         dvo_batch_create with synth.K_640, no distortion (the bench.py path: k_pyramid_raw4<1, false>)
  shared        the same with one D for every sequence (one remap table, k_pyramid_remap_depth<4, false>)
  shared_scalar the same with the scalar kernel forced (DVO_REMAP_DEPTH_SCALAR=1: k_pyramid_remap_depth<1, false>)
  distinct4     four (K, D) pairs through dvo_batch_set_intrinsics + per-sequence D, sequence q on pair q % 4 (four tables; the
                intrinsics table puts the batch on the per-sequence path: k_plan + k_pyramid_remap_depth<4, true>)
  distinct_all  every sequence its own D (one table per sequence, [n_seq][240][320] int32: the worst case; --distinct-batch)
  two_pass      what a user had to do without the fused path: k_ingest's conversion and three torch gathers through an index image
                built once with dvo.undistort (of an image of pixel indices), in chunks, then the plain float push
ms per push comes from device events on the handle's stream around the timed pushes (after a warm-up).  Pose check: the shared mode's
twists of every timed push must equal the two_pass mode's bit for bit.  Prints one JSON line.

    python tools/bench_sensor_undistort.py --batch 16384 --steps 8 --warmup 2 --rounds 2
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

F, W, H = 4, 640, 480
D_TUM = np.array([0.2624, -0.9531, -0.0054, 0.0026, 1.1633], np.float32)   # TUM fr1 RGB camera
CAMS = [synth.K_640,
        np.array([[517.3, 0, 318.6], [0, 516.5, 255.3], [0, 0, 1]], np.float32),
        np.array([[535.4, 0, 320.1], [0, 539.2, 247.6], [0, 0, 1]], np.float32),
        np.array([[400.0, 0, 300.0], [0, 400.0, 260.0], [0, 0, 1]], np.float32)]
DS = [D_TUM,
      np.array([-0.0462, 0.152, -0.00429, 0.0117, -0.0725], np.float32),
      np.array([0.0, 0.0, 0.0, 0.0, 0.0], np.float32),
      np.array([-0.1, 0.05, 0.001, -0.002, 0.0], np.float32)]
CHUNK = 1024   # sequences per two_pass gather (bounds its temporaries)


def frames(B, U, dev):
    """U distinct synthetic sequences of F frames, tiled over B slots: u8 gray, u16 depth (as int16 bits) [F][B][H][W]"""
    g8 = torch.empty((F, U, H, W), dtype=torch.uint8, device=dev)
    d16 = torch.empty((F, U, H, W), dtype=torch.int16, device=dev)
    for u0 in range(0, U, 16):
        u1 = min(U, u0 + 16)
        Ts = np.stack([synth.trajectory(F, seed=42 + u)[f] for u in range(u0, u1) for f in range(F)])
        g, d = synth.render_batch(Ts, synth.K_640, W, H, device=dev, newton_iters=6)
        g8[:, u0:u1] = torch.clamp(torch.round(g * 255.0), 0, 255).to(torch.uint8).reshape(u1 - u0, F, H, W).permute(1, 0, 2, 3)
        d16[:, u0:u1] = (torch.clamp(torch.round(d * 5000.0), 0, 65535).to(torch.int32).to(torch.int16)
                         .reshape(u1 - u0, F, H, W).permute(1, 0, 2, 3))
    idx = torch.arange(B, device=dev) % U
    return g8.index_select(1, idx).contiguous(), d16.index_select(1, idx).contiguous()


def index_image(K, D, dev):
    """the remap of dvo.undistort as an index image: undistort an image whose pixels hold their own index (exact in float32 below
    2^24); INVALID (-2) marks the border"""
    src = np.arange(W * H, dtype=np.float32).reshape(H, W)
    m = dvo.undistort(src, K, D)
    return torch.from_numpy(np.where(m < 0, -1, m).astype(np.int64).reshape(-1)).to(dev)


def run(mode, a, g8, d16, stream):
    B = a.distinct_batch if mode == "distinct_all" else a.batch
    cfg = dvo.default_config(stream=stream)
    bt = dvo.Batch(B, synth.K_640, W, H, 4, 1, cfg=cfg)
    if mode in ("shared", "shared_scalar"):
        bt.set_distortion(D_TUM)
    elif mode == "distinct4":
        bt.set_intrinsics(np.stack([CAMS[q % 4] for q in range(B)]))
        bt.set_distortion(np.stack([DS[q % 4] for q in range(B)]))
    elif mode == "distinct_all":   # every sequence its own coefficients (distinct bits: one table each)
        bt.set_distortion(D_TUM[None] * (1.0 + 1e-6 * np.arange(B, dtype=np.float32))[:, None])
    elif mode == "two_pass":
        idx = index_image(synth.K_640, D_TUM, g8.device)
        valid = idx >= 0
        gidx = idx.clamp(min=0)
        fl = [torch.empty((B, H * W), dtype=torch.float32, device=g8.device) for _ in range(3)]
        inv = torch.tensor(-2.0, dtype=torch.float32, device=g8.device)
        s255 = torch.tensor(1.0 / 255.0, dtype=torch.float32, device=g8.device)
        s5000 = torch.tensor(1.0 / 5000.0, dtype=torch.float32, device=g8.device)
        sv, si = (torch.tensor(v, dtype=torch.float32, device=g8.device) for v in (0.1, 1.0))   # k_ingest's sigma (valid / invalid)
    torch.cuda.synchronize()
    ev = []
    n = 1 + a.warmup + a.steps
    xi_dev = torch.zeros((a.steps, B, 6), dtype=torch.float32, device="cuda")
    for k in range(n):
        timed = k > a.warmup
        if timed:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
        gk, dk = g8[k % F, :B], d16[k % F, :B]
        if mode == "two_pass":
            for c0 in range(0, B, CHUNK):
                c1 = min(B, c0 + CHUNK)
                g = torch.index_select(gk[c0:c1].reshape(c1 - c0, H * W), 1, gidx).to(torch.float32) * s255     # k_ingest's conversion
                d = torch.index_select(dk[c0:c1].reshape(c1 - c0, H * W), 1, gidx).to(torch.int32) & 0xffff
                df = d.to(torch.float32) * s5000
                sg = torch.where(d > 0, sv, si)
                g = torch.where(d == 0, inv, g)
                fl[0][c0:c1] = torch.where(valid, g, inv)
                fl[1][c0:c1] = torch.where(valid, df, inv)
                fl[2][c0:c1] = torch.where(valid, sg, inv)
            bt.push_device(*(x.data_ptr() for x in fl))
        else:
            bt.push_raw_device(gk.data_ptr(), 1, dk.data_ptr())
        if timed:
            e1.record()
            ev.append((e0, e1))
            bt.copy_poses_device(xi_dev[k - a.warmup - 1].data_ptr())   # (after the push's end event)
    torch.cuda.synchronize()
    ms = sum(e0.elapsed_time(e1) for e0, e1 in ev)
    bt.close()
    return {"batch": B, "ms_per_push": ms / a.steps, "frames_per_s": B * a.steps / (ms / 1e3)}, xi_dev.cpu().numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16384)
    ap.add_argument("--distinct-batch", type=int, default=16384, help="batch of the distinct_all mode (one 307 KB table per sequence)")
    ap.add_argument("--unique", type=int, default=64, help="distinct synthetic sequences tiled over the batch")
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--modes", default="plain,shared,shared_scalar,distinct4,distinct_all,two_pass")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    g8, d16 = frames(max(a.batch, a.distinct_batch), a.unique, dev)
    torch.cuda.synchronize()
    modes = a.modes.split(",")
    res = {m: [] for m in modes}
    xi_of = {}
    mismatches, compared = 0, 0
    for r in range(a.rounds):
        for m in modes:
            if m == "shared_scalar":
                os.environ["DVO_REMAP_DEPTH_SCALAR"] = "1"   # (read at every launch)
            out, xi = run(m, a, g8, d16, stream)
            os.environ.pop("DVO_REMAP_DEPTH_SCALAR", None)
            res[m].append(out)
            xi_of[m] = xi
            if m in ("shared", "two_pass") and "shared" in xi_of and "two_pass" in xi_of:
                s, t = xi_of.pop("shared"), xi_of.pop("two_pass")
                mismatches += int((~np.all(s == t, axis=2)).sum()); compared += s.shape[0] * s.shape[1]
    summary = {}
    for m in modes:
        ms = sorted(x["ms_per_push"] for x in res[m])
        summary[m] = {"batch": res[m][0]["batch"], "ms_per_push": round(ms[len(ms) // 2], 3),
                      "ms_per_push_all_rounds": [round(x["ms_per_push"], 3) for x in res[m]],
                      "frames_per_s": round(float(np.median([x["frames_per_s"] for x in res[m]])), 1)}
    if "plain" in summary:
        for m in modes:
            if m != "plain" and summary[m]["batch"] == summary["plain"]["batch"]:
                summary[m]["vs_plain"] = round(summary[m]["ms_per_push"] / summary["plain"]["ms_per_push"], 4)
    print(json.dumps({"batch": a.batch, "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds, "modes": summary,
                      "pose_check_shared_vs_two_pass": {"compared": compared, "mismatches": mismatches}}))
    return 0 if mismatches == 0 and (compared > 0 or not {"shared", "two_pass"} <= set(modes)) else 1


if __name__ == "__main__":
    sys.exit(main())
