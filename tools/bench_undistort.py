#!/usr/bin/env python3
"""bench_undistort.py -- cost of the lens undistortion fused into the mono ingest (dvo_batch_set_distortion).

8 192 resident raw 640x480 mono sequences (u8 gray in HBM, as bench.py's mono leg), run in five modes, alternated round by round in one
process (one batch alive at a time):
  plain         dvo_batch_create_mono with synth.K_640, no distortion (the bench.py path: k_pyramid_raw4<2, false>)
  shared        the same with one D for every sequence (one remap table, k_pyramid_remap)
  distinct4     dvo_batch_create_mono_cameras with four (K, D) pairs, sequence q on pair q % 4 (four tables)
  distinct_all  every sequence on its own D (one table per sequence: the worst case, [n_seq][120][160] int32)
  two_pass      what a user had to do without the fused path: a torch gather over the full frames through an index image built once
                with dvo.undistort (of an image of pixel indices), the u8 -> float conversion of k_ingest, then the plain float path
ms per frame comes from device events on the handle's stream around the timed frames (after a warm-up).  Pose check: the shared mode's
world poses of every timed frame must equal the two_pass mode's bit for bit.  Prints one JSON line.

    python tools/bench_undistort.py --batch 8192 --steps 12 --warmup 3 --rounds 2
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
D_LOGICOOL = np.array([-0.0462, 0.152, -0.00429, 0.0117, -0.0725], np.float32)   # src/core/loader.cpp:18
CAMS = [synth.K_640,
        np.array([[517.3, 0, 318.6], [0, 516.5, 255.3], [0, 0, 1]], np.float32),
        np.array([[535.4, 0, 320.1], [0, 539.2, 247.6], [0, 0, 1]], np.float32),
        np.array([[400.0, 0, 300.0], [0, 400.0, 260.0], [0, 0, 1]], np.float32)]
DS = [D_LOGICOOL,
      np.array([0.2624, -0.9531, -0.0054, 0.0026, 1.1633], np.float32),
      np.array([0.0, 0.0, 0.0, 0.0, 0.0], np.float32),
      np.array([-0.1, 0.05, 0.001, -0.002, 0.0], np.float32)]


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


def index_image(K, D, dev):
    """the remap of dvo.undistort as an index image: undistort an image whose pixels hold their own index (exact in float32 below
    2^24); INVALID (-2) marks the border"""
    src = np.arange(W * H, dtype=np.float32).reshape(H, W)
    m = dvo.undistort(src, K, D)
    return torch.from_numpy(np.where(m < 0, -1, m).astype(np.int64).reshape(-1)).to(dev)


def run(mode, a, g8, stream):
    B = a.batch
    cfg = dvo.default_config(stream=stream, rng_seed=1)
    fl = None
    if mode == "distinct4":
        mb = dvo.MonoBatch(B, np.stack([CAMS[q % 4] for q in range(B)]), W, H, cfg=cfg, per_sequence_K=True)
        mb.set_distortion(np.stack([DS[q % 4] for q in range(B)]))
    else:
        mb = dvo.MonoBatch(B, synth.K_640, W, H, cfg=cfg)
        if mode == "shared":
            mb.set_distortion(D_LOGICOOL)
        elif mode == "distinct_all":   # every sequence its own coefficients (distinct bits: one table each)
            mb.set_distortion(D_LOGICOOL[None] * (1.0 + 1e-6 * np.arange(B, dtype=np.float32))[:, None])
        elif mode == "two_pass":
            idx = index_image(synth.K_640, D_LOGICOOL, g8.device)
            valid = (idx >= 0)
            gidx = idx.clamp(min=0)
            fl = torch.empty((B, H, W), dtype=torch.float32, device=g8.device)
            scale = torch.tensor(1.0 / 255.0, dtype=torch.float32, device=g8.device)
    torch.cuda.synchronize()
    ev = []
    n = 1 + a.warmup + a.steps
    xi_dev = torch.zeros((a.steps, B, 6), dtype=torch.float32, device="cuda")
    for k in range(n):
        timed = k > a.warmup
        if timed:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
        if mode == "two_pass":
            src = g8[k % F].view(B, H * W)
            g = torch.index_select(src, 1, gidx).to(torch.float32) * scale            # k_ingest's (float)u8 * (1/255)
            fl.view(B, H * W).copy_(torch.where(valid, g, torch.tensor(-2.0, device=g.device)))
            mb.odometrize_device(fl.data_ptr())
        else:
            mb.odometrize_raw_device(g8[k % F].data_ptr(), 1)
        if timed:
            e1.record()
            ev.append((e0, e1))
            mb.copy_world_poses_device(xi_dev[k - a.warmup - 1].data_ptr())   # (after the frame's end event)
    torch.cuda.synchronize()
    ms = sum(e0.elapsed_time(e1) for e0, e1 in ev)
    mb.close()
    return {"ms_per_frame": ms / a.steps, "frames_per_s": B * a.steps / (ms / 1e3)}, xi_dev.cpu().numpy()


def single(n):
    """single-stream frames/s of a dvo_vo handle fed raw u8 host frames (odometrizeRaw) and float frames (odometrize), without D and
    with D_LOGICOOL, through the staged upload (DVO_MONO_STAGE=1: the pyramid kernel reads pinned, device-mapped host memory) and the
    runtime's copy (DVO_MONO_STAGE=0).  The handle reads the variable when it is created."""
    import time
    g = synth.sequence(16, seed=42, sigma_value=0.5)[0].numpy()
    g8 = np.clip(np.rint(g * 255), 0, 255).astype(np.uint8)
    idx = [i if i < 16 else 30 - i for i in range(31)]
    out = {}
    for stage in ("1", "0"):
        for D in (None, D_LOGICOOL):
            for feed in ("raw", "float"):
                os.environ["DVO_MONO_STAGE"] = stage
                vo = dvo.VisualOdometry(synth.K_640, W, H)
                if D is not None:
                    vo.setDistortion(D)
                fr = g8 if feed == "raw" else g
                call = vo.odometrizeRaw if feed == "raw" else vo.odometrize
                for k in range(5):
                    call(fr[idx[k]])
                t0 = time.perf_counter()
                for k in range(n):
                    call(fr[idx[(5 + k) % 30]])
                dt = time.perf_counter() - t0
                vo.close()
                out["%s_%s_%s" % ("staged" if stage == "1" else "dma", "D" if D is not None else "plain", feed)] = round(n / dt, 1)
    os.environ.pop("DVO_MONO_STAGE", None)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--unique", type=int, default=64, help="distinct synthetic sequences tiled over the batch")
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--modes", default="plain,shared,distinct4,distinct_all,two_pass")
    ap.add_argument("--single", type=int, default=0, help="N > 0: only the single-stream dvo_vo rates over N frames per case")
    a = ap.parse_args()
    if a.single > 0:
        print(json.dumps({"single_stream_frames_per_s": single(a.single)}))
        return 0
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    g8 = frames(a.batch, a.unique, dev)
    torch.cuda.synchronize()
    modes = a.modes.split(",")
    res = {m: [] for m in modes}
    xi_of = {}
    mismatches, compared = 0, 0
    for r in range(a.rounds):
        for m in modes:
            out, xi = run(m, a, g8, stream)
            res[m].append(out)
            xi_of[m] = xi
            if m in ("shared", "two_pass") and "shared" in xi_of and "two_pass" in xi_of:
                s, t = xi_of.pop("shared"), xi_of.pop("two_pass")
                mismatches += int((~np.all(s == t, axis=2)).sum()); compared += s.shape[0] * s.shape[1]
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
                      "pose_check_shared_vs_two_pass": {"compared": compared, "mismatches": mismatches}}))
    return 0 if mismatches == 0 and (compared > 0 or not {"shared", "two_pass"} <= set(modes)) else 1


if __name__ == "__main__":
    sys.exit(main())
