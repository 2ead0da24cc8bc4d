#!/usr/bin/env python3
"""bench_photometric.py -- cost of the photometric calibration fused into the mono ingest (dvo_batch_set_photometric).

8 192 resident raw 640x480 mono sequences (u8 gray in HBM, as bench.py's mono leg), run in six modes, alternated round by round in one
process (one batch alive at a time):
  plain       dvo_batch_create_mono with synth.K_640, no calibration (the bench.py path: k_pyramid_raw4<2, false>)
  shared      one calibration (gamma-2.2 inverse response, cos^4 vignette) for every sequence: one gain table (k_pyramid_raw4_photo)
  four        four calibrations, sequence q on calibration q % 4 (four gain tables)
  per_seq     one calibration per sequence with a NULL vignette: the tables are deduplicated on the integer pair, not on their
              contents, so this is one gain table per sequence ([n_seq][120][160] float, none of it shared: the worst case)
  shared_D    the shared calibration and one D for every sequence (k_pyramid_photo<false, true>)
  two_pass    what a user had to do without the fused path: torch looks the response up, multiplies by 1 / vignette over the full
              frames, and the float frames go to a plain handle
ms per frame comes from device events on the handle's stream around the timed frames (after a warm-up).  Pose check: the shared mode's
world poses of every timed frame must equal the two_pass mode's bit for bit.  Prints one JSON line.

    python tools/bench_photometric.py --batch 8192 --steps 12 --warmup 3 --rounds 2

--kernels N: instead, N frames each of plain, shared with the response row staged in LDS, and shared with the response read by plain
loads (DVO_PHOTO_RESPONSE=global), for a `rocprofv3 --kernel-trace --stats` run of its own: the per-launch times of
k_pyramid_raw4<2, false> and of the two k_pyramid_raw4_photo<2, false, .> instances.
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


def response(gamma):
    return ((np.arange(256, dtype=np.float64) / 255.0) ** gamma).astype(np.float32)


def vignette(corner, cx=(W - 1) / 2.0, cy=(H - 1) / 2.0):
    """cos^4 fall-off reaching `corner` at the farthest image corner"""
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    r2 = (x - cx) ** 2 + (y - cy) ** 2
    return ((1.0 + r2 * (corner ** -0.5 - 1.0) / r2.max()) ** -2).astype(np.float32)


def run(mode, a, g8, stream):
    B = a.batch
    cfg = dvo.default_config(stream=stream, rng_seed=1)
    mb = dvo.MonoBatch(B, synth.K_640, W, H, cfg=cfg)
    lut, V = response(2.2), vignette(0.4)
    fl = None
    if mode in ("shared", "shared_D"):
        mb.set_photometric(lut, V)
        if mode == "shared_D":
            mb.set_distortion(D_LOGICOOL)
    elif mode == "four":
        mb.set_photometric(np.stack([response(g) for g in (2.2, 2.0, 1.8, 2.4)]),
                           np.stack([V, vignette(0.5), vignette(0.45, 300.0, 250.0), vignette(0.6, 330.0, 230.0)]), np.arange(B) % 4)
    elif mode == "per_seq":
        mb.set_photometric(np.stack([response(2.2 + 1e-4 * (q % 64)) for q in range(B)]), None, np.arange(B))
    elif mode == "two_pass":
        lut_d = torch.from_numpy(lut).to(g8.device)
        gain_d = (torch.tensor(1.0, dtype=torch.float32) / torch.from_numpy(V)).to(g8.device)   # float32: the one division
        fl = torch.empty((B, H, W), dtype=torch.float32, device=g8.device)
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
            torch.mul(lut_d[g8[k % F].to(torch.int32)], gain_d, out=fl)   # table lookup, multiply
            mb.odometrize_device(fl.data_ptr())
        else:
            mb.odometrize_raw_device(g8[k % F].data_ptr(), 1)
        if timed:
            e1.record()
            ev.append((e0, e1))
            mb.copy_world_poses_device(xi_dev[k - a.warmup - 1].data_ptr())   # (after the frame's end event)
    torch.cuda.synchronize()
    ms = sum(e0.elapsed_time(e1) for e0, e1 in ev)
    ran = mb.last_pyramid_kernel().name()
    mb.close()
    return {"ms_per_frame": ms / a.steps, "frames_per_s": B * a.steps / (ms / 1e3), "kernel": ran}, xi_dev.cpu().numpy()


def kernels(a, g8, stream):
    """a few frames of each form, to be traced from outside"""
    out = {}
    for name, env in (("plain", None), ("photo_lds", "lds"), ("photo_global", "global")):
        if env:
            os.environ["DVO_PHOTO_RESPONSE"] = env
        mb = dvo.MonoBatch(a.batch, synth.K_640, W, H, cfg=dvo.default_config(stream=stream, rng_seed=1))
        if env:
            mb.set_photometric(response(2.2), vignette(0.4))
        for k in range(a.kernels):
            mb.odometrize_raw_device(g8[k % F].data_ptr(), 1)
        mb.synchronize()
        out[name] = mb.last_pyramid_kernel().name()
        mb.close()
    os.environ.pop("DVO_PHOTO_RESPONSE", None)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--unique", type=int, default=64, help="distinct synthetic sequences tiled over the batch")
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--modes", default="plain,shared,four,per_seq,shared_D,two_pass")
    ap.add_argument("--kernels", type=int, default=0, help="N > 0: only N frames each of plain / LDS response / plain-load response, for a kernel trace")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    g8 = frames(a.batch, a.unique, dev)
    torch.cuda.synchronize()
    if a.kernels > 0:
        print(json.dumps({"batch": a.batch, "frames_each": a.kernels, "kernels": kernels(a, g8, stream)}))
        return 0
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
                      "frames_per_s": round(float(np.median([x["frames_per_s"] for x in res[m]])), 1), "kernel": res[m][0]["kernel"]}
    if "plain" in summary:
        for m in modes:
            if m != "plain":
                summary[m]["vs_plain"] = round(summary[m]["ms_per_frame"] / summary["plain"]["ms_per_frame"], 4)
    print(json.dumps({"batch": a.batch, "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds, "modes": summary,
                      "pose_check_shared_vs_two_pass": {"compared": compared, "mismatches": mismatches}}))
    return 0 if mismatches == 0 and (compared > 0 or not {"shared", "two_pass"} <= set(modes)) else 1


if __name__ == "__main__":
    sys.exit(main())
