#!/usr/bin/env python3
"""kf_fusion_outcome.py -- the outcome of keyframe depth fusion on the CPU replica: oracle tracking + kf_fusion_ref.fuse.

Workload (tests/kf_fusion_ref.py, outcome_sequence): geometric_ref.OUTCOME's scene at 320x240, 3 levels, culls 1, four seeds, 8 frames
of smooth motion (0.005 m, 0.25 degrees per frame), depth noise sigma 0.02 m on every frame, frames 1..7 tracked against frame 0.
  (a) R_d: RMS error of the fused keyframe depth against the noise-free depth over pixels with count >= 4 after frame 7, over the
      unfused keyframe's on the same pixels.
  (b) mean 6-norm pose error of frames 5..7 with fusion on and off, plain estimator (orc.track); with --geometric also the geometric
      estimator (geometric_ref.geometric_track, weight 10: a numpy replica, minutes per seed).
--carry: the outcome of the keyframe carry (tests/kf_carry_ref.py): the same scene and motion over 24 frames, keyframes at
frames 0, 6, 12 and 18.  R_c: RMS error of the last keyframe's depth against its noise-free depth after frame 23 with carry on, over
the same with fusion only, on the pixels whose fusion-only count is >= 4; and the mean pose error of frames 19..23 with carry on and
off.  The runs are independent processes (--jobs).
No GPU.    python tools/kf_fusion_outcome.py [--geometric] [--carry] [--jobs N] [--seeds 42 43 44 45]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("direct-visual-odometry_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))

import geometric_ref as gref   # noqa: E402
import kf_carry_ref as cref    # noqa: E402
import kf_fusion_ref as kref   # noqa: E402
import orc                     # noqa: E402


def run(seed, fusion, geometric):
    o, s = gref.OUTCOME, kref.OUTCOME
    g, d, sg, clean, K, truths = kref.outcome_sequence(seed)
    L, Cu = o["levels"], o["culls"]
    key = orc.OFrame(g[0], d[0], sg[0], K, L, Cu)
    levels = [key.depth(l) for l in range(L)]
    unfused_top = levels[-1].copy()
    counts = np.zeros(levels[-1].shape, np.uint8)
    k_top = key.K(L - 1)
    errs = {}
    for k in range(1, s["frames"]):
        obj = orc.OFrame(g[k], d[k], sg[k], K, L, Cu, id=k)
        if geometric:
            xi, _ = gref.geometric_track(obj, key, L, s["geometric_weight"], s["geometric_max_diff"], False, o["max_iterations"],
                                         o["min_update"], o["min_residual"])
        else:
            xi, _ = orc.track(obj, key, crop=False)
        errs[k] = gref.pose_error(xi, truths[k])
        if fusion:
            levels, counts, rec = kref.fuse(levels, counts, obj.depth(L - 1), k_top, orc.se3_exp(xi), orc.se3_exp(-xi), 0.2, s["max_diff"],
                                            s["max_count"])
            key.update_depth_sigma(levels[-1], key.sigma(L - 1))
            for l in range(L):   # the oracle's own re-decimation must be the contract's point decimation
                assert key.depth(l).tobytes() == levels[l].tobytes(), l
    clean_top = kref.cull(clean[0], Cu).astype(np.float64)
    ratio, n = kref.map_ratio(levels[-1], unfused_top, clean_top, counts, s["min_count"]) if fusion else (1.0, 0)
    return float(np.mean([errs[k] for k in s["score_frames"]])), ratio, n


def run_carry(job):
    """(seed, carry, geometric) -> (mean pose error of the score frames, the last keyframe's top-level depth, its counts)"""
    seed, carry, geometric = job
    o, s, c = gref.OUTCOME, kref.OUTCOME, cref.OUTCOME
    orc.set_tracker_params(step3=o["steps"], min_residual=o["min_residual"], min_update=o["min_update"])
    g, d, sg, clean, K, poses = cref.outcome_sequence(seed)
    L, Cu = o["levels"], o["culls"]
    key = orc.OFrame(g[0], d[0], sg[0], K, L, Cu)
    levels = [key.depth(l) for l in range(L)]
    counts = np.zeros(levels[-1].shape, np.uint8)
    k_top = key.K(L - 1)
    kf, errs = 0, {}
    for k in range(1, c["frames"]):
        obj = orc.OFrame(g[k], d[k], sg[k], K, L, Cu, id=k)
        if geometric:
            xi, _ = gref.geometric_track(obj, key, L, s["geometric_weight"], s["geometric_max_diff"], False, o["max_iterations"],
                                         o["min_update"], o["min_residual"])
        else:
            xi, _ = orc.track(obj, key, crop=False)
        errs[k] = gref.pose_error(xi, cref.truth(poses, k, kf))
        promote = k - kf >= c["keyframe_max_frames"]
        cm, fm = cref.modes(True, promote, False, xi)
        levels, counts, _, _, _ = cref.step(cm, fm, levels, counts, [obj.depth(l) for l in range(L)], k_top, orc.se3_exp(xi),
                                            orc.se3_exp(-xi), 0.2, c["max_diff"], s["max_diff"], s["max_count"], carry_on=carry)
        if promote:
            key, kf = obj, k
        key.update_depth_sigma(levels[-1], key.sigma(L - 1))
        for l in range(L):   # the oracle's own re-decimation must be the contract's point decimation
            assert key.depth(l).tobytes() == levels[l].tobytes(), l
    assert kf == c["last_keyframe"]
    clean_top = kref.cull(clean[kf], Cu).astype(np.float64)
    return float(np.mean([errs[k] for k in c["score_frames"]])), levels[-1], counts, clean_top


def main_carry(a):
    import multiprocessing as mp
    s = kref.OUTCOME
    ests = [False, True] if a.geometric else [False]
    jobs = [(seed, carry, geo) for geo in ests for seed in a.seeds for carry in (False, True)]
    with mp.Pool(min(a.jobs, len(jobs))) as pool:
        res = dict(zip(jobs, pool.map(run_carry, jobs, chunksize=1)))
    print("seed  estimator  err_off      err_on       on/off   R_c     pixels(fusion-only count>=4)")
    for geo in ests:
        est, ratios = ("geometric" if geo else "plain"), []
        for seed in a.seeds:
            e_off, top_off, c_off, clean_top = res[(seed, False, geo)]
            e_on, top_on, _, _ = res[(seed, True, geo)]
            r, n = cref.carry_ratio(top_on, top_off, clean_top, c_off, s["min_count"])
            ratios.append(r)
            print("%4d  %-9s  %.4e  %.4e  %.3f   %.4f  %d" % (seed, est, e_off, e_on, e_on / e_off, r, n), flush=True)
        print("      %-9s  mean R_c %.4f" % (est, float(np.mean(ratios))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--geometric", action="store_true")
    ap.add_argument("--carry", action="store_true", help="the 24-frame carry workload of DESIGN.md section 36")
    ap.add_argument("--jobs", type=int, default=4)
    ap.add_argument("--seeds", type=int, nargs="*", default=list(gref.OUTCOME["seeds"]))
    a = ap.parse_args()
    if a.carry:
        return main_carry(a)
    o = gref.OUTCOME
    orc.set_tracker_params(step3=o["steps"], min_residual=o["min_residual"], min_update=o["min_update"])
    print("seed  estimator  err_off      err_on       on/off   R_d     pixels(count>=4)")
    for est in (["plain", "geometric"] if a.geometric else ["plain"]):
        ratios = []
        for seed in a.seeds:
            e_off, _, _ = run(seed, False, est == "geometric")
            e_on, r, n = run(seed, True, est == "geometric")
            ratios.append(r)
            print("%4d  %-9s  %.4e  %.4e  %.3f   %.4f  %d" % (seed, est, e_off, e_on, e_on / e_off, r, n), flush=True)
        print("      %-9s  mean R_d %.4f" % (est, float(np.mean(ratios))), flush=True)


if __name__ == "__main__":
    main()
