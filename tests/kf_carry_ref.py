"""Contract-exact replica of the keyframe carry (dvo_batch_set_keyframe_carry, include/dvo.h).

numpy float32, one correctly rounded operation per contract operation, on kf_fusion_ref's restatements (intr, back_project, transform,
project, write_levels) and robust_ref.fmaf.  The poses F = float(exp(xi)) and Bk = float(exp(-xi)) are inputs, as for kf_fusion_ref.
`step` composes carry -> promote -> clear / commit -> fuse for one sequence and one push.  Nothing here is tuned on a device result.
Test infrastructure only."""
import numpy as np

import kf_fusion_ref as kref
import robust_ref as rr

F32 = np.float32
NONE, CARRY = 0, 1
ZERO = dict(n_candidates=0, n_carried=0, n_gated=0)


def carry(frame_levels, kf_top, counts, k_top, F, Bk, min_depth, max_diff, max_count):
    """One carrying push of one sequence.  frame_levels: the tracked frame's depth maps, index = level (the last is the top);
    kf_top / counts: the OLD keyframe's top-level depth and its uint8 count plane; k_top: the top level's 3x3 K.
    Returns (the frame's new levels = the new keyframe's depth, the new counts, record)."""
    levels = [np.array(l, F32) for l in frame_levels]
    d = levels[-1]
    old = np.ascontiguousarray(kf_top, F32)
    h, w = d.shape
    k = kref.intr(k_top)
    md = F32(min_depth); mxd = F32(max_diff); inf = F32(np.inf)
    ys, xs = np.mgrid[0:h, 0:w]
    with np.errstate(all="ignore"):
        cand = (d >= md) & (d < inf)                                              # 1 (false for NaN)
        X, Y, Z = kref.back_project(k, xs.astype(F32), ys.astype(F32), d)         # 2
        Xk, Yk, Zk = kref.transform(Bk, X, Y, Z)                                  # 3
        ok = cand & (Zk >= md)
        u, v = kref.project(k, Xk, Yk, Zk)                                        # 4
        ok &= (u >= 0) & (u < F32(w - 1)) & (v >= 0) & (v < F32(h - 1))
        x0 = np.where(ok, u, 0).astype(np.int64); y0 = np.where(ok, v, 0).astype(np.int64)
        a = (u - x0.astype(F32)).astype(F32); b = (v - y0.astype(F32)).astype(F32)
        x1 = np.minimum(x0 + 1, w - 1); y1 = np.minimum(y0 + 1, h - 1)
        z00, z10, z01, z11 = old[y0, x0], old[y0, x1], old[y1, x0], old[y1, x1]   # 5
        for z in (z00, z10, z01, z11):
            ok &= (z >= md) & (z < inf)
        mx = np.maximum(np.maximum(z00, z10), np.maximum(z01, z11)); mn = np.minimum(np.minimum(z00, z10), np.minimum(z01, z11))
        ok &= (mx - mn).astype(F32) <= mxd
        top = rr.fmaf(a, (z10 - z00).astype(F32), z00)                            # 6
        bot = rr.fmaf(a, (z11 - z01).astype(F32), z01)
        zi = rr.fmaf(b, (bot - top).astype(F32), top)
        near = np.abs((zi - Zk).astype(F32)) <= mxd                               # 7
        gated = ok & ~near
        ok &= near
        Xo, Yo, Zo = kref.back_project(k, u, v, zi)                               # 8
        _, _, d_prior = kref.transform(F, Xo, Yo, Zo)
        ok &= (d_prior >= md) & (d_prior < inf)
        c = counts.astype(np.int64)                                               # 9
        c_prior = np.minimum(np.minimum(c[y0, x0], c[y0, x1]), np.minimum(c[y1, x0], c[y1, x1]))
        r = ((c_prior + 1).astype(F32) * (F32(1) / (c_prior + 2).astype(F32)).astype(F32)).astype(F32)   # 10
        d_new = rr.fmaf((d_prior - d).astype(F32), r, d)                          # 11
        ok &= (d_new >= md) & (d_new < inf)
    top_new = d.copy()
    top_new[ok] = d_new[ok]
    counts_new = np.zeros_like(counts)
    counts_new[ok] = np.minimum(c_prior[ok] + 1, max_count).astype(np.uint8)      # 12
    rec = dict(n_candidates=int(cand.sum()), n_carried=int(ok.sum()), n_gated=int(gated.sum()))
    return kref.write_levels(levels, top_new, ok), counts_new, rec               # 13


def modes(eff_track, is_key, started, xi):
    """(carry mode, fusion mode) of a sequence's push: eff_track = the push TRACKED it, is_key = its keyframe flag, started = the push
    STARTED it (a RESTART, or its first frame); everything else is a skip"""
    finite = bool(np.all(np.isfinite(xi)))
    if started:
        return NONE, kref.CLEAR
    if eff_track and is_key:
        return (CARRY if finite else NONE), kref.CLEAR
    if eff_track:
        return NONE, (kref.FUSE if finite else kref.NONE)
    return NONE, kref.NONE


def step(carry_mode, fuse_mode, kf_levels, counts, frame_levels, k_top, F, Bk, min_depth, carry_max_diff, fuse_max_diff, max_count,
         carry_on=True):
    """One push of one sequence: carry -> promote -> clear / commit -> fuse.  kf_levels / counts: the keyframe before the push (None
    while the sequence has never started); frame_levels: the tracked frame's depth pyramid as the push built it.
    Returns (keyframe levels, counts, frame levels as dvo_batch_frame_get returns them, carry record, fusion record)."""
    frame = [np.array(l, F32) for l in frame_levels]
    zf = dict(n_candidates=0, n_fused=0, n_gated=0)
    if fuse_mode == kref.CLEAR:
        h, w = frame[-1].shape
        if carry_on and carry_mode == CARRY:
            frame, staged, rec = carry(frame, kf_levels[-1], counts, k_top, F, Bk, min_depth, carry_max_diff, max_count)
            return [l.copy() for l in frame], staged, frame, rec, zf
        return [l.copy() for l in frame], np.zeros((h, w), np.uint8), frame, dict(ZERO), zf
    if fuse_mode == kref.FUSE:
        lv, c, rf = kref.fuse(kf_levels, counts, frame[-1], k_top, F, Bk, min_depth, fuse_max_diff, max_count)
        return lv, c, frame, dict(ZERO), rf
    lv = None if kf_levels is None else [np.array(l, F32) for l in kf_levels]
    return lv, None if counts is None else counts.copy(), frame, dict(ZERO), zf


# ---- the outcome workload of DESIGN.md §36: kf_fusion_ref.OUTCOME's scene, sizes, noise and motion per frame, 24 frames, keyframes at
# frames 0, 6, 12 and 18 (keyframe_max_frames = 6; keyframe_min_translation = 1.0 never fires) ---------------------------------------
OUTCOME = dict(frames=24, keyframe_max_frames=6, keyframe_min_translation=1.0, seeds=(42, 43, 44, 45), score_frames=(19, 20, 21, 22, 23),
               last_keyframe=18, max_diff=0.05)


def outcome_sequence(seed):
    """kf_fusion_ref.outcome_sequence with OUTCOME['frames'] frames.  Returns (gray [n][h][w], noisy depth, sigma, clean depth, K,
    poses [n][4][4] float64 world <- camera): the twist a tracker of frame k against keyframe j should return is log(inv(T_k) T_j)."""
    import geometric_ref as gref
    from dvo_amd import synth
    o, s = gref.OUTCOME, kref.OUTCOME
    K = synth.K_640.copy(); K[:2] *= 0.5
    rng = np.random.RandomState(2000 + seed)
    dt = rng.normal(size=3); dt *= s["step_t"] / np.linalg.norm(dt)
    dr = rng.normal(size=3); dr *= np.radians(s["step_r_deg"]) / np.linalg.norm(dr)
    step_T = synth.se3_exp_np(np.concatenate([dt, dr]))
    poses = [np.eye(4)]
    for _ in range(1, OUTCOME["frames"]):
        poses.append(poses[-1] @ step_T)
    g, d = synth.render_batch(poses, K, o["width"], o["height"])
    g = g.numpy().astype(np.float64); clean = d.numpy().astype(np.float64)
    g = 0.5 + o["contrast"] * (g - 0.5) + rng.normal(0.0, o["gray_sigma"], g.shape)
    noisy = clean + rng.normal(0.0, s["depth_sigma"], clean.shape)
    sigma = np.full(g.shape, 0.5, F32)
    return g.astype(F32), noisy.astype(F32), sigma, clean.astype(F32), K, np.array(poses)


def truth(poses, k, j):
    import orc
    return np.asarray(orc.se3_log(np.linalg.inv(poses[k]) @ poses[j]), F32)


def carry_ratio(carry_top, fusion_top, clean_top, fusion_counts, min_count):
    """RMS error of the carried keyframe depth against the noise-free depth over the pixels whose FUSION-ONLY count is >= min_count,
    divided by the fusion-only keyframe's over the same pixels; and the number of those pixels"""
    m = fusion_counts >= min_count
    e1 = (carry_top.astype(np.float64) - clean_top)[m]; e0 = (fusion_top.astype(np.float64) - clean_top)[m]
    return float(np.sqrt(np.mean(e1 ** 2)) / np.sqrt(np.mean(e0 ** 2))), int(m.sum())
