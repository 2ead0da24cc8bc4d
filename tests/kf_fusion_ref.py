"""Contract-exact replica of keyframe depth fusion (dvo_batch_set_keyframe_fusion, include/dvo.h).

numpy float32, one correctly rounded operation per contract operation: fmaf is robust_ref's, back_project / transform / project are
restated as geometric_ref restates them (tests/test_geometric_abi.py holds that restatement to the oracle bit for bit).  The poses
F = float(exp(xi)) and Bk = float(exp(-xi)) are inputs: 4x4 (or flat 16) float32 matrices, as dvo_batch_last_poses and
dvo_op_se3_exp(-xi) return them.  Nothing here is tuned on a device result.  Test infrastructure only."""
import numpy as np

import robust_ref as rr

F32 = np.float32
NONE, CLEAR, FUSE = 0, 1, 2


def intr(K):
    """(fx, fy, cx, cy, 1 / fx, 1 / fy) of a level's 3x3 K, the reciprocals rounded once (dvo_math.h make_intr)"""
    K = np.asarray(K, F32).reshape(3, 3)
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    return fx, fy, cx, cy, F32(1) / fx, F32(1) / fy


def back_project(k, px, py, d):
    fx, fy, cx, cy, ifx, ify = k
    with np.errstate(all="ignore"):
        X = ((d * (px - cx)).astype(F32) * ifx).astype(F32)
        Y = ((d * (py - cy)).astype(F32) * ify).astype(F32)
    return X, Y, d


def transform(T, X, Y, Z):
    T = np.asarray(T, F32).reshape(4, 4)
    full = lambda v: np.full_like(X, v)
    with np.errstate(all="ignore"):
        row = lambda i: rr.fmaf(full(T[i, 0]), X, rr.fmaf(full(T[i, 1]), Y, rr.fmaf(full(T[i, 2]), Z, full(T[i, 3]))))
        return row(0), row(1), row(2)


def project(k, X, Y, Z):
    fx, fy, cx, cy, _, _ = k
    with np.errstate(all="ignore"):
        iz = (F32(1) / Z).astype(F32)
        u = ((X * fx).astype(F32) * iz).astype(F32) + cx
        v = ((Y * fy).astype(F32) * iz).astype(F32) + cy
    return u.astype(F32), v.astype(F32)


def cull(img, times):
    """point decimation (orc_cull_image, frame.cpp:39-61): pixel (x, y) of the result is (x << times, y << times), size truncated"""
    h, w = img.shape
    return np.ascontiguousarray(img[::1 << times, ::1 << times][:h >> times, :w >> times])


def write_levels(levels, top_new, changed):
    """the coarser levels after step 9: pixels the decimation picks take the new top-level value where it changed"""
    T = len(levels) - 1
    out = [None] * len(levels)
    out[T] = top_new
    for l in range(T):
        t = T - l
        lv = levels[l].copy()
        h, w = lv.shape
        sel = cull(changed, t)[:h, :w]
        lv[:sel.shape[0], :sel.shape[1]][sel] = cull(top_new, t)[:h, :w][sel]
        out[l] = lv
    return out


def clear(kf_levels, counts):
    """a start or a promotion: the depth was just replaced, the counts become 0, the record zeros"""
    return [np.array(l, F32) for l in kf_levels], np.zeros_like(counts), dict(n_candidates=0, n_fused=0, n_gated=0)


def fuse(kf_levels, counts, frame_top, k_top, F, Bk, min_depth, max_diff, max_count):
    """One fusing push of one sequence.  kf_levels: the keyframe's depth maps, index = level (the last is the top); counts uint8 [h][w];
    frame_top: the tracked frame's top-level depth; k_top: the top level's 3x3 K.  Returns (new levels, new counts, record)."""
    levels = [np.array(l, F32) for l in kf_levels]
    d = levels[-1]
    frame = np.ascontiguousarray(frame_top, F32)
    h, w = d.shape
    k = intr(k_top)
    md = F32(min_depth); mxd = F32(max_diff)
    ys, xs = np.mgrid[0:h, 0:w]
    with np.errstate(all="ignore"):
        cand = d >= md                                                            # 1 (false for NaN)
        X, Y, Z = back_project(k, xs.astype(F32), ys.astype(F32), d)              # 2
        Xf, Yf, Zf = transform(F, X, Y, Z)
        ok = cand & (Zf >= md)
        u, v = project(k, Xf, Yf, Zf)
        ok &= (u >= 0) & (u < F32(w - 1)) & (v >= 0) & (v < F32(h - 1))           # 3 (false for NaN / inf)
        x0 = np.where(ok, u, 0).astype(np.int64); y0 = np.where(ok, v, 0).astype(np.int64)
        a = (u - x0.astype(F32)).astype(F32); b = (v - y0.astype(F32)).astype(F32)
        x1 = np.minimum(x0 + 1, w - 1); y1 = np.minimum(y0 + 1, h - 1)
        z00, z10, z01, z11 = frame[y0, x0], frame[y0, x1], frame[y1, x0], frame[y1, x1]   # 4
        for z in (z00, z10, z01, z11):
            ok &= (z >= md) & (z < F32(np.inf))
        mx = np.maximum(np.maximum(z00, z10), np.maximum(z01, z11)); mn = np.minimum(np.minimum(z00, z10), np.minimum(z01, z11))
        ok &= (mx - mn).astype(F32) <= mxd
        top = rr.fmaf(a, (z10 - z00).astype(F32), z00)                            # 5
        bot = rr.fmaf(a, (z11 - z01).astype(F32), z01)
        zi = rr.fmaf(b, (bot - top).astype(F32), top)
        near = np.abs((zi - Zf).astype(F32)) <= mxd                               # 6
        gated = ok & ~near
        ok &= near
        Xo, Yo, Zo = back_project(k, u, v, zi)                                    # 7
        _, _, d_obs = transform(Bk, Xo, Yo, Zo)
        ok &= (d_obs >= md) & (d_obs < F32(np.inf))
        c = counts.astype(np.int64)                                               # 8
        r = (F32(1) / (c + 2).astype(F32)).astype(F32)
        d_new = rr.fmaf((d_obs - d).astype(F32), r, d)
    top_new = d.copy()
    top_new[ok] = d_new[ok]                                                       # 9
    counts_new = counts.copy()
    counts_new[ok] = np.minimum(c[ok] + 1, max_count).astype(np.uint8)
    rec = dict(n_candidates=int(cand.sum()), n_fused=int(ok.sum()), n_gated=int(gated.sum()))
    return write_levels(levels, top_new, ok), counts_new, rec


def step(mode, kf_levels, counts, frame_top, k_top, F, Bk, min_depth, max_diff, max_count):
    """one push of one sequence by its resolved mode (NONE: skipped, or a non-finite twist)"""
    if mode == CLEAR:
        return clear(kf_levels, counts)
    if mode == FUSE:
        return fuse(kf_levels, counts, frame_top, k_top, F, Bk, min_depth, max_diff, max_count)
    return [np.array(l, F32) for l in kf_levels], counts.copy(), dict(n_candidates=0, n_fused=0, n_gated=0)


# ---- the outcome workload of DESIGN.md §28: one keyframe, seven tracked frames, sensor noise on every depth map -----------------
OUTCOME = dict(frames=8, step_t=0.005, step_r_deg=0.25, depth_sigma=0.02, keyframe_min_translation=1.0, keyframe_max_frames=8,
               max_diff=0.05, max_count=16, min_count=4, score_frames=(5, 6, 7), geometric_weight=10.0, geometric_max_diff=0.1)


def outcome_sequence(seed):
    """geometric_ref.OUTCOME's scene and sizes under smooth motion: frame k sits at T_k = T_{k-1} exp(xi), xi a constant twist of
    0.005 m and 0.25 degrees whose directions come from the seed; gray with the scene's reduced contrast and noise; depth with
    Gaussian noise of 0.02 m on every frame.  Returns (gray [n][h][w], noisy depth, sigma, clean depth, K, truths [n][6]) with
    truths[k] = log(inv(T_k) T_0), the twist a tracker of frame k against frame 0 should return."""
    import geometric_ref as gref
    import orc
    from dvo_amd import synth
    o, s = gref.OUTCOME, OUTCOME
    K = synth.K_640.copy(); K[:2] *= 0.5
    rng = np.random.RandomState(2000 + seed)
    dt = rng.normal(size=3); dt *= s["step_t"] / np.linalg.norm(dt)
    dr = rng.normal(size=3); dr *= np.radians(s["step_r_deg"]) / np.linalg.norm(dr)
    step = synth.se3_exp_np(np.concatenate([dt, dr]))
    poses = [np.eye(4)]
    for _ in range(1, s["frames"]):
        poses.append(poses[-1] @ step)
    g, d = synth.render_batch(poses, K, o["width"], o["height"])
    g = g.numpy().astype(np.float64); clean = d.numpy().astype(np.float64)
    g = 0.5 + o["contrast"] * (g - 0.5) + rng.normal(0.0, o["gray_sigma"], g.shape)
    noisy = clean + rng.normal(0.0, s["depth_sigma"], clean.shape)
    truths = np.array([orc.se3_log(np.linalg.inv(P) @ poses[0]) for P in poses], F32)
    sigma = np.full(g.shape, 0.5, F32)
    return g.astype(F32), noisy.astype(F32), sigma, clean.astype(F32), K, truths


def map_ratio(fused_top, unfused_top, clean_top, counts, min_count):
    """(a): RMS error of the fused keyframe depth against the noise-free depth over pixels with count >= min_count, divided by the
    unfused keyframe's over the same pixels; and the number of those pixels"""
    m = counts >= min_count
    e1 = (fused_top.astype(np.float64) - clean_top)[m]; e0 = (unfused_top.astype(np.float64) - clean_top)[m]
    return float(np.sqrt(np.mean(e1 ** 2)) / np.sqrt(np.mean(e0 ** 2))), int(m.sum())
