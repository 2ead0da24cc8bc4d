"""Contract-exact replica of the keyframe point-cloud export (dvo_batch_export_points, include/dvo.h).

numpy float32, one correctly rounded operation per contract operation: back_project / transform are kf_fusion_ref's (the fmaf is
robust_ref's).  The inputs are what the public readers return: the maps and twist of dvo_batch_keyframe_get, the count plane of
dvo_batch_keyframe_fusion_counts and Wk = dvo_op_se3_exp(-xi).  Nothing here is tuned on a device result.  Test infrastructure only."""
import numpy as np

import kf_fusion_ref as kref

F32 = np.float32
ALL, NEW = 0, 1
CHUNK = 1024    # pixels of one workgroup of the device's passes (the tests place points around its edges; the replica does not use it)


def level_K(K, culls, levels, level):
    """the 3x3 K of pyramid level `level`, by the engine's steps: cull to the pyramid base, then to the level"""
    import orc
    return orc.cull_intrinsic(orc.cull_intrinsic(np.asarray(K, F32).reshape(3, 3), culls), levels - 1 - level)


def gates(depth, stride=1, min_depth=0.2, max_depth=np.inf, sigma=None, max_sigma=np.inf, age=None, min_age=0.0, counts=None, min_count=0):
    """bool [h][w]: the candidates.  A gate at its neutral value (+inf, 0, 0) is no gate: its map is not read."""
    d = np.asarray(depth, F32)
    h, w = d.shape
    ys, xs = np.mgrid[0:h, 0:w]
    with np.errstate(invalid="ignore"):
        m = (d >= F32(min_depth)) & (d <= F32(max_depth)) & np.isfinite(d)       # false for NaN / inf
        m &= (xs % stride == 0) & (ys % stride == 0)
        if F32(max_sigma) < F32(np.inf):
            m &= np.asarray(sigma, F32) <= F32(max_sigma)
        if F32(min_age) > 0:
            m &= np.asarray(age, F32) >= F32(min_age)
        if min_count > 0:
            m &= np.asarray(counts).astype(np.int64) >= min_count
    return m


def export_sequence(depth, gray, K_level, Wk, sigma=None, **gate_kw):
    """one selected sequence: (xyzg float32 [n][4], src uint32 [n], sigma float32 [n] or None), raster order"""
    d = np.asarray(depth, F32)
    h, w = d.shape
    m = gates(d, sigma=sigma, **gate_kw)
    ys, xs = np.nonzero(m)                                                       # raster order: rows, then columns
    X, Y, Z = kref.back_project(kref.intr(K_level), xs.astype(F32), ys.astype(F32), d[ys, xs])
    Xw, Yw, Zw = kref.transform(Wk, X, Y, Z)
    xyzg = np.stack([Xw, Yw, Zw, np.asarray(gray, F32)[ys, xs]], axis=1).astype(F32).reshape(-1, 4)
    src = (ys * w + xs).astype(np.uint32)
    sg = np.asarray(sigma, F32)[ys, xs] if sigma is not None else None
    return xyzg, src, sg


def export(seqs, want_sigma=False, **gate_kw):
    """seqs: per sequence None (never started, or deselected) or dict(depth, gray, K, Wk[, sigma, age, counts]).
    Returns (offsets uint32 [n + 1], xyzg [total][4], src [total], sigma [total] or None)."""
    parts, off = [], [0]
    for s in seqs:
        if s is None:
            off.append(off[-1])
            continue
        kw = dict(gate_kw)
        kw.update(age=s.get("age"), counts=s.get("counts"))
        p = export_sequence(s["depth"], s["gray"], s["K"], s["Wk"], sigma=s.get("sigma"), **kw)
        parts.append(p)
        off.append(off[-1] + len(p[1]))
    if parts:
        xyzg = np.concatenate([p[0] for p in parts]); src = np.concatenate([p[1] for p in parts])
        sg = np.concatenate([p[2] for p in parts]) if want_sigma else None
    else:
        xyzg = np.zeros((0, 4), F32); src = np.zeros(0, np.uint32); sg = np.zeros(0, F32) if want_sigma else None
    return np.asarray(off, np.uint32), xyzg, src, sg


# ---- the convention workload of DESIGN.md §35: one sensor-depth sequence on synth.sequence(6, 320x240, seed 42), keyframes every three
# frames, so the keyframe after five pushes is frame 3.  `ratio`: median surface distance of the replica's points over that of the
# wrong direction, with the ground-truth pose in place of the tracked one (tools-free: python -c "import points_ref; print(points_ref.convention_cpu())")
CONVENTION = dict(max_frames=3, pushes=5, keyframe=3, ratio=2.4e-6)   # (5.1e-8 m against 0.0215 m)


def surface_distance(P):
    """|Z - height(X, Y)| of world points [n][3] against synth's surface (synth.height), float64"""
    P = np.asarray(P, np.float64)
    Z = 1.5 + 0.3 * np.sin(2 * np.pi * P[:, 0] / 2.0) * np.cos(2 * np.pi * P[:, 1] / 1.5)
    return np.abs(P[:, 2] - Z)


def convention_figures(depth, K_level, T_kf, src, exported):
    """T_kf: float64 4x4, world -> keyframe camera (T_world of the push that made the keyframe).  Median surface distances of the
    exported points, of inv(T_kf) X_k in float64, of the same chain in float32 and of the wrong direction T_kf X_k; and the worst ratio
    of |exported - float64 reference| to 16 * 2^-24 * (|X_k| + |Y_k| + |Z_k| + |t|_1)."""
    d = np.asarray(depth, F32)
    h, w = d.shape
    src = np.asarray(src, np.int64)
    ys, xs = np.divmod(src, w)
    K = np.asarray(K_level, np.float64).reshape(3, 3)
    Z = d[ys, xs].astype(np.float64)
    Xk = np.stack([Z * (xs - K[0, 2]) / K[0, 0], Z * (ys - K[1, 2]) / K[1, 1], Z, np.ones_like(Z)], axis=1)
    T = np.asarray(T_kf, np.float64).reshape(4, 4)
    Ti = np.linalg.inv(T)
    ref = (Xk @ Ti.T)[:, :3]
    wrong = (Xk @ T.T)[:, :3]
    X32, Y32, Z32 = kref.back_project(kref.intr(K_level), xs.astype(F32), ys.astype(F32), d[ys, xs])
    rep = np.stack(kref.transform(Ti.astype(F32), X32, Y32, Z32), axis=1)
    exported = np.asarray(exported, np.float64).reshape(-1, 3)
    bound = 16 * 2.0 ** -24 * (np.abs(Xk[:, :3]).sum(axis=1) + np.abs(Ti[:3, 3]).sum())
    return dict(exported=float(np.median(surface_distance(exported))), reference=float(np.median(surface_distance(ref))),
                replica32=float(np.median(surface_distance(rep))), wrong=float(np.median(surface_distance(wrong))),
                chain_worst_ratio=float((np.abs(exported - ref).max(axis=1) / bound).max()), n=int(len(src)))


def convention_cpu():
    """the replica's figures with the ground-truth pose of frame CONVENTION['keyframe'] in place of the tracked one (no GPU)"""
    import orc
    from dvo_amd import synth
    K = synth.K_640.copy(); K[:2] *= 0.5
    g, d, s, poses = synth.sequence(6, width=320, height_px=240, K=K, seed=42, sigma_value=0.5)
    k = CONVENTION["keyframe"]
    top = orc.cull_image(d.numpy()[k], 1)
    Kt = level_K(K, 1, 3, 2)
    T_kf = np.linalg.inv(poses[k])                    # world -> keyframe camera
    xyzg, src, _ = export_sequence(top, top, Kt, poses[k].astype(F32), min_depth=0.2)
    return convention_figures(top, Kt, T_kf, src, xyzg[:, :3])
