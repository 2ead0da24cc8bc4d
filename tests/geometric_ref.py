"""Reference of the geometric (depth) term of a sensor-depth batch (dvo_batch_set_geometric, include/dvo.h).

The photometric rows are the oracle's own: orc.optimize_terms(obj_gray, ref_gray, obj_depth, obj_sigma, ...) -- while the term is on,
pixel x of the tracked frame uses that frame's own depth and sigma.  The geometric rows are restated here in numpy float32, one
correctly rounded operation per contract operation (fmaf is robust_ref's), independent of dvo_math.h: back_project / transform /
project for (u, v, Zw), the three bilinear blends on the reference-depth taps, the Jacobian formula with (gzx, gzy), the z-row
correction, lam = weight * iz^2.  self_check() holds this restatement to the oracle: with the GRAY taps in place of the depth taps it
must reproduce the oracle's photometric J and r bit for bit on every fast-path pixel.  Every product is summed exactly in float64,
beside the sum of its absolute values; only the device's reduction differs.

Reduction depth (gn_sums.reduction_depth counts the float32 roundings on the longest path): a thread's main loop now performs TWO
accumulations per pixel into slots 0..26 (the photometric add, then the geometric one), its deferred loop still one (deferred pixels
have no geometric row): 2 * ppt + ppt, then the 6 + 3 of the wave and workgroup steps -- 3 * ppt + 9 (21 for ppt = 4) for H and g.
sum_r2 (slot 27) keeps the plain depth 2 * ppt + 9; S29 has ppt fmafs, a six-step butterfly and three additions: ppt + 9.  n_geo is a
sum of ones below 2^24: exact.  This module owns the geometric rows, their exact sums and what a geometric log adds to a replayed
iteration (replay_step, shared with geometric_affine_ref); the per-entry bound loop is gn_sums.assert_entries, the log walker and the
tracking loop are tests/term_replay.py's.  Nothing here is tuned on a device result.  Test infrastructure only."""
import numpy as np

import gn_sums
import orc
import robust_ref as rr
import term_replay

F32 = np.float32
OFF, ON = 0, 1

_nonempty_calls = 0


def nonempty_calls():
    """how often assert_step has passed with at least one geometric row (a skipped helper fails its test)"""
    return _nonempty_calls


def depths(ppt=4):
    """(H and g, sum_r2, S29): see the module docstring"""
    return 3 * ppt + 9, 2 * ppt + 9, ppt + 9


def weight_params(cfg=None):
    """(step per level, sigma_min, sigma_max, min_depth) of a dvo config (None: the defaults)"""
    if cfg is None:
        import dvo_amd
        cfg = dvo_amd.default_config()
    return (lambda l: cfg.step_level1 if l == 1 else (cfg.step_level2 if l == 2 else cfg.step_default)), cfg.sigma_min, cfg.sigma_max, cfg.min_depth


def blend4(g0, g1, g2, g3, hx, vy):
    omh = (F32(1) - hx).astype(F32); omv = (F32(1) - vy).astype(F32)
    top = rr.fmaf(g1, hx, (g0 * omh).astype(F32))
    bot = rr.fmaf(g3, hx, (g2 * omh).astype(F32))
    return rr.fmaf(bot, vy, (top * omv).astype(F32))


def _taps(img, x0, y0):
    """the 12 plus-shaped taps around (x0, y0) (interior positions only): rows y0-1 .. y0+2"""
    g = lambda dx, dy: img[y0 + dy, x0 + dx]
    return dict(a0=g(0, -1), a1=g(1, -1), bm=g(-1, 0), b0=g(0, 0), b1=g(1, 0), b2=g(2, 0),
                cm=g(-1, 1), c0=g(0, 1), c1=g(1, 1), c2=g(2, 1), d0=g(0, 2), d1=g(1, 2))


def _sample(t, hx, vy):
    """the fast sampler's three blends: value, unhalved x-gradient, unhalved y-gradient"""
    with np.errstate(all="ignore"):
        val = blend4(t["b0"], t["b1"], t["c0"], t["c1"], hx, vy)
        gx = blend4((t["b1"] - t["bm"]).astype(F32), (t["b2"] - t["b0"]).astype(F32), (t["c1"] - t["cm"]).astype(F32),
                    (t["c2"] - t["c0"]).astype(F32), hx, vy)
        gy = blend4((t["c0"] - t["a0"]).astype(F32), (t["c1"] - t["a1"]).astype(F32), (t["d0"] - t["b0"]).astype(F32),
                    (t["d1"] - t["b1"]).astype(F32), hx, vy)
    return val, gx, gy


def _jacobian(fx, fy, X, Y, iz, gx, gy):
    """optimize.cpp:67-77 in the shared-reciprocal form, on float32 arrays"""
    with np.errstate(all="ignore"):
        fgx = (fx * gx).astype(F32); fgy = (fy * gy).astype(F32)
        xz = (X * iz).astype(F32); yz = (Y * iz).astype(F32)
        one = np.ones_like(xz)
        J = np.empty(X.shape + (6,), F32)
        J[:, 0] = fgx * iz
        J[:, 1] = fgy * iz
        J[:, 2] = ((-rr.fmaf(fgy, Y, (fgx * X).astype(F32))) * iz).astype(F32) * iz
        J[:, 3] = -((((fgx * xz).astype(F32) * yz).astype(F32)) + (fgy * rr.fmaf(yz, yz, one)).astype(F32))
        J[:, 4] = (fgx * rr.fmaf(xz, xz, one)).astype(F32) + ((fgy * xz).astype(F32) * yz).astype(F32)
        J[:, 5] = rr.fmaf(fgy, xz, -((fgx * yz).astype(F32)))
    return J


def pixels(obj_gray, obj_depth, obj_sigma, ref_gray, ref_depth, K, xi, level, crop, wp):
    """The contributing pixels of one evaluation at the input pose xi: the oracle's photometric terms on the tracked frame's own depth
    and sigma, and for each of them the pieces of its geometric row that do not depend on (weight, max_diff)."""
    obj_gray = np.ascontiguousarray(obj_gray, F32); obj_depth = np.ascontiguousarray(obj_depth, F32)
    ref_gray = np.ascontiguousarray(ref_gray, F32); ref_depth = np.ascontiguousarray(ref_depth, F32)
    t = orc.optimize_terms(obj_gray, ref_gray, obj_depth, obj_sigma, K, xi, level, crop=crop)
    h, w = ref_gray.shape
    K = np.asarray(K, F32).reshape(3, 3)
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    ifx = F32(1) / fx; ify = F32(1) / fy
    step, smin, smax, min_depth = wp
    idx = t["index"]
    y = (idx // w).astype(np.int64); x = (idx % w).astype(np.int64)
    d = obj_depth.ravel()[idx]
    sig = np.ascontiguousarray(obj_sigma, F32).ravel()[idx]
    wgt = (F32(step(level)) / np.clip(sig, F32(smin), F32(smax))).astype(F32)
    with np.errstate(all="ignore"):
        iz = (F32(1) / d).astype(F32)
        X = ((d * (x.astype(F32) - cx)).astype(F32) * ifx).astype(F32)
        Y = ((d * (y.astype(F32) - cy)).astype(F32) * ify).astype(F32)
        Rt = orc.pose_from_xi(np.asarray(xi, F32), -1.0)
        row = lambda i: rr.fmaf(np.full_like(X, Rt[3 * i]), X, rr.fmaf(np.full_like(X, Rt[3 * i + 1]), Y,
                                                                        rr.fmaf(np.full_like(X, Rt[3 * i + 2]), d, np.full_like(X, Rt[9 + i]))))
        Xw, Yw, Zw = row(0), row(1), row(2)
        izw = (F32(1) / Zw).astype(F32)
        u = ((Xw * fx).astype(F32) * izw).astype(F32) + cx
        v = ((Yw * fy).astype(F32) * izw).astype(F32) + cy
    inter = (u >= 1) & (v >= 1) & (u < F32(w - 2)) & (v < F32(h - 2))
    x0 = np.where(inter, u, 1).astype(np.int64); y0 = np.where(inter, v, 1).astype(np.int64)
    hx = (u - x0.astype(F32)).astype(F32); vy = (v - y0.astype(F32)).astype(F32)
    tg = _taps(ref_gray, x0, y0); tz = _taps(ref_depth, x0, y0)
    gray_ok = inter.copy()
    z_ok = np.ones_like(inter)
    with np.errstate(all="ignore"):
        for k in tg:
            gray_ok &= tg[k] > orc.INVALID            # (false for NaN)
            z_ok &= np.isfinite(tz[k]) & (tz[k] >= F32(min_depth))
    Zs, gzx, gzy = _sample(tz, hx, vy)
    with np.errstate(all="ignore"):
        rz = (Zs - Zw).astype(F32)
    Jz = _jacobian(fx, fy, X, Y, iz, gzx, gzy)
    with np.errstate(all="ignore"):
        Jz[:, 2] = Jz[:, 2] - F32(1)
        Jz[:, 3] = Jz[:, 3] - Y
        Jz[:, 4] = Jz[:, 4] + X
    return dict(terms=t, n_valid=t["n_valid"], index=idx, wgt=wgt, iz=iz, rz=rz, Jz=Jz, fast=gray_ok, z_ok=z_ok,
                u=u, v=v, x=x, y=y, d=d, X=X, Y=Y, hx=hx, vy=vy, gray_taps=tg, K=(fx, fy), shape=(h, w))


def self_check(px, obj_gray):
    """The restated warp, sampler and Jacobian against the oracle: on every fast-path pixel, the gray taps through the same code give
    the oracle's own J and r bit for bit.  Returns the number of pixels compared."""
    t = px["terms"]; m = px["fast"]
    I2, gx, gy = _sample(px["gray_taps"], px["hx"], px["vy"])
    J = _jacobian(px["K"][0], px["K"][1], px["X"], px["Y"], px["iz"], gx, gy)
    I1 = np.ascontiguousarray(obj_gray, F32).ravel()[px["index"]]
    r = (I2 - I1).astype(F32)
    assert J[m].tobytes() == t["J"][m].tobytes(), "the restated Jacobian differs from the oracle's on a fast-path pixel"
    assert r[m].tobytes() == t["r"][m].tobytes() and (r * px["wgt"]).astype(F32)[m].tobytes() == t["rw"][m].tobytes(), \
        "the restated residual or weight differs from the oracle's on a fast-path pixel"
    return int(m.sum())


def rows(px, weight, max_diff):
    """The geometric rows: (Jg [n_geo][6], rg, rgw) of the pixels that have one, and their mask over the contributing pixels."""
    with np.errstate(all="ignore"):
        on = px["fast"] & px["z_ok"] & (np.abs(px["rz"]) <= F32(max_diff))
    lam = (F32(weight) * (px["iz"][on] * px["iz"][on]).astype(F32)).astype(F32)
    Jg = (lam[:, None] * px["Jz"][on]).astype(F32)
    rg = (lam * px["rz"][on]).astype(F32)
    rgw = (rg * px["wgt"][on]).astype(F32)
    return Jg, rg, rgw, on


def exact(px, weight, max_diff):
    """Exact float64 sums of both rows and, beside each, the sum of the absolute values of its terms: H (21), g (6) combined;
    sum_r2 photometric; S29 = sum rg^2; n = n_valid, n_geo."""
    ex = gn_sums.exact_sums(px["terms"])
    Jg, rg, rgw, on = rows(px, weight, max_diff)
    J = Jg.astype(np.float64); w = rgw.astype(np.float64)
    k = 0
    for a in range(6):
        for b in range(a, 6):
            p = J[:, a] * J[:, b]
            ex["H"][k] += p.sum(); ex["A_H"][k] += np.abs(p).sum(); k += 1
        p = J[:, a] * w
        ex["g"][a] += p.sum(); ex["A_g"][a] += np.abs(p).sum()
    ex["S29"] = float((rg.astype(np.float64) ** 2).sum())
    ex["n_geo"] = int(on.sum())
    ex["Jg"], ex["rg"], ex["rgw"], ex["on"] = Jg, rg, rgw, on
    return ex


def assert_exact(got, ex, ppt=4, tag=""):
    """`got` (H, g, sum_r2, n_valid, n_geo, sum_sq of the device) against exact() output: n_valid and n_geo equal, every sum finite and
    inside gn_sums.bounds at the depths of depths(); an entry whose absolute sum is zero must be exactly zero.  Returns the largest
    error / bound ratio."""
    assert int(got["n_valid"]) == ex["n"], "%s: n_valid %d, %d terms" % (tag, int(got["n_valid"]), ex["n"])
    assert int(got["n_geo"]) == ex["n_geo"], "%s: n_geo %d, %d geometric rows" % (tag, int(got["n_geo"]), ex["n_geo"])
    dH, dr, dS = depths(ppt)
    bH, bg, _ = gn_sums.bounds(ex, dH)
    br = gn_sums.bounds(ex, dr)[2]
    bS = gn_sums.factor(dS) * ex["S29"]
    # (S29 as a float of the log: one more rounding)
    bS += float(np.spacing(F32(ex["S29"]))) if got.get("sum_sq_is_float") else 0.0
    groups = gn_sums.sum_groups(got, ex, bH, bg, br) + [("S29", [got["sum_sq"]], [ex["S29"]], [bS])]
    for name, val, _, _ in groups:
        assert np.isfinite(np.asarray(val, np.float64)).all(), "%s: %s of the device is not finite" % (tag, name)
    worst = gn_sums.assert_entries(groups, "%d for H and g, %d for sum_r2, %d for S29" % (dH, dr, dS), tag)
    gn_sums.RATIOS.append(("geometric " + str(tag), worst))
    return worst


def assert_step(got, px, weight, max_diff, ppt=4, tag=""):
    """One evaluation against the exact sums of pixels() output (assert_exact).  Returns the exact sums."""
    global _nonempty_calls
    ex = exact(px, weight, max_diff)
    assert_exact(got, ex, ppt, tag)
    if ex["n_geo"] > 0:
        _nonempty_calls += 1
    return ex


def replay_call(log, glog, pixels_at, levels, weight, max_diff, ppt=4, xi0=None, tag=""):
    """One whole tracking call from its track log and its geometric log.  pixels_at(level, xi) -> pixels() at that level and input
    pose.  Every logged iteration, at the logged input pose: n_valid and n_geo EQUAL the replica's, the logged residual and the logged
    (float)S29 are inside the reduction bound, and the logged update solves the replayed combined (H, g) within TOL_BACKWARD.
    ppt: the pixels per thread the levels ran, one value or one per level (Batch.level_plan).
    Returns the exact sums of the last iteration and the number of iterations replayed."""
    global _nonempty_calls
    walk = term_replay.Replay(log, levels, xi0, tag)
    term_replay.assert_indexed_like(glog, log, levels, "geometric", tag)
    last = None
    for st in walk:
        last = ex = exact(pixels_at(st.l, st.xi), weight, max_diff)
        if replay_step(st, glog, ex, ppt):
            _nonempty_calls += 1
    return last, walk.n_it


def replay_step(st, glog, ex, ppt):
    """One iteration of term_replay's walker with a geometric log: n_geo EQUALS the replica's and the logged (float)S29 is inside the
    reduction bound, then the walker's own checks at sum_r2's depth.  True where the evaluation had a geometric row."""
    _, dr, dS = depths(gn_sums.at_level(ppt, st.l))
    n_geo = int(glog["n_geo"][st.l][st.it])
    assert ex["n_geo"] == n_geo, (st.where, "n_geo", ex["n_geo"], n_geo)
    s29 = F32(glog["sum_sq"][st.l][st.it])
    assert abs(float(s29) - ex["S29"]) <= gn_sums.factor(dS) * ex["S29"] + float(np.spacing(s29)), (st.where, "S29", float(s29), ex["S29"])
    st.check(ex, gn_sums.factor(dr))
    return ex["n"] > 0 and ex["n_geo"] > 0


def frame_pixels(obj, ref, crop, wp, own_depth=True):
    """pixels_at for two orc.OFrame; own_depth = False: the reference's depth and sigma at pixel x (the plain estimator's inputs)"""
    src = obj if own_depth else ref
    return lambda l, xi: pixels(obj.gray(l), src.depth(l), src.sigma(l), ref.gray(l), ref.depth(l), ref.K(l), xi, l, crop, wp)


def combined_step(px, t, weight, max_diff):
    """(update, residual, n_geo) of one evaluation: the photometric products of the terms t summed in double in raster order (the
    oracle's own loop), the geometric products of px's rows added to them, orc.solve6; the residual is the photometric one"""
    J = t["J"].astype(np.float64); rw = t["rw"].astype(np.float64); r = t["r"].astype(np.float64)
    H, g = term_replay.raster_sums(J, J, rw)
    Jg, rg, rgw, on = rows(px, weight, max_diff)
    Jd = Jg.astype(np.float64); wd = rgw.astype(np.float64)
    Hg, gg = term_replay.raster_sums(Jd, Jd, wd)
    return term_replay.gn_step(t["n_valid"], H + Hg, g + gg, term_replay.seq_sum(r * r)) + (int(on.sum()),)


def geometric_track(obj, ref, levels, weight, max_diff, crop, max_iterations, min_update, min_residual=0.0, wp=None, own_depth=True):
    """A numpy replica of one tracking call on the oracle: pixels(), the photometric products summed in double in raster order (the
    oracle's own loop), the geometric products added to them, orc.solve6, orc.se3_concatenate and the stop tests of tracker.cpp:68-73.
    weight = 0 with own_depth = False is orc.track bit for bit.  Returns (xi, log)."""
    wp = weight_params() if wp is None else wp
    at = frame_pixels(obj, ref, crop, wp, own_depth)

    def evaluate(l, xi):
        px = at(l, xi)
        upd, res, n_geo = combined_step(px, px["terms"], weight, max_diff)
        return upd, res, dict(n_valid=px["terms"]["n_valid"], n_geo=n_geo)
    return term_replay.track(levels, max_iterations, min_update, min_residual, evaluate)


# ---- the outcome scene of DESIGN.md §25: a weakly textured pair with sensor noise ---------------------------------------------------
OUTCOME = dict(width=320, height=240, levels=3, culls=1, contrast=0.1, gray_sigma=0.01, depth_sigma=0.002, sigma_t=0.03, sigma_r_deg=1.0,
               seeds=(42, 43, 44, 45), steps=(1.0, 0.75, 0.5), min_residual=0.0, min_update=2e-5, max_iterations=15)


def outcome_pair(seed):
    """(gray [2][h][w], depth, sigma, K, the true twist of frame 1 against frame 0) of one seed of the outcome scene: synth's pair with
    the gray contrast reduced around 0.5, Gaussian gray noise and depth noise growing with z^2, from a RandomState seeded here."""
    from dvo_amd import synth
    o = OUTCOME
    K = synth.K_640.copy(); K[:2] *= 0.5
    g, d, s, poses = synth.sequence(2, o["width"], o["height"], K, seed, sigma_value=0.5, sigma_t=o["sigma_t"], sigma_r_deg=o["sigma_r_deg"])
    g = g.numpy().astype(np.float64); d = d.numpy().astype(np.float64); s = s.numpy()
    rng = np.random.RandomState(1000 + seed)
    g = 0.5 + o["contrast"] * (g - 0.5) + rng.normal(0.0, o["gray_sigma"], g.shape)
    d = d + rng.normal(0.0, 1.0, d.shape) * o["depth_sigma"] * d * d
    truth = orc.se3_log(np.linalg.inv(poses[1]) @ poses[0])
    return g.astype(F32), d.astype(F32), s.astype(F32), K, truth


def pose_error(xi, truth):
    return float(np.sqrt(np.sum((np.asarray(xi, np.float64) - np.asarray(truth, np.float64)) ** 2)))
