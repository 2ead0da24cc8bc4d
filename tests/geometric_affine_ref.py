"""Reference of the geometric term composed with affine brightness compensation (dvo_batch_set_geometric_affine, include/dvo.h,
DESIGN.md §27).

Nothing is restated a second time: the warp, the gates and the pieces of the geometric row are geometric_ref.pixels' (the tracked
frame's own depth and sigma), and the compensated terms c = fmaf(a, I1, b), r = I2 - c, rw = r * wgt and the brightness moments are
affine_ref's float32 restatement (fmaf is robust_ref's) on the same contributing pixels -- pixels() asserts that the two helpers see
the same pixels and the same weights, bit for bit.  Every product is summed exactly in float64, beside the sum of its absolute
values; only the device's reduction differs.

Reduction depths, from the code (gn_tile with both flags): H and g take the photometric add and the geometric add of every main-loop
pixel and the photometric add of every deferred pixel, 3 * ppt + 9 as in DESIGN.md §25; sum_r2 keeps 2 * ppt + 9; S29 has ppt + 9; n_geo
is exact.  The moments are accumulated in the main loop and in the deferred loop and reduced like the 29 sums: 2 * ppt + 9 as in
DESIGN.md §24.  Nothing here is tuned on a device result.  Test infrastructure only."""
import numpy as np

import affine_ref as ar
import geometric_ref as gr
import gn_sums
import orc
from util import TOL_BACKWARD, assert_composed, backward_error

F32 = np.float32
ESTIMATE, GIVEN = ar.ESTIMATE, ar.GIVEN
GUARDS = ar.GUARDS

_nonempty_calls = 0


def nonempty_calls():
    """how often a helper here has passed on an evaluation with at least one geometric row (a skipped helper fails its test)"""
    return _nonempty_calls


def moment_depth(ppt=4):
    return 2 * ppt + 9


def pixels(obj_gray, obj_depth, obj_sigma, ref_gray, ref_depth, K, xi, level, crop, wp):
    """geometric_ref.pixels, and under "aff" affine_ref.pixels of the same evaluation (own-depth inputs): the same contributing pixels
    and weights.  wp: geometric_ref.weight_params."""
    px = dict(gr.pixels(obj_gray, obj_depth, obj_sigma, ref_gray, ref_depth, K, xi, level, crop, wp))
    aff = ar.pixels(obj_gray, ref_gray, obj_depth, obj_sigma, K, xi, level, crop, wp[:3])
    assert np.array_equal(aff["index"], px["index"]) and aff["wgt"].tobytes() == px["wgt"].tobytes(), "the two helpers disagree on the pixels"
    px["aff"] = aff
    return px


def compensated(px, a, b):
    """px with the photometric terms against the compensated brightness (geometric_ref's functions then see those)"""
    q = dict(px)
    q["terms"] = ar.terms(px["aff"], a, b)
    return q


def exact(px, weight, max_diff, a, b):
    """geometric_ref.exact of the compensated terms (combined H and g, photometric sum_r2, S29, n_geo) and affine_ref's exact moments
    M / A_M without robust weights"""
    ex = gr.exact(compensated(px, a, b), weight, max_diff)
    m = ar.exact(px["aff"], a, b)
    ex["M"], ex["A_M"] = m["M"], m["A_M"]
    return ex


def assert_step(got, px, weight, max_diff, a, b, ppt=4, guards=GUARDS, tag=""):
    """One evaluation of the operator with the entry (a, b) (an entry that is not finite or has a <= 0 is (1, 0)): the 28 sums, S29,
    n_valid and n_geo (geometric_ref.assert_exact), the moments and the next entry (affine_ref).  Returns the exact sums."""
    global _nonempty_calls
    ex = exact(px, weight, max_diff, a, b)
    gr.assert_exact(got, ex, ppt, tag)
    ar.assert_moments(got["moments"], ex, moment_depth(ppt), False, tag)
    ar.assert_next(got["next_ab"], ex, moment_depth(ppt), False, guards, (F32(a), F32(b)), tag)
    if ex["n_geo"] > 0:
        _nonempty_calls += 1
    return ex


def replay_call(log, glog, alog, pixels_at, levels, weight, max_diff, mode, given_ab=None, guards=GUARDS, ppt=4, xi0=None, tag=""):
    """One whole tracking call from its track log, its geometric log and its affine log.  pixels_at(level, xi) -> pixels().  Every
    logged iteration, at the logged input pose and the logged (a, b): n_valid and n_geo EQUAL the replica's, the logged residual and
    (float)S29 are inside the reduction bound, the logged update solves the replayed combined (H, g) within TOL_BACKWARD, and the next
    logged (a, b) is the closed form of the replayed moments inside the propagated bound (ESTIMATE; the first one is the priming
    entry, the closed form at the start pose from (1, 0)) or the given row (GIVEN).
    ppt: the pixels per thread the levels ran, one value or one per level (Batch.level_plan).
    Returns (exact sums, (a, b)) of the last iteration and the number of iterations replayed."""
    global _nonempty_calls
    xi = np.zeros(6, F32) if xi0 is None else np.asarray(xi0, F32).copy()
    iters = [int(n) for n in log["n_iter"][:levels]]
    assert int(glog["levels"]) == levels and [int(n) for n in glog["n_iter"][:levels]] == iters, (tag, "geometric log", glog["n_iter"], iters)
    assert int(alog["levels"]) == levels and [int(n) for n in alog["n_iter"][:levels]] == iters, (tag, "affine log", alog["n_iter"], iters)
    one = (F32(1), F32(0))
    if mode == ESTIMATE:
        exp = exact(pixels_at(0, xi), weight, max_diff, 1.0, 0.0)
        ar.assert_next((alog["prime_a"], alog["prime_b"]), exp, moment_depth(gn_sums.at_level(ppt, 0)), False, guards, one, tag + " priming pair")
        want = (F32(alog["prime_a"]), F32(alog["prime_b"]))
    else:
        want = one if given_ab is None else (F32(given_ab[0]), F32(given_ab[1]))
        assert alog["prime_a"] == 0 and alog["prime_b"] == 0, (tag, "no priming pair in GIVEN mode")
    ex_prev = None
    last = None
    n_it = 0
    for l in range(levels):
        assert iters[l] >= 1, "%s: level %d ran no iteration" % (tag, l)
        _, dr, dS = gr.depths(gn_sums.at_level(ppt, l))
        dM = moment_depth(gn_sums.at_level(ppt, l))
        fr = dr * gn_sums.U32 * gn_sums.SECOND_ORDER; fS = dS * gn_sums.U32 * gn_sums.SECOND_ORDER
        for it in range(iters[l]):
            where = "%s level %d iteration %d" % (tag, l, it)
            ab = (F32(alog["a"][l][it]), F32(alog["b"][l][it]))
            if ex_prev is None or mode != ESTIMATE:   # the priming entry / the given row: the device's own bits
                assert ab[0].tobytes() == want[0].tobytes() and ab[1].tobytes() == want[1].tobytes(), (where, ab, want)
            else:
                ar.assert_next(ab, ex_prev[0], ex_prev[2], False, guards, ex_prev[1], where + " (entry from the iteration before)")
            ex = exact(pixels_at(l, xi), weight, max_diff, ab[0], ab[1])
            assert ex["n"] == int(log["n_valid"][l][it]), (where, "n_valid", ex["n"], int(log["n_valid"][l][it]))
            assert ex["n_geo"] == int(glog["n_geo"][l][it]), (where, "n_geo", ex["n_geo"], int(glog["n_geo"][l][it]))
            s29 = F32(glog["sum_sq"][l][it])
            assert abs(float(s29) - ex["S29"]) <= fS * ex["S29"] + float(np.spacing(s29)), (where, "S29", float(s29), ex["S29"])
            res = F32(log["residual"][l][it])
            upd = log["xi_update"][l][it]
            if ex["n"] > 0:
                assert abs(float(res) - ex["sum_r2"] / ex["n"]) <= (fr * ex["A_r"] + 2 * float(np.spacing(F32(ex["sum_r2"])))) / ex["n"] \
                    + float(np.spacing(res)), (where, float(res), ex["sum_r2"] / ex["n"])
                back = backward_error(ex["H"], ex["g"], upd)
                assert back <= TOL_BACKWARD, (where, "backward error %.3g" % back)
                if ex["n_geo"] > 0:
                    _nonempty_calls += 1
            else:
                assert res == F32(-1.0) and not np.any(upd), where
            after = np.asarray(log["xi_after"][l][it], F32)
            if np.all(np.isfinite(orc.se3_concatenate(xi, upd))):
                assert_composed(xi, upd, after, tag=where)
            else:
                assert after.tobytes() == xi.tobytes(), where
            last = (ex, ab)
            ex_prev = (ex, ab, dM)
            xi = after.copy()
            n_it += 1
    return last, n_it


def frame_pixels(obj, ref, crop, wp):
    """pixels_at for two orc.OFrame"""
    return lambda l, xi: pixels(obj.gray(l), obj.depth(l), obj.sigma(l), ref.gray(l), ref.depth(l), ref.K(l), xi, l, crop, wp)


class OwnDepth:
    """The reference the affine estimator sees while the geometric term is on: the reference's gray and K, the tracked frame's own
    depth and sigma (affine_ref.affine_track(obj, OwnDepth(obj, ref), ...) is the weight = 0 anchor)."""

    def __init__(self, obj, ref):
        self.gray, self.K, self.depth, self.sigma = ref.gray, ref.K, obj.depth, obj.sigma


def geometric_affine_track(obj, ref, levels, weight, max_diff, mode, crop, max_iterations, min_update, min_residual=0.0, wp=None,
                           guards=GUARDS, given_ab=(1.0, 0.0)):
    """A numpy replica of one tracking call on the oracle: geometric_ref.geometric_track with the compensated photometric terms, and
    affine_ref.affine_track's alternating estimate -- the priming evaluation at the start pose, then every iteration uses the entry
    the iteration before it wrote.  GIVEN with (1, 0) is geometric_track bit for bit; weight = 0 is affine_track on own-depth inputs
    bit for bit.  Returns (xi, log) with log["ab"] the entry every iteration used."""
    wp = gr.weight_params() if wp is None else wp
    at = frame_pixels(obj, ref, crop, wp)
    seq = gr._seq_sum
    xi = np.zeros(6, F32)
    ab = (F32(given_ab[0]), F32(given_ab[1]))
    if mode == ESTIMATE:
        m = ar.exact(at(0, xi)["aff"], 1.0, 0.0)
        ab, _ = ar.closed_form(m["n"], m["M"], m["n"], guards, (F32(1), F32(0)))
    log = dict(n_iter=[], residual=[], xi_after=[], n_valid=[], n_geo=[], ab=[], prime=ab)
    for l in range(levels):
        res_l, xi_l, nv_l, ng_l, ab_l = [], [], [], [], []
        for it in range(max_iterations):
            px = at(l, xi)
            m = ar.exact(px["aff"], ab[0], ab[1])
            t = m["terms"]
            ab_l.append(ab)
            upd = np.zeros(6, F32); res = F32(-1.0)
            n_geo = 0
            if t["n_valid"] > 0:
                J = t["J"].astype(np.float64); rw = t["rw"].astype(np.float64); r = t["r"].astype(np.float64)
                H = np.array([seq(J[:, p] * J[:, q]) for p in range(6) for q in range(p, 6)])
                g = np.array([seq(J[:, p] * rw) for p in range(6)])
                Jg, rg, rgw, on = gr.rows(px, weight, max_diff)
                n_geo = int(on.sum())
                Jd = Jg.astype(np.float64); wd = rgw.astype(np.float64)
                H = H + np.array([seq(Jd[:, p] * Jd[:, q]) for p in range(6) for q in range(p, 6)])
                g = g + np.array([seq(Jd[:, p] * wd) for p in range(6)])
                upd = orc.solve6(H, g)
                res = F32(F32(seq(r * r)) / F32(t["n_valid"]))
            if mode == ESTIMATE:
                ab, _ = ar.closed_form(m["n"], m["M"], m["n"], guards, ab)
            nxt = orc.se3_concatenate(xi, upd)
            if np.all(np.isfinite(nxt)):
                xi = nxt
            res_l.append(res); xi_l.append(xi.copy()); nv_l.append(t["n_valid"]); ng_l.append(n_geo)
            nrm = float(np.sqrt(np.sum(upd.astype(np.float64) ** 2)))
            if nrm < float(F32(min_update)) or res < F32(min_residual):
                break
        log["n_iter"].append(len(res_l)); log["residual"].append(np.array(res_l, F32)); log["xi_after"].append(np.array(xi_l, F32))
        log["n_valid"].append(np.array(nv_l)); log["n_geo"].append(np.array(ng_l)); log["ab"].append(ab_l)
    return xi, log


# ---- the outcome scene of DESIGN.md §27: §25's weakly textured pair, the tracked frame under another exposure ----------------------
EXPOSURE = (1.10, 0.02)


def outcome_pair(seed, exposure=EXPOSURE):
    """geometric_ref.outcome_pair with frame 1's gray replaced by a* . g + b* (float32; at contrast 0.1 no gray leaves [0, 1])"""
    g, d, s, K, truth = gr.outcome_pair(seed)
    g = g.copy()
    g[1] = (F32(exposure[0]) * g[1] + F32(exposure[1])).astype(F32)
    assert g.min() >= 0.0 and g.max() <= 1.0
    return g, d, s, K, truth
