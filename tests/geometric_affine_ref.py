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
DESIGN.md §24.  replay_call and geometric_affine_track compose the pieces only: geometric_ref.replay_step / combined_step,
affine_ref.EntryChain / closed_form, and the log walker and tracking loop of tests/term_replay.py.  Nothing here is tuned on a device
result.  Test infrastructure only."""
import numpy as np

import affine_ref as ar
import geometric_ref as gr
import gn_sums
import term_replay

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
    walk = term_replay.Replay(log, levels, xi0, tag)
    term_replay.assert_indexed_like(glog, log, levels, "geometric", tag)
    term_replay.assert_indexed_like(alog, log, levels, "affine", tag)
    chain = ar.EntryChain(alog, mode, given_ab, guards, tag)
    if mode == ESTIMATE:
        chain.prime(exact(pixels_at(0, walk.xi), weight, max_diff, 1.0, 0.0), moment_depth(gn_sums.at_level(ppt, 0)))
    last = None
    for st in walk:
        ab = chain.entry(st)
        ex = exact(pixels_at(st.l, st.xi), weight, max_diff, ab[0], ab[1])
        if gr.replay_step(st, glog, ex, ppt):
            _nonempty_calls += 1
        last = (ex, ab)
        chain.wrote(ex, ab, moment_depth(gn_sums.at_level(ppt, st.l)))
    return last, walk.n_it


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
    ab = (F32(given_ab[0]), F32(given_ab[1]))
    if mode == ESTIMATE:
        m = ar.exact(at(0, np.zeros(6, F32))["aff"], 1.0, 0.0)
        ab, _ = ar.closed_form(m["n"], m["M"], m["n"], guards, (F32(1), F32(0)))
    prime = ab

    def evaluate(l, xi):
        nonlocal ab
        px = at(l, xi)
        used = ab
        m = ar.exact(px["aff"], ab[0], ab[1])
        upd, res, n_geo = gr.combined_step(px, m["terms"], weight, max_diff)
        if mode == ESTIMATE:
            ab, _ = ar.closed_form(m["n"], m["M"], m["n"], guards, ab)
        return upd, res, dict(n_valid=m["terms"]["n_valid"], n_geo=n_geo, ab=used)
    xi, log = term_replay.track(levels, max_iterations, min_update, min_residual, evaluate)
    log["prime"] = prime
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
