"""Reference of the affine brightness compensation (dvo_batch_set_affine_brightness, include/dvo.h) on the oracle's
per-pixel terms.

The contract is float32 arithmetic on values the device and the oracle share bit for bit.  I1 = obj_gray[index]; I2 is the r of a second
orc.optimize_terms call whose object image has every valid pixel set to 0.0 (r = I2 - 0 exactly; 0 is a valid gray, kInvalid being -2),
with J and the contributing set asserted equal in both calls; wgt is gn_weight's expression in float32.  The compensated residual, the
weights and the moments are restated with numpy float32 operations (each correctly rounded; fmaf is robust_ref's) and every product is
summed exactly in float64, beside the sum of its absolute values.  Only the device's reduction differs: the 29 sums keep the depth of
DESIGN.md §6, and the moments are reduced in the same shape -- 2 * ppt per-thread accumulations (main loop and deferred loop), a six-step
butterfly over the wave, three additions over the four waves, the tiles in double -- so the same depth holds for them
(gn_sums.reduction_depth).  The bound of the next entry is propagated from the moment bounds through the closed form: it is evaluated at
the ends of the moment intervals, and one float ulp is added for the cast.  This module owns the compensated terms, the moments, the
closed form and the entry chain (EntryChain, shared with geometric_affine_ref); the per-entry bound loop is gn_sums.assert_entries,
the log walker and the tracking loop are tests/term_replay.py's.  Nothing here is tuned on a device result.  Test infrastructure only."""
import itertools

import numpy as np

import gn_sums
import orc
import robust_ref as rr
import term_replay

OFF, ESTIMATE, GIVEN = 0, 1, 2
F32 = np.float32
GUARDS = dict(min_pixels=64, min_contrast=1e-3, gain_min=0.25, gain_max=4.0)   # the binding's defaults

_nonempty_calls = 0


def nonempty_calls():
    """how often assert_step has passed on a non-empty term list (as gn_sums.nonempty_calls: a skipped helper fails its test)"""
    return _nonempty_calls


def weight_params(cfg=None):
    """(step per level, sigma_min, sigma_max) of a dvo config (None: the defaults): what gn_weight takes"""
    if cfg is None:
        import dvo_amd
        cfg = dvo_amd.default_config()
    return (lambda l: cfg.step_level1 if l == 1 else (cfg.step_level2 if l == 2 else cfg.step_default)), cfg.sigma_min, cfg.sigma_max


def pixels(obj_gray, ref_gray, ref_depth, ref_sigma, K, xi, level, crop, wp):
    """The contributing pixels of one evaluation: J, I1, I2, wgt (float32) and the plain terms they came from."""
    obj_gray = np.ascontiguousarray(obj_gray, F32)
    t = orc.optimize_terms(obj_gray, ref_gray, ref_depth, ref_sigma, K, xi, level, crop=crop)
    zero = obj_gray.copy()
    zero[zero > orc.INVALID] = F32(0.0)
    t0 = orc.optimize_terms(zero, ref_gray, ref_depth, ref_sigma, K, xi, level, crop=crop)
    assert t0["n_valid"] == t["n_valid"] and np.array_equal(t0["index"], t["index"]) and t0["J"].tobytes() == t["J"].tobytes(), \
        "the contributing set or J depends on the object image's values"
    step, smin, smax = wp
    sig = np.ascontiguousarray(ref_sigma, F32).ravel()[t["index"]]
    wgt = (F32(step(level)) / np.clip(sig, F32(smin), F32(smax))).astype(F32)
    I1 = obj_gray.ravel()[t["index"]]; I2 = t0["r"]
    # (1, 0) is the plain term: the restated pieces reproduce the oracle's own r and rw bit for bit
    assert (I2 - I1).astype(F32).tobytes() == t["r"].tobytes() and (t["r"] * wgt).astype(F32).tobytes() == t["rw"].tobytes(), \
        "I1, I2 and wgt do not reproduce the oracle's r and rw"
    return dict(J=t["J"], I1=I1, I2=I2, wgt=wgt, index=t["index"], n_valid=t["n_valid"], plain=t)


def terms(px, a, b):
    """orc.optimize_terms-shaped terms against the compensated brightness c = fmaf(a, I1, b)"""
    c = rr.fmaf(np.full_like(px["I1"], F32(a)), px["I1"], np.full_like(px["I1"], F32(b)))
    r = (px["I2"] - c).astype(F32)
    return dict(J=px["J"], r=r, rw=(r * px["wgt"]).astype(F32), n_valid=px["n_valid"], index=px["index"])


def _sum(p):
    return float(p.sum()), float(np.abs(p).sum())


def exact(px, a, b, kind=rr.NONE, param=1.0, s2=rr.INF):
    """robust_ref.exact_sums of the compensated terms, and the exact moments (M0, M1, M2, M11, M12) with their absolute sums."""
    t = terms(px, a, b)
    ex = rr.exact_sums(t, kind, param, s2)
    rho = ex["rho"]
    p = (rho * px["I1"]).astype(F32).astype(np.float64)
    I1 = px["I1"].astype(np.float64); I2 = px["I2"].astype(np.float64); w = rho.astype(np.float64)
    pairs = [_sum(w), _sum(p), _sum(w * I2), _sum(p * I1), _sum(p * I2)]
    ex["M"] = np.array([v for v, _ in pairs]); ex["A_M"] = np.array([v for _, v in pairs])
    ex["terms"] = t
    return ex


def closed_form(N, M, n_valid, guards, prev):
    """the next entry from the totals in double; prev where a guard fails.  Returns ((a, b) float32, guards held)."""
    M1, M2, M11, M12 = (float(x) for x in M[1:5])
    N = float(N)
    with np.errstate(all="ignore"):
        det = np.float64(N) * M11 - np.float64(M1) * M1
        an = (np.float64(N) * M12 - np.float64(M1) * M2) / det
        bn = (np.float64(M2) - an * M1) / np.float64(N)
    ok = (n_valid >= guards["min_pixels"] and det > np.float64(F32(guards["min_contrast"])) * N * M11 and np.isfinite(an) and np.isfinite(bn)
          and np.float64(F32(guards["gain_min"])) <= an <= np.float64(F32(guards["gain_max"])))
    if not ok:
        return (F32(prev[0]), F32(prev[1])), False
    return (F32(an), F32(bn)), True


def next_entry_bounds(ex, depth, robust, guards, prev):
    """(lo[2], hi[2], verdicts): the closed form at every end of the moment intervals (N = M0 with robust weights, else the exact
    n_valid), widened by one float32 ulp for the cast; verdicts = the set of guard outcomes met on the way."""
    f = gn_sums.factor(depth)
    iv = [(ex["M"][k] - f * ex["A_M"][k], ex["M"][k] + f * ex["A_M"][k]) for k in range(5)]
    if not robust:
        iv[0] = (float(ex["n"]), float(ex["n"]))
    vals, verdicts = [], set()
    for corner in itertools.product(*[sorted(set(x)) for x in iv]):
        ab, ok = closed_form(corner[0], corner, ex["n"], guards, prev)
        verdicts.add(ok)
        vals.append(ab)
    vals = np.array(vals, np.float64)
    lo, hi = vals.min(axis=0), vals.max(axis=0)
    ulp = np.array([float(np.spacing(F32(max(abs(lo[k]), abs(hi[k]))))) for k in range(2)])
    return lo - ulp, hi + ulp, verdicts


def assert_moments(got, ex, depth, robust, tag=""):
    """device moments (N, M1, M2, M11, M12 in double) per entry inside depth * 2^-24 * (1 + 2^-10) * A; N is exact without weights"""
    got = np.asarray(got, np.float64)
    if not robust:
        assert got[0] == ex["n"], (tag, "N", got[0], ex["n"])
    f = gn_sums.factor(depth)
    worst = gn_sums.assert_entries([("moment %d" % k, [got[k]], [ex["M"][k]], [f * ex["A_M"][k]]) for k in range(0 if robust else 1, 5)], depth, tag)
    gn_sums.RATIOS.append(("affine moments " + str(tag), worst))


def assert_next(got_ab, ex, depth, robust, guards, prev, tag=""):
    """the entry a solve wrote against the closed form of the replayed moments, inside the propagated bound"""
    lo, hi, verdicts = next_entry_bounds(ex, depth, robust, guards, prev)
    got = np.asarray(got_ab, F32)
    keeps = got.tobytes() == np.asarray(prev, F32).tobytes()
    inside = bool(np.all(got.astype(np.float64) >= lo) and np.all(got.astype(np.float64) <= hi))
    if verdicts == {True}:
        assert inside, (tag, "next entry", got, lo, hi)
    elif verdicts == {False}:
        assert keeps, (tag, "a guard fails: the entry keeps its value", got, prev)
    else:   # a guard sits inside the interval: either outcome is the contract's
        assert inside or keeps, (tag, got, lo, hi, prev)
    return verdicts


def assert_step(got, moments, next_ab, px, a, b, kind, param, s2, depth, guards=GUARDS, tag=""):
    """One evaluation with the entry (a, b): the 29 sums (robust_ref.assert_sums on the compensated terms), the moments and the next entry."""
    global _nonempty_calls
    ex = exact(px, a, b, kind, param, s2)
    rr.assert_sums(got, ex["terms"], kind, param, s2, depth, tag)
    robust = kind != rr.NONE
    if moments is not None:
        assert_moments(moments, ex, depth, robust, tag)
    if next_ab is not None:
        assert_next(next_ab, ex, depth, robust, guards, (F32(a), F32(b)), tag)
    if ex["n"] > 0:
        _nonempty_calls += 1
    return ex


class EntryChain:
    """The logged (a, b) of one call against the rule (replay_call here and geometric_affine_ref's): the first entry is the priming pair
    (ESTIMATE) and every entry the given row (GIVEN) in the device's own bits; a later ESTIMATE entry is the closed form of the moments
    of the iteration before, inside the propagated bound (assert_next)."""

    def __init__(self, alog, mode, given_ab, guards, tag):
        self.alog, self.mode, self.guards, self.tag = alog, mode, guards, tag
        self.prev = None   # (exact sums, (a, b), moment depth) of the iteration before
        if mode == ESTIMATE:
            self.want = (F32(alog["prime_a"]), F32(alog["prime_b"]))
        else:
            self.want = (F32(1), F32(0)) if given_ab is None else (F32(given_ab[0]), F32(given_ab[1]))
            assert alog["prime_a"] == 0 and alog["prime_b"] == 0, (tag, "no priming pair in GIVEN mode")

    def prime(self, ex, depth):
        """the priming pair: the closed form at the start pose from (1, 0) with rho = 1 (ex: the exact moments there)"""
        assert_next((self.alog["prime_a"], self.alog["prime_b"]), ex, depth, False, self.guards, (F32(1), F32(0)), self.tag + " priming pair")

    def entry(self, st, robust=False):
        """the checked (a, b) that iteration st of the walker used"""
        ab = (F32(self.alog["a"][st.l][st.it]), F32(self.alog["b"][st.l][st.it]))
        if self.prev is None or self.mode != ESTIMATE:   # the priming entry / the given row: the device's own bits
            assert ab[0].tobytes() == self.want[0].tobytes() and ab[1].tobytes() == self.want[1].tobytes(), (st.where, ab, self.want)
        else:
            assert_next(ab, self.prev[0], self.prev[2], robust, self.guards, self.prev[1], st.where + " (entry from the iteration before)")
        return ab

    def wrote(self, ex, ab, depth):
        """iteration st ran with the entry ab and left the moments of ex, reduced at `depth`"""
        self.prev = (ex, ab, depth)


def replay_call(log, alog, pixels_at, levels, mode, kind=rr.NONE, param=1.0, rob_mode=rr.ADAPTIVE, floor2=None, given_s2=None,
                given_ab=None, guards=GUARDS, depth=17, xi0=None, tag=""):
    """One whole tracking call from its track log and its affine log.  pixels_at(level, xi) -> pixels() at that level and input pose.
    Every logged iteration, at the logged input pose and the logged (a, b): n_valid equals the term count, the logged residual is
    inside the reduction bound, the logged update solves the replayed (H, g) within TOL_BACKWARD, and the NEXT logged (a, b) is the closed
    form of the replayed moments inside the propagated bound (ESTIMATE) or the given row (GIVEN).  ESTIMATE: the first logged entry is
    the priming entry, the closed form at the start pose from (1, 0) with rho = 1.  depth: one value or one per level
    (gn_sums.plan_depths); an entry is held to the depth of the level whose moments it came from.
    Returns (exact sums, (a, b), level, iteration) of the last iteration and the number of iterations replayed."""
    global _nonempty_calls
    walk = term_replay.Replay(log, levels, xi0, tag)
    robust = kind != rr.NONE
    term_replay.assert_indexed_like(alog, log, levels, "affine", tag)
    chain = EntryChain(alog, mode, given_ab, guards, tag)
    if mode == ESTIMATE:
        chain.prime(exact(pixels_at(0, walk.xi), 1.0, 0.0), gn_sums.at_level(depth, 0))
    prev_res = None
    last = None
    for st in walk:
        depth_l = gn_sums.at_level(depth, st.l)
        ab = chain.entry(st, robust)
        s2 = rr.INF
        if robust:
            s2 = rr.adaptive_s2(prev_res, floor2) if rob_mode == rr.ADAPTIVE else rr.entry(kind, param, given_s2)[3]
        ex = exact(pixels_at(st.l, st.xi), ab[0], ab[1], kind, param, s2)
        st.check(ex, gn_sums.factor(depth_l))
        if ex["n"] > 0:
            _nonempty_calls += 1
        last = (ex, ab, st.l, st.it)
        chain.wrote(ex, ab, depth_l)
        prev_res = st.res
    return last, walk.n_it


def oracle_pixels(obj, ref, crop, wp):
    """pixels_at for two orc.OFrame"""
    return lambda l, xi: pixels(obj.gray(l), ref.gray(l), ref.depth(l), ref.sigma(l), ref.K(l), xi, l, crop, wp)


def affine_track(obj, ref, levels, mode, crop, max_iterations, min_update, min_residual=0.0, wp=None, kind=rr.NONE, param=1.0, floor2=None,
                 guards=GUARDS, given_ab=(1.0, 0.0)):
    """A numpy replica of one tracking call on the oracle: pixels(), the sums in double in raster order, orc.solve6,
    orc.se3_concatenate, the stop tests of tracker.cpp:68-73 and the alternating estimate (priming pair included).  mode GIVEN with
    (1, 0) and kind NONE is orc.track bit for bit.  Returns (xi, log) with log["ab"] the entry every iteration used."""
    wp = weight_params() if wp is None else wp
    robust = kind != rr.NONE
    ab = (F32(given_ab[0]), F32(given_ab[1]))
    if mode == ESTIMATE:
        px = pixels(obj.gray(0), ref.gray(0), ref.depth(0), ref.sigma(0), ref.K(0), np.zeros(6, F32), 0, crop, wp)
        ex = exact(px, 1.0, 0.0)
        ab, _ = closed_form(ex["n"], ex["M"], ex["n"], guards, (F32(1), F32(0)))
    prime = ab
    prev = None

    def evaluate(l, xi):
        nonlocal ab, prev
        px = pixels(obj.gray(l), ref.gray(l), ref.depth(l), ref.sigma(l), ref.K(l), xi, l, crop, wp)
        s2 = rr.adaptive_s2(prev, floor2) if robust else rr.INF
        used = ab
        ex = exact(px, ab[0], ab[1], kind, param, s2)
        t = ex["terms"]
        J = t["J"].astype(np.float64)
        Jr = (ex["rho"][:, None] * t["J"]).astype(F32).astype(np.float64) if robust else J
        H, g = term_replay.raster_sums(J, Jr, t["rw"].astype(np.float64))
        wr = (ex["rho"] * t["r"]).astype(F32).astype(np.float64) if robust else t["r"].astype(np.float64)
        upd, prev = term_replay.gn_step(ex["n"], H, g, term_replay.seq_sum(wr * t["r"].astype(np.float64)))
        if mode == ESTIMATE:
            ab, _ = closed_form(ex["M"][0] if robust else ex["n"], ex["M"], ex["n"], guards, ab)
        return upd, prev, dict(n_valid=ex["n"], ab=used)
    xi, log = term_replay.track(levels, max_iterations, min_update, min_residual, evaluate)
    log["prime"] = prime
    return xi, log
