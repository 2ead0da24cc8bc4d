"""Reference of the robust residual weights (dvo_batch_set_robust_weights, include/dvo.h) on the oracle's per-pixel terms.

The contract is float32 arithmetic on values the device and the oracle share bit for bit (J[6], r, rw of orc.optimize_terms), so the
weight rho of every pixel and the weighted per-pixel terms Jr[p] * J[q], Jr[p] * rw, (rho * r) * r are restated here with numpy float32
operations (each correctly rounded, as the device's) and summed exactly in float64.  Only the device's reduction differs, and its shape
is the plain kernel's: the per-entry bound is tests/gn_sums.py's (assert_entries), with the depth it reads off the code.  This module
owns the weights, the weighted exact sums and the scale rule; replay_call hands them to tests/term_replay.py's walker and irls_track
to its tracking loop.  Nothing here is tuned on a device result.  Test infrastructure only."""
from fractions import Fraction

import numpy as np

import gn_sums
import orc
import term_replay

NONE, HUBER, STUDENT_T = 0, 1, 2
ADAPTIVE, GIVEN = 0, 1
F32 = np.float32
INF = F32(np.inf)

_nonempty_calls = 0


def nonempty_calls():
    """how often assert_sums has passed on a non-empty term list (as gn_sums.nonempty_calls: a skipped helper fails its test)"""
    return _nonempty_calls


def fmaf(a, b, c):
    """fmaf(a, b, c) of float32 arrays, correctly rounded.  a * b is exact in float64; the sum is rounded to float64 and then to
    float32, which differs from the single rounding only when the float64 value sits exactly on a float32 midpoint (low 29 mantissa
    bits 0x10000000) -- those elements are redone in exact rational arithmetic."""
    a = np.asarray(a, F32); b = np.asarray(b, F32); c = np.asarray(c, F32)
    a, b, c = np.broadcast_arrays(a, b, c)
    with np.errstate(all="ignore"):
        t = a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)
        out = t.astype(F32)
    bits = np.ascontiguousarray(t).view(np.uint64)
    risky = np.isfinite(t) & ((bits & np.uint64(0x1FFFFFFF)) == np.uint64(0x10000000))
    if risky.any():
        out = out.copy()
        for i in zip(*np.nonzero(risky)):
            exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
            lo = F32(np.nextafter(out[i], -INF)); hi = F32(np.nextafter(out[i], INF))
            best = min((lo, out[i], hi), key=lambda v: (abs(Fraction(float(v)) - exact), int(np.array(v, F32).view(np.uint32)) & 1))
            out[i] = best
    return out


def entry(kind, param, s2):
    """(kind_eff, A, B, s2_eff): the constants of one sequence and iteration; plain (NONE, s2 = +inf) unless s2 is finite and > 0"""
    s2 = F32(s2)
    if kind == NONE or not (s2 > 0) or not np.isfinite(s2):
        return NONE, F32(0), F32(0), INF
    p = F32(param)
    if kind == HUBER:
        return HUBER, p * np.sqrt(s2, dtype=F32), F32(0), s2
    return STUDENT_T, (p + F32(1)) * s2, p * s2, s2


def rho(kind, param, s2, r):
    """the weight of every residual in r (float32), by the contract's float32 operations"""
    r = np.asarray(r, F32)
    k, A, B, _ = entry(kind, param, s2)
    if k == NONE:
        return np.ones_like(r)
    with np.errstate(all="ignore"):
        if k == HUBER:
            ar = np.abs(r)
            return np.where(ar <= A, F32(1), (A / ar).astype(F32)).astype(F32)
        return (A / fmaf(r, r, np.full_like(r, B))).astype(F32)


def exact_sums(terms, kind, param, s2):
    """gn_sums.exact_sums of the weighted terms: float64 sums of Jr[a] * J[b] (Jr = rho * J rounded to float32), Jr[a] * rw and
    (rho * r rounded to float32) * r, and beside each the sum of the absolute values of its terms"""
    J32 = np.ascontiguousarray(terms["J"], F32).reshape(-1, 6)
    r32 = np.ascontiguousarray(terms["r"], F32); rw32 = np.ascontiguousarray(terms["rw"], F32)
    w = rho(kind, param, s2, r32)
    Jr = (w[:, None] * J32).astype(np.float64)
    wr = (w * r32).astype(np.float64)
    J = J32.astype(np.float64); r = r32.astype(np.float64); rw = rw32.astype(np.float64)
    H = np.zeros(21); A_H = np.zeros(21); g = np.zeros(6); A_g = np.zeros(6)
    k = 0
    for a in range(6):
        for b in range(a, 6):
            p = Jr[:, a] * J[:, b]
            H[k] = p.sum(); A_H[k] = np.abs(p).sum(); k += 1
        p = Jr[:, a] * rw
        g[a] = p.sum(); A_g[a] = np.abs(p).sum()
    p = wr * r
    return dict(H=H, g=g, sum_r2=float(p.sum()), A_H=A_H, A_g=A_g, A_r=float(np.abs(p).sum()), n=int(J.shape[0]), rho=w)


def assert_sums(got, terms, kind, param, s2, depth, tag=""):
    """`got` (H, g, sum_r2, n_valid of the device) against the exact weighted sums, per entry inside gn_sums.bounds; an entry whose
    absolute sum is zero must be exactly zero; n_valid is the term count.  Returns the exact sums."""
    global _nonempty_calls
    ex = exact_sums(terms, kind, param, s2)
    assert int(got["n_valid"]) == ex["n"], "%s: n_valid %d, %d terms" % (tag, int(got["n_valid"]), ex["n"])
    worst = gn_sums.assert_entries(gn_sums.sum_groups(got, ex, *gn_sums.bounds(ex, depth)), depth, tag)
    if ex["n"] > 0:
        _nonempty_calls += 1
    gn_sums.RATIOS.append(("robust " + str(tag), worst))
    return ex


def adaptive_s2(residual_prev, floor2):
    """the ADAPTIVE rule: s2 of an iteration from the sequence's previous logged residual (None: the first iteration of the coarsest
    level); +inf = plain"""
    if residual_prev is None or not (F32(residual_prev) > 0):
        return INF
    rp = F32(residual_prev); f2 = F32(floor2)
    return rp if rp > f2 else f2


def replay_call(log, terms_at, levels, kind, param, mode, floor2=None, given_s2=None, tag="", depth=17):
    """One whole tracking call from its track log.  terms_at(level, xi) -> orc.optimize_terms at that level and input pose.  Every
    logged iteration: the input pose is the previous xi_after (zero at the start), s2 follows the scale rule (ADAPTIVE: from the previous
    logged residual; GIVEN: given_s2), n_valid equals the term count, the logged residual is (float)sum_r2 / n of the weighted sums to
    the reduction bound, and the logged update solves the weighted normal equations within TOL_BACKWARD.
    depth: the reduction depth that places the logged residual, one value or one per level (gn_sums.plan_depths).
    Returns (terms, s2) of the finest level's last iteration and the number of iterations replayed."""
    walk = term_replay.Replay(log, levels, tag=tag)
    prev = None
    last = None
    for st in walk:
        s2 = adaptive_s2(prev, floor2) if mode == ADAPTIVE else entry(kind, param, given_s2)[3]
        t = terms_at(st.l, st.xi)
        st.check(exact_sums(t, kind, param, s2), gn_sums.factor(gn_sums.at_level(depth, st.l)))
        last = (t, s2, st.l, st.it)
        prev = st.res
    return last, walk.n_it


def oracle_terms(obj, ref, crop):
    """terms_at for two orc.OFrame"""
    return lambda l, xi: orc.optimize_terms(obj.gray(l), ref.gray(l), ref.depth(l), ref.sigma(l), ref.K(l), xi, l, crop=crop)


def irls_track(obj, ref, levels, kind, param, floor2, crop, max_iterations, min_update, min_residual=0.0):
    """A numpy replica of one ADAPTIVE tracking call on the oracle: orc.optimize_terms, the weighted sums in float64, orc.solve6,
    orc.se3_concatenate and the stop tests of tracker.cpp:68-73.  kind = NONE is orc.track.  Returns (xi, log)."""
    prev = None

    def evaluate(l, xi):
        nonlocal prev
        t = orc.optimize_terms(obj.gray(l), ref.gray(l), ref.depth(l), ref.sigma(l), ref.K(l), xi, l, crop=crop)
        ex = exact_sums(t, kind, param, adaptive_s2(prev, floor2) if kind != NONE else INF)
        upd, prev = term_replay.gn_step(ex["n"], ex["H"], ex["g"], ex["sum_r2"])
        return upd, prev, dict(n_valid=ex["n"])
    return term_replay.track(levels, max_iterations, min_update, min_residual, evaluate)
