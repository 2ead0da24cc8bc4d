"""Reference of the median (MAD) robust scale (dvo_batch_set_robust_median, include/dvo.h) on the oracle's per-pixel terms.

The bin of a residual, the counts, the selection of the median bin and the s2 it gives are integer and float32 operations, restated
here with numpy on the r of orc.optimize_terms; everything downstream of s2 is tests/robust_ref.py's.  median_track is
robust_ref.irls_track with this rule and the priming evaluation; replay_call replays a device call from its track log and robust log.
Both keep the rule only: the tracking loop and the log walker are tests/term_replay.py's.
Nothing here is tuned on a device result.  Test infrastructure only."""
import numpy as np

import gn_sums
import orc
import robust_ref as rr
import term_replay

NONE, HUBER, STUDENT_T = rr.NONE, rr.HUBER, rr.STUDENT_T
MEDIAN = 2
BINS = 256
K0 = (127 - 16) << 4
F32 = np.float32
INF = F32(np.inf)


def bins(r):
    """the bin of every residual in r: clamp((bits(|r|) >> 19) - K0, 0, 255)"""
    u = np.abs(np.ascontiguousarray(r, F32)).view(np.uint32).astype(np.int64)
    return np.clip((u >> 19) - K0, 0, BINS - 1).astype(np.int64)


def counts(r):
    """uint32 [256]: how many residuals of r fall in each bin"""
    return np.bincount(bins(r).ravel(), minlength=BINS).astype(np.uint32)


def edge(k):
    """the lower edge of bin k (1 <= k <= 255), float32: bits (k + K0) << 19"""
    return np.array([(int(k) + K0) << 19], np.uint32).view(F32)[0]


def select(cnt):
    """(m, n) of 256 counts: n = their sum, m = the smallest bin with cum(m) >= (n + 1) // 2; m = -1 where n == 0"""
    cnt = np.asarray(cnt, np.int64)
    n = int(cnt.sum())
    if n == 0:
        return -1, 0
    return int(np.searchsorted(np.cumsum(cnt), (n + 1) // 2, side="left")), n


def bin_s2(m, floor2):
    """s2 of median bin m: med = the bin's midpoint, s = 1.4826f * med, s2 = max(s * s, floor2), each operation rounded to float32"""
    med = np.array([((int(m) + K0) << 19) | (1 << 18)], np.uint32).view(F32)[0]
    s = F32(F32(1.4826) * med)
    s2 = F32(s * s)
    f2 = F32(floor2)
    return s2 if s2 > f2 else f2


def next_s2(cnt, floor2):
    """the s2 of the entry a solve writes from the counts (+inf: plain), with (m, n)"""
    m, n = select(cnt)
    return (INF if n == 0 else bin_s2(m, floor2)), m, n


def median_track(obj, ref, levels, kind, param, floor2, crop, max_iterations, min_update, min_residual=0.0, force_s2=None):
    """robust_ref.irls_track with the median rule: the priming evaluation at the start pose on the coarsest level gives the first
    iteration's s2, and every iteration's own residuals give the next one's.  force_s2: that scale at every iteration instead
    (+inf: orc.track).  Returns (xi, log); log adds s2, median_bin, count per iteration and prime = (m, n)."""
    xi = np.zeros(6, F32)
    t = orc.optimize_terms(obj.gray(0), ref.gray(0), ref.depth(0), ref.sigma(0), ref.K(0), xi, 0, crop=crop)
    s2, pm, pn = next_s2(counts(t["r"]), floor2)

    def evaluate(l, xi):
        nonlocal s2
        t = orc.optimize_terms(obj.gray(l), ref.gray(l), ref.depth(l), ref.sigma(l), ref.K(l), xi, l, crop=crop)
        used = F32(force_s2) if force_s2 is not None else s2
        ex = rr.exact_sums(t, kind, param, used)
        s2, m, n = next_s2(counts(t["r"]), floor2)
        upd, res = term_replay.gn_step(ex["n"], ex["H"], ex["g"], ex["sum_r2"])
        return upd, res, dict(n_valid=ex["n"], s2=rr.entry(kind, param, used)[3], median_bin=m, count=n)
    xi, log = term_replay.track(levels, max_iterations, min_update, min_residual, evaluate)
    log["prime"] = (pm, pn)
    return xi, log


def assert_selection(rlog, levels, kind, param, floor2, tag=""):
    """The robust log against the contract's rule applied to the log's OWN (m, n): the s2 every iteration used is the entry of the
    previous record (the priming pair's at the start), bit for bit.  Returns the number of iterations checked."""
    prev = (int(rlog["prime_bin"]), int(rlog["prime_count"]))
    n_it = 0
    for l in range(levels):
        for it in range(int(rlog["n_iter"][l])):
            m, n = prev
            want = INF if n == 0 else rr.entry(kind, param, bin_s2(m, floor2))[3]
            got = F32(rlog["s2"][l][it])
            assert got.tobytes() == F32(want).tobytes(), ("%s level %d iteration %d" % (tag, l, it), got, want, m, n)
            assert (m == -1) == (n == 0) and -1 <= m < BINS, (tag, m, n)
            prev = (int(rlog["median_bin"][l][it]), int(rlog["count"][l][it]))
            n_it += 1
    return n_it


def replay_call(log, rlog, terms_at, levels, kind, param, tag="", depth=17):
    """robust_ref.replay_call with the s2 of every iteration taken from the robust log: n_valid equals the term count (and the log's
    count n), the logged residual is (float)sum_r2 / n of the weighted sums to the reduction bound, the logged update solves the
    weighted normal equations within TOL_BACKWARD, and the median bin is the one of the reference's own residuals (the device's r is
    the oracle's bit for bit).  Returns (terms, s2, level, it) of the finest level's last iteration and the number of iterations
    replayed."""
    term_replay.assert_indexed_like(rlog, log, levels, "robust", tag, has_levels=False)
    walk = term_replay.Replay(log, levels, tag=tag)
    last = None
    for st in walk:
        s2 = F32(rlog["s2"][st.l][st.it])
        t = terms_at(st.l, st.xi)
        assert st.n_valid == int(rlog["count"][st.l][st.it]), (st.where, "count", st.n_valid, int(rlog["count"][st.l][st.it]))
        st.check(rr.exact_sums(t, kind, param, s2), gn_sums.factor(gn_sums.at_level(depth, st.l)))
        # (an empty evaluation has no median: select() gives -1 there)
        m_ref = select(counts(t["r"]))[0]
        m_dev = int(rlog["median_bin"][st.l][st.it])
        assert m_dev == m_ref, (st.where, m_dev, m_ref)
        last = (t, s2, st.l, st.it)
    return last, walk.n_it


def edge_slack(r, ulp=4):
    """e_k for k = 1 .. 255: how many residuals of r lie within `ulp` float32 steps of bin edge k (the lower edge of bin k)"""
    u = np.abs(np.ascontiguousarray(r, F32)).view(np.uint32).astype(np.int64).ravel()
    e = np.zeros(BINS, np.int64)
    # (a residual is near at most one edge: the edges are 2^19 steps apart)
    near = np.clip(((u + (1 << 18)) >> 19) - K0, 1, BINS - 1)
    hit = np.abs(u - ((near + K0) << 19)) <= ulp
    np.add.at(e, near[hit], 1)
    return e
