"""What the references of the opt-in tracking terms share (robust_ref, robust_median_ref, affine_ref, geometric_ref,
geometric_affine_ref; pyramid_filter_ref and lm_ref.plain_track for the loop): one walker over a device's track log and one plain
tracking loop on the oracle.

Replay (the walker) owns what every replay_call checks of a logged iteration, whatever the term: a level ran at least one iteration,
n_valid is the term count, the logged residual is (float)sum_r2 / n inside the reduction bound, the logged update solves the replayed
normal equations within TOL_BACKWARD, an empty evaluation has residual -1 and a zero update, and xi_after is the composition of input
pose and update -- or the input pose bit for bit where the composition is not finite (testXi, tracker.cpp:47-51).  The term's module
keeps the middle: where the exact sums of an iteration come from, and the checks of its own side log.

track() owns what every replica of a plain tracking call repeats (tracker.cpp:42-73): the pose is composed where the composition is
finite, the level stops on the update norm or the residual, and the log is assembled per level.  The per-iteration function is the
term's; the order of its float32 and float64 operations is what makes a replica a bit-exact anchor, so it stays in the term's module.
Test infrastructure only."""
import numpy as np

import orc
from util import TOL_BACKWARD, assert_composed, backward_error

F32 = np.float32


def assert_indexed_like(side, log, levels, name, tag="", has_levels=True):
    """a side log (affine, geometric, robust) has `levels` and n_iter equal to the track log's: its rows are those iterations"""
    iters = [int(n) for n in log["n_iter"][:levels]]
    assert (not has_levels or int(side["levels"]) == levels) and [int(n) for n in side["n_iter"][:levels]] == iters, \
        (tag, "the %s log is indexed like the track log" % name, side["n_iter"], iters)


class Replay:
    """One tracking call of the device, walked from its track log: `for st in Replay(log, levels, xi0, tag)` yields the walker itself
    once per logged iteration with l, it, where, the input pose xi, and the logged n_valid, res and upd.  The caller does the term's own
    checks and then calls st.check(ex, depth_u) once; the walker then advances xi to the logged xi_after and counts n_it."""

    def __init__(self, log, levels, xi0=None, tag=""):
        self.log, self.levels, self.tag = log, levels, tag
        self.xi = np.zeros(6, F32) if xi0 is None else np.asarray(xi0, F32).copy()
        self.n_it = 0

    def __iter__(self):
        log = self.log
        for l in range(self.levels):
            n = int(log["n_iter"][l])
            assert n >= 1, "%s: level %d ran no iteration" % (self.tag, l)
            for it in range(n):
                self.l, self.it, self.where = l, it, "%s level %d iteration %d" % (self.tag, l, it)
                self.n_valid = int(log["n_valid"][l][it])
                self.res = F32(log["residual"][l][it])
                self.upd = log["xi_update"][l][it]
                self._after = None
                yield self
                assert self._after is not None, (self.where, "the iteration was not checked")
                self.xi = self._after.copy()
                self.n_it += 1

    def check(self, ex, depth_u):
        """The logged iteration against its exact sums ex (n, H, g, sum_r2, A_r).  depth_u = depth * 2^-24 * (1 + 2^-10) of the
        reduction that made sum_r2: it places the logged residual (the sums themselves go through gn_sums.assert_entries)."""
        where, xi, res, upd = self.where, self.xi, self.res, self.upd
        assert ex["n"] == self.n_valid, (where, "n_valid", ex["n"], self.n_valid)
        if ex["n"] > 0:
            assert abs(float(res) - ex["sum_r2"] / ex["n"]) <= (depth_u * ex["A_r"] + 2 * float(np.spacing(F32(ex["sum_r2"])))) / ex["n"] \
                + float(np.spacing(res)), (where, float(res), ex["sum_r2"] / ex["n"])
            back = backward_error(ex["H"], ex["g"], upd)
            assert back <= TOL_BACKWARD, (where, "backward error %.3g" % back)
        else:
            assert res == F32(-1.0) and not np.any(upd), where
        after = np.asarray(self.log["xi_after"][self.l][self.it], F32)
        if np.all(np.isfinite(orc.se3_concatenate(xi, upd))):
            assert_composed(xi, upd, after, tag=where)
        else:                                # testXi (tracker.cpp:47-51): the pose is left unchanged
            assert after.tobytes() == xi.tobytes(), where
        self._after = after


def seq_sum(p):
    """the sum of a float64 vector in index order (np.cumsum accumulates sequentially): the oracle's own double loop"""
    return float(np.cumsum(p)[-1]) if p.size else 0.0


def raster_sums(J, Jr, rw):
    """(H [21], g [6]) of float64 J [n][6], the weighted Jr (J itself without weights) and rw [n]: every product summed in double in
    raster order, as the oracle sums them"""
    return (np.array([seq_sum(Jr[:, p] * J[:, q]) for p in range(6) for q in range(p, 6)]),
            np.array([seq_sum(Jr[:, p] * rw) for p in range(6)]))


def gn_step(n, H, g, sum_r2):
    """(update, residual) of one evaluation from the sums of its n terms: orc.solve6 and (float)sum_r2 / n, or a zero update and
    residual -1 without terms (optimize.cpp:92-93)"""
    if n <= 0:
        return np.zeros(6, F32), F32(-1.0)
    return orc.solve6(H, g), F32(F32(sum_r2) / F32(n))


def track(levels, max_iterations, min_update, min_residual, evaluate, xi0=None):
    """One plain tracking call (tracker.cpp:42-73).  evaluate(l, xi) -> (update, residual, extras) is one iteration at level l and
    input pose xi; extras holds n_valid and whatever else the replica logs per iteration.  The pose is composed where the composition
    is finite; a level ends when |update| < (float)min_update or residual < (float)min_residual.  Returns (xi, log): n_iter per level
    and, per level and iteration, residual, xi_after, xi_update and every key of extras (scalars as one array per level, anything else
    as a list)."""
    xi = np.zeros(6, F32) if xi0 is None else np.asarray(xi0, F32).copy()
    log = dict(n_iter=[])
    for l in range(levels):
        rows = {}
        for it in range(max_iterations):
            upd, res, extras = evaluate(l, xi)
            nxt = orc.se3_concatenate(xi, upd)
            if np.all(np.isfinite(nxt)):
                xi = nxt
            for k, v in dict(extras, residual=F32(res), xi_after=xi.copy(), xi_update=np.array(upd, F32)).items():
                rows.setdefault(k, []).append(v)
            nrm = float(np.sqrt(np.sum(upd.astype(np.float64) ** 2)))
            if nrm < float(F32(min_update)) or res < F32(min_residual):
                break
        log["n_iter"].append(len(rows["residual"]))
        for k, v in rows.items():
            log.setdefault(k, []).append(np.array(v) if np.ndim(v[0]) == 0 or k in ("xi_after", "xi_update") else v)
    return xi, log
