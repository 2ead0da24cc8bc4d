"""Reference of step control (dvo_batch_set_step_control, include/dvo.h) on the oracle.

The contract's decisions are float32 and integer operations on the logged residual and n_valid, so the decision and lambda chains
are restated here with numpy float32 operations (each correctly rounded, as the device's) and have the device's bits.  The sums come
from the oracle (orc.optimize, or the exact sums of orc.optimize_terms), the solve is orc.solve6 on the damped system and the pose
composition orc.se3_concatenate.  lm_track and replay_call are an algorithm of their own (steps are accepted and rejected, a level ends
on the accepted pose) and stay whole here; only plain_track, the iteration without step control, runs in tests/term_replay.py's loop.
Nothing here is tuned on a device result.  Test infrastructure only."""
import numpy as np

import orc
import robust_ref as rr
import term_replay
from util import TOL_BACKWARD, assert_composed, backward_error

F32 = np.float32
FIRST, ACCEPT, REJECT = 1, 2, 3
DIAG = (0, 6, 11, 15, 18, 20)   # the diagonal of the 21 upper-triangle sums
DEFAULTS = dict(lambda0=1.0, lambda_up=4.0, lambda_down=0.5, lambda_floor=1e-4, lambda_max=1e6, min_valid_fraction=0.5)

RATIOS = []   # (tag, backward error / TOL_BACKWARD) of every update replay_call has checked


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    return {k: F32(v) for k, v in p.items()}


def decide(first, n_valid, residual, n_acc, res_acc, lam, P):
    """(decision, lambda after it): the contract's step 1 in float32"""
    lam = F32(lam)
    if first:
        return FIRST, lam
    with np.errstate(all="ignore"):
        ok = n_valid > 0 and F32(n_valid) >= F32(P["min_valid_fraction"] * F32(n_acc)) and F32(residual) <= F32(res_acc)
        if ok:
            return ACCEPT, F32(lam * P["lambda_down"])
        return REJECT, F32(min(F32(max(lam, P["lambda_floor"]) * P["lambda_up"]), P["lambda_max"]))


def damped(H21, lam):
    H = np.array(H21, np.float64)
    H[list(DIAG)] *= 1.0 + float(F32(lam))
    return H


def residual_of(sum_r2, n_valid):
    return F32(F32(sum_r2) / F32(n_valid)) if n_valid > 0 else F32(-1.0)


def stops(upd, res_acc, it, max_iterations, fixed_iterations, min_update, min_residual, trial):
    """step 3: True when the level ends with this iteration"""
    nrm = float(np.sqrt(np.sum(np.asarray(upd, F32).astype(np.float64) ** 2)))
    if not np.all(np.isfinite(trial)) or not np.isfinite(nrm):
        return True
    if fixed_iterations > 0:
        return not (it + 1 < fixed_iterations)
    return nrm < float(F32(min_update)) or F32(res_acc) < F32(min_residual) or it + 1 >= max_iterations


def oracle_sums(obj, ref, crop=False):
    """sums_at for two orc.OFrame: the oracle's own finished sums"""
    cache = {}

    def at(l, xi):
        key = (l, np.asarray(xi, F32).tobytes())
        if key not in cache:
            cache[key] = orc.optimize(obj.gray(l), ref.gray(l), ref.depth(l), ref.sigma(l), ref.K(l), xi, l, crop=crop)
        return cache[key]
    return at


def term_sums(obj, ref, crop=False):
    """sums_at from the exact float64 sums of orc.optimize_terms, as robust_ref.irls_track(kind NONE) forms them"""
    def at(l, xi):
        t = orc.optimize_terms(obj.gray(l), ref.gray(l), ref.depth(l), ref.sigma(l), ref.K(l), xi, l, crop=crop)
        ex = rr.exact_sums(t, rr.NONE, 1.0, rr.INF)
        return dict(H=ex["H"], g=ex["g"], sum_r2=ex["sum_r2"], n_valid=ex["n"])
    return at


def lm_track(sums_at, levels, P, max_iterations, min_update, min_residual=0.0, fixed_iterations=0, xi0=None):
    """The contract-exact replica of one tracking call with step control.  Returns (xi, log): per level the evaluation's residual and
    n_valid, xi_after, decision, lambda, and the accepted residual after every iteration; log["evaluations"] counts tile launches."""
    xi = np.zeros(6, F32) if xi0 is None else np.asarray(xi0, F32).copy()
    lam = F32(P["lambda0"])
    log = dict(n_iter=[], residual=[], n_valid=[], xi_after=[], xi_update=[], decision=[], lambda_=[], accepted=[], evaluations=0)
    acc = None
    for l in range(levels):
        rows = dict(residual=[], n_valid=[], xi_after=[], xi_update=[], decision=[], lambda_=[], accepted=[])
        n_its = fixed_iterations if fixed_iterations > 0 else max_iterations
        for it in range(n_its):
            s = sums_at(l, xi)
            log["evaluations"] += 1
            res = residual_of(s["sum_r2"], s["n_valid"])
            d, lam = decide(it == 0, s["n_valid"], res, acc["n_valid"] if acc else 0, acc["residual"] if acc else F32(-1), lam, P)
            if d != REJECT:
                acc = dict(xi=xi.copy(), H=np.array(s["H"], np.float64), g=np.array(s["g"], np.float64), n_valid=int(s["n_valid"]), residual=res)
            upd = orc.solve6(damped(acc["H"], lam), acc["g"]) if acc["n_valid"] > 0 else np.zeros(6, F32)
            with np.errstate(all="ignore"):
                trial = orc.se3_concatenate(acc["xi"], upd)
            stop = stops(upd, acc["residual"], it, max_iterations, fixed_iterations, min_update, min_residual, trial)
            xi = acc["xi"].copy() if stop else trial
            for k, v in (("residual", res), ("n_valid", s["n_valid"]), ("xi_after", xi.copy()), ("xi_update", upd), ("decision", d),
                         ("lambda_", lam), ("accepted", acc["residual"])):
                rows[k].append(v)
            if stop:
                break
        log["n_iter"].append(len(rows["residual"]))
        for k, v in rows.items():
            log[k].append(np.array(v, np.int32 if k in ("n_valid", "decision") else F32))
    return xi, log


def plain_track(sums_at, levels, max_iterations, min_update, min_residual=0.0):
    """the plain iteration on the same sums (tracker.cpp:42-73): every step taken.  Returns (xi, evaluations)."""
    def evaluate(l, xi):
        s = sums_at(l, xi)
        return term_replay.gn_step(s["n_valid"], s["H"], s["g"], s["sum_r2"]) + (dict(n_valid=s["n_valid"]),)
    xi, log = term_replay.track(levels, max_iterations, min_update, min_residual, evaluate)
    return xi, sum(log["n_iter"])


def replay_call(track_log, lm_log, sums_at, levels, P, max_iterations, min_update, min_residual=0.0, fixed_iterations=0, xi0=None, tag=""):
    """One whole tracking call of the device from its two logs.  The decision and lambda chains are recomputed bit for bit from the
    device's own logged residual and n_valid; every logged update must solve the damped normal equations of the oracle's sums at the
    accepted pose within TOL_BACKWARD; xi_after is the composed trial pose (assert_composed) for an iteration that stays active and
    the accepted pose bit for bit for the one that ends its level, which must be the level's last.
    Returns dict(accepted=[(level, it, xi)] the accepted evaluation each level ended on, rejects, early_stops, lam, residual)."""
    xi = np.zeros(6, F32) if xi0 is None else np.asarray(xi0, F32).copy()
    lam = F32(P["lambda0"])
    acc = None
    out = dict(accepted=[], rejects=0, accepts=0, early_stops=0, lam=lam, residual=None, iterations=0)
    for l in range(levels):
        n = int(track_log["n_iter"][l])
        assert n >= 1 and n == int(lm_log["n_iter"][l]), "%s: level %d ran %d iterations, the step-control log has %d" % (tag, l, n, int(lm_log["n_iter"][l]))
        acc_res = []
        for it in range(n):
            where = "%s level %d iteration %d" % (tag, l, it)
            res = F32(track_log["residual"][l][it]); nv = int(track_log["n_valid"][l][it])
            d, lam = decide(it == 0, nv, res, acc["n_valid"] if acc else 0, acc["residual"] if acc else F32(-1), lam, P)
            assert d == int(lm_log["decision"][l][it]), (where, "decision", d, int(lm_log["decision"][l][it]))
            assert F32(lm_log["lambda_"][l][it]).tobytes() == F32(lam).tobytes(), (where, "lambda", lm_log["lambda_"][l][it], lam)
            if d != REJECT:
                s = sums_at(l, xi)
                assert int(s["n_valid"]) == nv, (where, "n_valid", int(s["n_valid"]), nv)
                acc = dict(xi=xi.copy(), s=s, n_valid=nv, residual=res, level=l, it=it)
                out["accepts"] += d == ACCEPT
            else:
                out["rejects"] += 1
            acc_res.append(acc["residual"])
            upd = np.asarray(track_log["xi_update"][l][it], F32)
            if acc["n_valid"] > 0:
                back = backward_error(damped(acc["s"]["H"], lam), acc["s"]["g"], upd)
                RATIOS.append((where, back / TOL_BACKWARD))
                assert back <= TOL_BACKWARD, (where, "backward error %.3g" % back)
            else:
                assert not np.any(upd), where
            assert F32(track_log["upd_norm"][l][it]) == F32(np.sqrt(np.sum(upd.astype(np.float64) ** 2))), where
            with np.errstate(all="ignore"):
                trial = orc.se3_concatenate(acc["xi"], upd)
            stop = stops(upd, acc["residual"], it, max_iterations, fixed_iterations, min_update, min_residual, trial)
            after = np.asarray(track_log["xi_after"][l][it], F32)
            assert stop == (it == n - 1), (where, "stop test", stop, n)
            if stop:
                assert after.tobytes() == acc["xi"].tobytes(), (where, "a level ends on the accepted pose", after, acc["xi"])
                if it + 1 < (fixed_iterations if fixed_iterations > 0 else max_iterations):
                    out["early_stops"] += 1
            else:
                assert_composed(acc["xi"], upd, after, tag=where)
            xi = after.copy()
            out["iterations"] += 1
        assert all(a >= b for a, b in zip(acc_res, acc_res[1:])), "%s level %d: accepted residuals increase: %s" % (tag, l, acc_res)
        out["accepted"].append((acc["level"], acc["it"], acc["xi"].copy(), acc["s"]))
        assert xi.tobytes() == acc["xi"].tobytes()
    out["lam"] = lam
    out["residual"] = acc["residual"]
    out["xi"] = xi
    return out
