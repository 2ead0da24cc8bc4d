"""The five replay_call functions of the opt-in tracking terms (robust_ref, robust_median_ref, affine_ref, geometric_ref,
geometric_affine_ref) still reject what they rejected, now that they share tests/term_replay.py's walker.

No device: the logs of one tracking call are built from the term's own numpy replica on the oracle (its track log carries xi_update
and n_valid; the side logs are laid out like the binding's), replay_call must accept them, and every single mutation of them -- a
count, a residual, an update, a pose, an iteration count, an entry of a side log -- must raise."""
import copy
import functools

import numpy as np
import pytest

import affine_ref as ar
import geometric_affine_ref as ga
import geometric_ref as gr
import orc
import robust_median_ref as mr
import robust_ref as rr
from dvo_amd import synth

F32 = np.float32
LEVELS, CULLS = 3, 1
ITS, MIN_UPDATE = 4, 2e-5          # four iterations on every level: no stop test fires at this update norm
FLOOR2 = 1e-6
PARAM = {rr.NONE: 1.0, rr.HUBER: 1.345, rr.STUDENT_T: 5.0}
WEIGHT, MAX_DIFF = 10.0, 0.1


@functools.lru_cache(maxsize=None)
def frames():
    K = synth.K_640.copy()
    K[:2] *= 0.25
    g, d, s, _ = synth.sequence(2, 160, 120, K, 42, sigma_value=0.5)
    g, d, s = g.numpy(), d.numpy(), s.numpy()
    return orc.OFrame(g[1], d[1], s[1], K, LEVELS, CULLS), orc.OFrame(g[0], d[0], s[0], K, LEVELS, CULLS)


def _side(log, **rows):
    return dict(levels=LEVELS, n_iter=np.array(log["n_iter"]), **rows)


def _affine_log(log, mode):
    prime = log["prime"] if mode == ar.ESTIMATE else (F32(0), F32(0))
    return _side(log, a=[np.array([e[0] for e in lv], F32) for lv in log["ab"]], b=[np.array([e[1] for e in lv], F32) for lv in log["ab"]],
                 prime_a=F32(prime[0]), prime_b=F32(prime[1]))


def _geometric_log(log, exact_at):
    """n_geo of the replica and sum_sq = (float)S29 of the exact sums at every iteration's input pose"""
    xi = np.zeros(6, F32)
    sum_sq = []
    for l in range(LEVELS):
        sum_sq.append(np.zeros(log["n_iter"][l], F32))
        for it in range(log["n_iter"][l]):
            sum_sq[l][it] = F32(exact_at(l, xi, it)["S29"])
            xi = log["xi_after"][l][it]
    return _side(log, n_geo=[np.array(n) for n in log["n_geo"]], sum_sq=sum_sq)


# ---- one call per term: (logs, replay) with replay(logs) -> the number of iterations replayed ---------------------------------------
def _robust(kind):
    obj, ref = frames()
    _, log = rr.irls_track(obj, ref, LEVELS, kind, PARAM[kind], FLOOR2, False, ITS, MIN_UPDATE)
    return dict(track=log), lambda L: rr.replay_call(L["track"], rr.oracle_terms(obj, ref, False), LEVELS, kind, PARAM[kind], rr.ADAPTIVE,
                                                     floor2=FLOOR2, tag="robust", depth=17)[1]


def _median():
    obj, ref = frames()
    _, log = mr.median_track(obj, ref, LEVELS, mr.HUBER, 1.345, FLOOR2, False, ITS, MIN_UPDATE)
    rlog = dict(n_iter=np.array(log["n_iter"]), s2=log["s2"], median_bin=[np.array(m) for m in log["median_bin"]],
                count=[np.array(n) for n in log["count"]], prime_bin=log["prime"][0], prime_count=log["prime"][1])
    return dict(track=log, robust=rlog), lambda L: mr.replay_call(L["track"], L["robust"], rr.oracle_terms(obj, ref, False), LEVELS, mr.HUBER,
                                                                  1.345, tag="median", depth=17)[1]


def _affine(mode):
    obj, ref = frames()
    wp = ar.weight_params()
    _, log = ar.affine_track(obj, ref, LEVELS, mode, False, ITS, MIN_UPDATE, wp=wp, given_ab=(1.15, -0.03))
    return dict(track=log, affine=_affine_log(log, mode)), lambda L: ar.replay_call(
        L["track"], L["affine"], ar.oracle_pixels(obj, ref, False, wp), LEVELS, mode, given_ab=(1.15, -0.03), depth=17, tag="affine")[1]


def _geometric():
    obj, ref = frames()
    at = gr.frame_pixels(obj, ref, False, gr.weight_params())
    _, log = gr.geometric_track(obj, ref, LEVELS, WEIGHT, MAX_DIFF, False, ITS, MIN_UPDATE)
    glog = _geometric_log(log, lambda l, xi, it: gr.exact(at(l, xi), WEIGHT, MAX_DIFF))
    return dict(track=log, geometric=glog), lambda L: gr.replay_call(L["track"], L["geometric"], at, LEVELS, WEIGHT, MAX_DIFF, ppt=4, tag="geometric")[1]


def _geometric_affine(mode):
    obj, ref = frames()
    at = ga.frame_pixels(obj, ref, False, gr.weight_params())
    _, log = ga.geometric_affine_track(obj, ref, LEVELS, WEIGHT, MAX_DIFF, mode, False, ITS, MIN_UPDATE, given_ab=(1.15, -0.03))
    glog = _geometric_log(log, lambda l, xi, it: ga.exact(at(l, xi), WEIGHT, MAX_DIFF, *log["ab"][l][it]))
    return dict(track=log, geometric=glog, affine=_affine_log(log, mode)), lambda L: ga.replay_call(
        L["track"], L["geometric"], L["affine"], at, LEVELS, WEIGHT, MAX_DIFF, mode, given_ab=(1.15, -0.03), ppt=4, tag="geometric-affine")[1]


CALLS = {"robust-none": lambda: _robust(rr.NONE), "robust-huber": lambda: _robust(rr.HUBER), "robust-student_t": lambda: _robust(rr.STUDENT_T),
         "median": _median, "affine-estimate": lambda: _affine(ar.ESTIMATE), "affine-given": lambda: _affine(ar.GIVEN),
         "geometric": _geometric, "geometric_affine-estimate": lambda: _geometric_affine(ga.ESTIMATE),
         "geometric_affine-given": lambda: _geometric_affine(ga.GIVEN)}


@functools.lru_cache(maxsize=None)
def call(name):
    """(logs, replay) of one term, built once; replay_call accepts the logs as they are"""
    logs, replay = CALLS[name]()
    assert replay(logs) == LEVELS * ITS
    return logs, replay


# ---- the mutations: name -> (the log it changes, what it does to that log) ----------------------------------------------------------
def _set(key, l, it, change):
    def mutate(log):
        log[key][l] = np.array(log[key][l])
        log[key][l][it] = change(log[key][l][it])
    return mutate


def _component(key, l, it, c, delta):
    def mutate(log):
        log[key][l] = np.array(log[key][l], F32)
        log[key][l][it][c] += F32(delta)
    return mutate


def _n_iter(l, n):
    def mutate(log):
        log["n_iter"] = [int(v) for v in log["n_iter"]]
        log["n_iter"][l] = n
    return mutate


def _ulp(v):
    return np.nextafter(F32(v), F32(np.inf))


TRACK = {"n_valid + 1": ("track", _set("n_valid", 1, 2, lambda v: v + 1)),
         "residual * (1 + 1e-4)": ("track", _set("residual", 1, 1, lambda v: F32(v * F32(1.0001)))),
         "xi_update + 1e-4": ("track", _component("xi_update", 2, 0, 4, 1e-4)),
         "xi_after + 1e-5": ("track", _component("xi_after", 0, 3, 1, 1e-5)),
         "n_iter[0] = 0": ("track", _n_iter(0, 0))}
GEOMETRIC = {"n_geo + 1": ("geometric", _set("n_geo", 1, 0, lambda v: v + 1)),
             "sum_sq * (1 + 1e-4)": ("geometric", _set("sum_sq", 2, 1, lambda v: F32(v * F32(1.0001)))),
             "geometric n_iter": ("geometric", _n_iter(1, ITS - 1))}
AFFINE = {"first a + 1 ulp": ("affine", _set("a", 0, 0, _ulp)), "first b + 1 ulp": ("affine", _set("b", 0, 0, _ulp)),
          "affine n_iter": ("affine", _n_iter(2, ITS - 1))}
ESTIMATE = {"later a + 1e-3": ("affine", _set("a", 1, 1, lambda v: F32(v + F32(1e-3))))}
MEDIAN = {"median_bin + 1": ("robust", _set("median_bin", 1, 1, lambda v: v + 1)), "count + 1": ("robust", _set("count", 0, 2, lambda v: v + 1)),
          "robust n_iter": ("robust", _n_iter(1, ITS - 1))}
MUTATIONS = {name: {**TRACK, **(MEDIAN if name == "median" else {}), **(GEOMETRIC if name.startswith("geometric") else {}),
                    **(AFFINE if "affine" in name else {}), **(ESTIMATE if name.endswith("estimate") else {})} for name in CALLS}


@pytest.mark.parametrize("name", list(CALLS))
def test_replay_accepts_the_replica_logs(name):
    logs, _ = call(name)
    assert all(len(logs["track"][k]) == LEVELS for k in ("xi_update", "n_valid", "residual", "xi_after"))
    if "affine" in logs and name.endswith("estimate"):    # the estimate moved: the entry chain is not a row of constants
        assert len({float(a) for lv in logs["affine"]["a"] for a in lv}) > LEVELS
    if "geometric" in logs:
        assert min(int(n.min()) for n in logs["geometric"]["n_geo"]) > 100


@pytest.mark.parametrize("name,mutation", [(n, m) for n in CALLS for m in MUTATIONS[n]])
def test_replay_rejects(name, mutation):
    logs, replay = call(name)
    which, mutate = MUTATIONS[name][mutation]
    bad = dict(logs)
    bad[which] = copy.deepcopy(logs[which])
    mutate(bad[which])
    with pytest.raises(AssertionError):
        replay(bad)
