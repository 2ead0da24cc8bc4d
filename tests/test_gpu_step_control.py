"""Step control of a batch (dvo_batch_set_step_control, include/dvo.h) on the GPU, both batch kinds.

The serial tail's decision rules are reached exactly through dvo_op_lm_step on hand-made sums; whole pushes are replayed by
tests/lm_ref.py: the decision and lambda chains bit for bit from the device's own logged residual and n_valid, every logged update
against the damped normal equations of the oracle's sums at the accepted pose, every level ending on its accepted pose; the schedules,
the feeds and the tile shapes give the same records; the quality record holds the accepted evaluation's sums; and on the reference's own
sensor-depth constants, where the plain iteration diverges, step control wins.

Everything runs on 320x240 frames (one case at the ragged 328x248), 3 levels, culls 1, crop off.  Two workloads: "ref", the reference's
step constants on sigma 0.1 (over-relaxed: rejects and early stops occur), and "conv", the converging literals of bench.py on sigma 0.5."""
import functools

import numpy as np
import pytest

import dvo_amd as dvo
import gn_sums
import lm_ref as lr
import lockstep
import orc
import term_batch as tb
from dvo_amd import synth
from term_batch import CULLS, F32, KH, LEVELS, MIN_UPDATE, SIZE, SKIP, RESTART, STEPS, TOP, TRACK, TRACKED
from util import K640, TOL_BACKWARD, assert_composed, backward_error

pytestmark = pytest.mark.gpu

FIRST, ACCEPT, REJECT = dvo.LM_FIRST, dvo.LM_ACCEPT, dvo.LM_REJECT
WORK = dict(ref=dict(sigma=0.1, steps=None, its=8), conv=dict(sigma=0.5, steps=STEPS, its=6))


def _oracle(work):
    orc.set_tracker_params(step3=WORK[work]["steps"], min_residual=0.0, min_update=MIN_UPDATE)


@pytest.fixture(autouse=True)
def _oracle_back():
    yield
    orc.set_tracker_params()


def _cfg(work="ref", **kw):
    """(not term_batch.cfg: the "ref" workload keeps the reference's step constants, and max_iterations follows the workload)"""
    kw.setdefault("max_iterations", WORK[work]["its"])
    kw.setdefault("gn_pixels_per_thread", 4)
    if WORK[work]["steps"]:
        kw.update(step_default=STEPS[0], step_level1=STEPS[1], step_level2=STEPS[2])
    return dvo.default_config(crop_enable=0, min_residual=0.0, min_update=MIN_UPDATE, **kw)


def _wide_idx(B, pushes=3):
    """(without term_batch's table for up to five sequences)"""
    return tb.wide_idx(B, pushes, table=False)


def _term(idx, work="ref", lm=None, clear=False, size=SIZE, guess=None):
    """run() keywords of a batch on the frames of a workload.  lm: set_step_control arguments ({} = the defaults; None: never set;
    clear: set, then turned off before the first push); guess[k]: the given start poses of push k, read back as `start`"""
    def setup(bt, keep):
        bt.set_step_control(**lm)
        if clear:
            bt.set_step_control(dvo.LM_OFF)
    reads = (("start",) if guess is not None else ()) + (("step",) if lm is not None and not clear else ())
    return dict(setup=setup if lm is not None else None, reads=reads, maps=tb.frame_maps(idx, size, WORK[work]["sigma"]), size=size, guess=guess)


def _empty(o, b):
    """the zero record and the empty log of a sequence that did not track"""
    r = o["rec"][b]
    assert (r["n_first"], r["n_accepted"], r["n_rejected"], r["lambda"], r["residual"]) == (0, 0, 0, 0.0, 0.0), (b, r)
    lg = o["lmlogs"][b]
    assert not lg["n_iter"].any() and not lg["lambda_"].any() and not lg["decision"].any() and lg["levels"] == LEVELS
    return True


# ------------------------------------------------------------------------------------------------------------------ 1: the serial tail
def _spd(seed, scale=1.0):
    rng = np.random.default_rng(seed)
    A = rng.normal(size=(40, 6)) * np.array([1, 1, 1, 3, 3, 3.0])
    H = (A.T @ A) * scale
    return np.array([H[i, j] for i in range(6) for j in range(i, 6)]), (A.T @ rng.normal(size=40) * 1e-3) * scale


def _state_of(xi):
    """(Tc, pose) the device derives from a twist: exp(xi) in double and float(exp(-xi)) (dvo_op_pose_algebra, op 0)"""
    xi = np.asarray(xi, F32)
    return dvo.pose_algebra(0, xi.astype(np.float64)[None])[0], dvo.pose_algebra(0, -xi.astype(np.float64)[None])[0].astype(F32)


def _entry(xi, H, g, n_valid, residual, lam, sum_r2=None):
    e = np.zeros((), dvo.LM_ENTRY_DTYPE)
    e["xi"] = np.asarray(xi, F32)
    e["Tc"], e["pose"] = _state_of(xi)
    e["H"], e["g"], e["n_valid"], e["residual"], e["lambda"] = H, g, n_valid, F32(residual), F32(lam)
    e["sum_r2"] = float(residual) * n_valid if sum_r2 is None else sum_r2
    return e


def _sums(H, g, sum_r2, n_valid):
    return np.concatenate([H, g, [sum_r2, float(n_valid)]])


XA = F32([0.01, -0.02, 0.005, 0.003, -0.004, 0.002])     # the accepted twist of the hand-made entries
XE = F32([0.012, -0.018, 0.004, 0.0035, -0.0038, 0.0021])  # the twist the sums were evaluated at
RES = F32(F32(2.0) / F32(1000))


def _cases():
    """name -> dict(sums, entry, first, it_prev, lm, stop constants, want): the contract's rules, each reached exactly"""
    Ha, ga = _spd(1)
    He, ge = _spd(2)
    base = lambda res=RES, n=1000, lam=1.0: _entry(XA, Ha, ga, n, res, lam)
    ev = lambda sum_r2=2.0, n=1000: _sums(He, ge, sum_r2, n)
    tiny = ga * 1e-9
    c = {}
    c["first"] = dict(sums=ev(5.0), entry=base(), first=True, want=(FIRST, True))                       # accepted although worse
    c["tie_accepts"] = dict(sums=ev(), entry=base(), it_prev=3, want=(ACCEPT, True))
    c["larger_residual_rejects"] = dict(sums=ev(), entry=base(np.nextafter(RES, F32(0))), it_prev=3, want=(REJECT, True))
    c["below_the_fraction_rejects"] = dict(sums=ev(0.5, 499), entry=base(), it_prev=3, want=(REJECT, True))
    c["at_the_fraction_accepts"] = dict(sums=ev(0.5, 500), entry=base(), it_prev=3, want=(ACCEPT, True))
    c["no_pixels_rejects"] = dict(sums=np.zeros(29), entry=base(), it_prev=3, want=(REJECT, True))
    c["nan_residual_rejects"] = dict(sums=ev(np.nan), entry=base(), it_prev=3, want=(REJECT, True))
    c["lambda_at_the_floor"] = dict(sums=ev(9.0), entry=base(lam=0.0), it_prev=3, want=(REJECT, True), lam=F32(1e-4) * F32(4))
    # (with lambda = 1e6 the step is a millionth of the Gauss-Newton one: below min_update, the level ends)
    c["lambda_at_the_maximum"] = dict(sums=ev(9.0), entry=base(lam=5e5), it_prev=3, want=(REJECT, False), lam=F32(1e6))
    c["nothing_accepted"] = dict(sums=np.zeros(29), entry=_entry(XA, Ha * 0, ga * 0, 0, -1.0, 1.0, sum_r2=0.0), it_prev=3, want=(REJECT, False))
    c["first_without_pixels"] = dict(sums=np.zeros(29), entry=base(), first=True, want=(FIRST, False))   # n_acc = 0: a zero update, the level ends
    bad = ga.copy(); bad[0] = np.inf
    c["non_finite_update"] = dict(sums=ev(9.0), entry=_entry(XA, Ha, bad, 1000, RES, 1.0), it_prev=1, fixed_iterations=8, want=(REJECT, False))
    c["stops_on_the_update"] = dict(sums=_sums(He, tiny, 2.0, 1000), entry=base(), it_prev=3, want=(ACCEPT, False))
    c["stops_on_the_residual"] = dict(sums=ev(), entry=base(), it_prev=3, min_residual=1e-2, want=(ACCEPT, False))
    # (the residual stop reads the ACCEPTED residual: a rejected evaluation below min_residual does not end the level)
    c["rejected_is_no_residual_stop"] = dict(sums=ev(1e-4, 100), entry=base(), it_prev=3, min_residual=1e-4, want=(REJECT, True))
    c["stops_on_the_count"] = dict(sums=ev(), entry=base(), it_prev=14, want=(ACCEPT, False))
    c["one_before_the_count"] = dict(sums=ev(), entry=base(), it_prev=13, want=(ACCEPT, True))
    c["fixed_goes_on"] = dict(sums=_sums(He, tiny, 2.0, 1000), entry=base(), it_prev=2, fixed_iterations=4, want=(ACCEPT, True))
    c["fixed_ends"] = dict(sums=ev(), entry=base(), it_prev=3, fixed_iterations=4, want=(ACCEPT, False))
    c["fixed_first_of_one"] = dict(sums=ev(), entry=base(), first=True, it_prev=7, fixed_iterations=1, want=(FIRST, False))
    return c


def _check_case(name, c, got, i):
    P = lr.params(**c.get("lm", {}))
    first, it_prev = c.get("first", False), c.get("it_prev", 0)
    s, e = c["sums"], c["entry"]
    nv = int(s[28])
    res = lr.residual_of(s[27], nv)
    d, lam = lr.decide(first, nv, res, int(e["n_valid"]), e["residual"], e["lambda"], P)
    assert (d, bool(got["active"][i])) == c["want"] and d == got["decision"][i], (name, d, got["decision"][i], got["active"][i])
    if "lam" in c:
        assert F32(lam).tobytes() == F32(c["lam"]).tobytes(), name
    want = e.copy()
    if d != REJECT:
        want["xi"] = XE
        want["Tc"], want["pose"] = _state_of(XE)
        want["H"], want["g"], want["sum_r2"], want["n_valid"], want["residual"] = s[:21], s[21:27], s[27], nv, res
    want["lambda"] = lam
    out = got["entry"][i]
    for f in dvo.LM_ENTRY_DTYPE.names:
        if f != "reserved":
            assert np.asarray(out[f]).tobytes() == np.asarray(want[f]).tobytes(), (name, f, out[f], want[f])
    upd = got["update"][i]
    if int(want["n_valid"]) > 0 and np.isfinite(want["g"]).all():
        back = backward_error(lr.damped(want["H"], lam), want["g"], upd)
        lr.RATIOS.append(("op_lm_step " + name, back / TOL_BACKWARD))
        assert back <= TOL_BACKWARD, (name, back)
    elif int(want["n_valid"]) == 0:
        assert not upd.any(), name
    else:
        assert not np.isfinite(upd).all(), name
    with np.errstate(all="ignore"):
        trial = orc.se3_concatenate(want["xi"], upd)
    it = 0 if first else it_prev
    stop = lr.stops(upd, want["residual"], it, 15, c.get("fixed_iterations", 0), MIN_UPDATE, c.get("min_residual", 0.0), trial)
    assert stop == (not c["want"][1]), name
    if stop:
        assert got["xi_next"][i].tobytes() == np.asarray(want["xi"], F32).tobytes(), (name, "a level ends on the accepted pose")
    else:
        assert_composed(want["xi"], upd, got["xi_next"][i], tag=name)


def _op(cases, names):
    c0 = cases[names[0]]
    key = lambda c: (c.get("first", False), c.get("it_prev", 0), c.get("fixed_iterations", 0), c.get("min_residual", 0.0))
    assert all(key(cases[n]) == key(c0) for n in names)
    cfg = dvo.default_config(max_iterations=15, fixed_iterations=c0.get("fixed_iterations", 0), min_update=MIN_UPDATE,
                             min_residual=c0.get("min_residual", 0.0))
    return dvo.op_lm_step(np.stack([cases[n]["sums"] for n in names]), np.stack([XE] * len(names)), np.stack([cases[n]["entry"] for n in names]),
                          level_first=c0.get("first", False), it_prev=c0.get("it_prev", 0), cfg=cfg)


def test_serial_tail_on_hand_made_sums():
    """every rule alone (a batch of 1), then the cases that share their call constants side by side in batches of 8 and 9
    (DVO_SOLVE_SEQ is 8): the same bits in every slot"""
    cases = _cases()
    before = len(lr.RATIOS)
    for name in cases:
        _check_case(name, cases[name], _op(cases, [name]), 0)
    shared = [n for n in cases if not cases[n].get("first") and cases[n].get("it_prev") == 3 and not cases[n].get("fixed_iterations")
              and not cases[n].get("min_residual")]
    assert len(shared) >= 8
    for n in (8, 9):
        names = [shared[(i * 3) % len(shared)] for i in range(n)]
        got = _op(cases, names)
        for i, name in enumerate(names):
            _check_case(name, cases[name], got, i)
    assert len(lr.RATIOS) >= before + len(cases) - 4


# ------------------------------------------------------------------------------------------------------------------ 2: whole pushes
def _replay(outs, cfg, B, work, lm=None, cams=None, size=SIZE, kf=False, guess=None, seqs=None, min_tracked=None, idx=None):
    """every TRACKED sequence of every push through lr.replay_call; the others have zero records and empty logs.  Returns the totals."""
    _oracle(work)
    idx = _wide_idx(B, len(outs)) if idx is None else idx
    P = lr.params(**(lm or {}))
    depth = gn_sums.depth_for_cfg(cfg)
    tot = dict(n=0, rejects=0, early_stops=0, iterations=0, accepts=0)

    def check(k, b, kr, o, K):
        where = "push %d seq %d of %d" % (k, b, B)
        sigma = WORK[work]["sigma"]
        obj, ref = tb.oframe(idx[k][b], K, size, sigma), tb.oframe(idx[kr][b], K, size, sigma)
        lg, ll, rec = o["logs"][b], o["lmlogs"][b], o["rec"][b]
        r = lr.replay_call(lg, ll, lr.oracle_sums(obj, ref), LEVELS, P, cfg.max_iterations, cfg.min_update, cfg.min_residual,
                           cfg.fixed_iterations, xi0=o.get("start", [None] * B)[b], tag=where)
        # the returned pose is the last accepted one; the record counts the decisions and keeps lambda and the accepted residual
        assert o["xi"][b].tobytes() == r["xi"].tobytes(), where
        assert (rec["n_first"], rec["n_accepted"], rec["n_rejected"]) == (LEVELS, r["accepts"], r["rejects"]), (where, rec)
        assert F32(rec["lambda"]).tobytes() == F32(r["lam"]).tobytes() and F32(rec["residual"]).tobytes() == F32(r["residual"]).tobytes(), where
        if o["q"] is not None:   # the quality record: the accepted evaluation's sums of the finest level
            l, it, xa, _ = r["accepted"][TOP]
            q = o["q"][b]
            assert l == TOP and q["status"] == TRACKED and q["n_valid"] == int(lg["n_valid"][TOP][it]), where
            assert F32(q["residual"]).tobytes() == F32(lg["residual"][TOP][it]).tobytes(), where
            t = orc.optimize_terms(obj.gray(TOP), ref.gray(TOP), ref.depth(TOP), ref.sigma(TOP), ref.K(TOP), xa, TOP, crop=False)
            gn_sums.assert_gn_sums(q, t, gn_sums.at_level(depth, TOP), "step control " + where)
        for f in ("rejects", "early_stops", "iterations", "accepts"):
            tot[f] += r[f]
        return r["iterations"]
    tot["n"], _ = tb.walk(outs, B, check, _empty, kf=kf, cams=cams, seqs=seqs, min_tracked=min_tracked)
    return tot


@functools.lru_cache(maxsize=None)
def _base(work, B):
    return tb.run(_cfg(work), B, _wide_idx(B), **_term(_wide_idx(B), work, lm={}))


@pytest.mark.parametrize("B", [5, 17])
@pytest.mark.parametrize("work", ["ref", "conv"])
def test_whole_pushes_replay(work, B):
    """B = 17: k_gn_solve_lm takes 8 sequences per workgroup, so the third workgroup holds one"""
    before = gn_sums.nonempty_calls()
    tot = _replay(_base(work, B), _cfg(work), B, work)
    assert gn_sums.nonempty_calls() >= before + tot["n"]
    if work == "ref":   # rejects and active-list compaction really occur
        assert tot["rejects"] >= 1 and tot["early_stops"] >= 1, tot
    else:
        assert tot["accepts"] > 3 * tot["n"], tot


def test_whole_pushes_replay_ragged_size():
    outs = tb.run(_cfg("ref"), 3, _wide_idx(3), **_term(_wide_idx(3), "ref", lm={}, size=(328, 248)))
    _replay(outs, _cfg("ref"), 3, "ref", size=(328, 248))


@pytest.mark.parametrize("work", ["ref", "conv"])
def test_feeds_are_bit_identical(work):
    idx = _wide_idx(5)
    tb.same(_base(work, 5), tb.run(_cfg(work), 5, idx, feed="host", **_term(idx, work, lm={})))
    a = tb.run(_cfg(work), 5, idx, feed="raw", **_term(idx, work, lm={}))
    tb.same(a, tb.run(_cfg(work), 5, idx, feed="raw_host", **_term(idx, work, lm={})))
    assert all((o["rec"]["n_first"] == LEVELS).all() for o in a[1:])


# ------------------------------------------------------------------------------------------------------------------ 3: configurations
@pytest.fixture(scope="module")
def base19():
    return tb.run(_cfg("ref"), 19, _wide_idx(19), **_term(_wide_idx(19), "ref", lm={}))


@pytest.mark.parametrize("variant", ["adaptive_off", "fused_tiles", "single_launch", "two_streams"])
def test_configurations_give_the_same_records(variant, base19):
    """19 sequences: two sub-batches need more than 16, and 19 is no multiple of 8; the tables are offset per sub-batch"""
    kw = tb.SCHEDULE_VARIANTS[variant]
    other = tb.run(_cfg("ref", **kw), 19, _wide_idx(19), **_term(_wide_idx(19), "ref", lm={}))
    assert all(p["schedule"] == dvo.PLAN_PAIRS for p in other[0]["plan"])
    tb.same(base19, other)
    assert sum(int(o["rec"]["n_rejected"].sum()) for o in base19[1:]) >= 1


def test_nineteen_sequences_replay(base19):
    _replay(base19, _cfg("ref"), 19, "ref", seqs=(0, 7, 8, 15, 16, 18))


# ------------------------------------------------------------------------------------------------------------------ 4: tile shapes
SHAPES = [(1, 1), (2, 1), (2, 2), (4, 1), (4, 2), (4, 4), (8, 1), (8, 2), (8, 4)]


@pytest.mark.parametrize("ppt,group", SHAPES)
def test_every_tile_shape(ppt, group):
    """each (PPT, G) pair of the plain k_track_gn under step control on a batch of two, held to the contract at its own poses"""
    cfg = _cfg("ref", gn_gather_group=group, gn_pixels_per_thread=ppt)
    outs = tb.run(cfg, 2, _wide_idx(2), **_term(_wide_idx(2), "ref", lm={}))
    assert all((p["ppt"], p["group"], p["schedule"]) == (ppt, group, dvo.PLAN_PAIRS) for p in outs[0]["plan"]), outs[0]["plan"]
    _replay(outs, cfg, 2, "ref")


def test_equal_cameras_are_the_plain_path():
    """the _cam kernels with a table of equal K's: bit for bit the batch without a table"""
    cams = np.stack([KH] * 5).astype(np.float32)
    tb.same(_base("ref", 5), tb.run(_cfg("ref"), 5, _wide_idx(5), cams=cams, **_term(_wide_idx(5), "ref", lm={})))


# ------------------------------------------------------------------------------------------------------------------ 5: batch features
def test_per_sequence_intrinsics():
    cams = tb.sequence_cams(5)
    outs = tb.run(_cfg("ref"), 5, _wide_idx(5), cams=cams, **_term(_wide_idx(5), "ref", lm={}))
    _replay(outs, _cfg("ref"), 5, "ref", cams=cams)


def test_keyframes():
    cfg = _cfg("conv", keyframe_max_frames=2)
    outs = tb.run(cfg, 5, _wide_idx(5), kf=True, **_term(_wide_idx(5), "conv", lm={}))
    _replay(outs, cfg, 5, "conv", kf=True)


def test_pose_guess():
    B = 5
    rng = np.random.default_rng(5)
    guess = [(rng.normal(size=(B, 6)) * 2e-3).astype(np.float32) for _ in range(3)]
    outs = tb.run(_cfg("conv"), B, _wide_idx(B), **_term(_wide_idx(B), "conv", lm={}, guess=guess))
    for k in (1, 2):
        assert outs[k]["start"].tobytes() == guess[k].tobytes()
    _replay(outs, _cfg("conv"), B, "conv", guess=guess)


def test_actions_and_camera_change_leave_zero_records():
    acts = tb.acts(5, 3, 9)
    assert (acts[1:] == SKIP).any() and (acts[1:] == RESTART).any()
    outs = tb.run(_cfg("ref"), 5, _wide_idx(5), acts=acts, **_term(_wide_idx(5), "ref", lm={}))
    tot = _replay(outs, _cfg("ref"), 5, "ref", min_tracked=3)
    assert sum(int((o["status"] != TRACKED).sum()) for o in outs[1:]) >= 2 and tot["n"] >= 3
    # a camera change restarts the sequence: a zero record and an empty log; a bad action likewise
    g, d, s = tb.frames(SIZE, 0.1)
    bt = dvo.Batch(3, KH, SIZE[0], SIZE[1], LEVELS, CULLS, cfg=_cfg("ref"))
    bt.set_step_control()
    for k in range(3):
        if k == 2:
            cams = np.stack([KH] * 3).astype(np.float32)
            cams[1, 0, 0] *= 1.02
            bt.set_intrinsics(cams)
            bt.set_actions(np.array([TRACK, TRACK, 7], np.uint8))
        t = [tb.dev(x[[k, k + 1, k + 2]]) for x in (g, d, s)]
        bt.push_device(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr())
        o = dict(rec=bt.last_step_control(), lmlogs=[bt.last_step_control_log(b) for b in range(3)], status=bt.last_status())
        for b in range(3):
            if k == 0 or (k == 2 and b > 0):
                assert o["status"][b] != TRACKED
                _empty(o, b)
            else:
                assert o["status"][b] == TRACKED and o["rec"][b]["n_first"] == LEVELS and o["lmlogs"][b]["n_iter"][:LEVELS].all()
    bt.close()


@pytest.mark.parametrize("mode", ["plain", "actions", "keyframes"])
def test_set_then_cleared_is_never_set(mode):
    kw = dict(acts=tb.acts(5, 3, 3) if mode == "actions" else None, kf=mode == "keyframes")
    cfg = _cfg("conv", keyframe_max_frames=2) if mode == "keyframes" else _cfg("conv")
    idx = _wide_idx(5)
    tb.same(tb.run(cfg, 5, idx, **_term(idx, "conv"), **kw), tb.run(cfg, 5, idx, **_term(idx, "conv", lm={}, clear=True), **kw))


class StepControlReplay(lockstep.Replay):
    """lockstep.Replay whose tracking step restates the step-control contract (tests/lm_ref.py) instead of the plain comparison"""
    lm_log = None
    result = None

    def _track(self, obj, ref, log):
        cfg = dvo.default_config()
        sums = lambda l, xi: orc.optimize(obj.gray(l), ref.gray(l), ref.depth(l), ref.sigma(l), ref.K(l), xi, l, crop=self.crop)
        self.result = lr.replay_call(log, self.lm_log, sums, lockstep.LEVELS, lr.params(), cfg.max_iterations, cfg.min_update, cfg.min_residual,
                                     tag=self._where("step control"))
        self.n_iterations += self.result["iterations"]
        return self.result["xi"]


def test_mono_batch_follows_the_contract():
    """a mono batch (the reference's constants, crop on, the automatic plan) through tests/lockstep.py: the mapping runs from the
    accepted pose, and the oracle's keyframes stay equal to the GPU's bit for bit"""
    import test_gpu_mono_lockstep as ml
    orc.set_tracker_params()
    g, _ = ml.render(K640)
    init = ml.init_depth(K640)
    sig = np.full_like(init, ml.INIT_SIGMA)
    B, seed = 2, 3
    orders = [[0, 1, 2, 3], [5, 4, 3, 2]]
    mb = dvo.MonoBatch(B, K640, 640, 480, ring_keyframes=16, cfg=dvo.default_config(rng_seed=seed))
    mb.setInitialDepth(init, sig)
    mb.set_step_control()
    assert all(mb.level_plan(l)["schedule"] == dvo.PLAN_PAIRS for l in range(lockstep.LEVELS))
    reps = [StepControlReplay(K640, 640, 480, seed, init, sig, name="sequence %d" % q) for q in range(B)]
    n = 0
    for k in range(len(orders[0])):
        fr = np.stack([g[orders[q][k]] for q in range(B)])
        t = tb.dev(fr)
        mb.odometrize_device(t.data_ptr())
        rec = mb.last_step_control()
        for q, gf in enumerate(lockstep.batch_frames(mb, k == 0)):
            reps[q].lm_log = mb.last_step_control_log(q)
            reps[q].result = None
            reps[q].step(fr[q], gf)
            if k == 0:
                assert rec[q]["n_first"] == 0 and not reps[q].lm_log["n_iter"].any()
                continue
            r = reps[q].result
            assert (rec[q]["n_first"], rec[q]["n_accepted"], rec[q]["n_rejected"]) == (lockstep.LEVELS, r["accepts"], r["rejects"])
            n += 1
    mb.close()
    assert n == B * (len(orders[0]) - 1)


# ------------------------------------------------------------------------------------------------------------------ 7: refusals
def test_errors_are_refused():
    import ctypes as C
    L = dvo.lib()
    bt = dvo.Batch(2, KH, SIZE[0], SIZE[1], LEVELS, CULLS, cfg=_cfg("conv"))
    from test_step_control_abi import BAD_CONFIGS
    for bad in BAD_CONFIGS:
        if bad == dict(mode=dvo.LM_OFF):
            continue
        c = dvo.lm_default_config()
        for k, v in bad.items():
            setattr(c, k, v)
        assert L.dvo_batch_set_step_control(bt._p, C.byref(c)) == dvo.DVO_ERR_BAD_ARGUMENT, bad
        assert L.dvo_last_error().decode().startswith("dvo_batch_set_step_control: "), bad
    with pytest.raises(dvo.DvoError):
        bt.last_step_control()                      # nothing pushed
    with pytest.raises(dvo.DvoError):
        bt.last_step_control_log(0)
    # the other terms refuse step control, and it refuses them, each naming the offender
    others = [("robust weights", lambda: bt.set_robust_weights(dvo.ROBUST_HUBER, 1.345), lambda: bt.set_robust_weights(None)),
              ("median", lambda: bt.set_robust_median(dvo.ROBUST_HUBER, 1.345), lambda: bt.set_robust_weights(None)),
              ("affine", lambda: bt.set_affine_brightness(dvo.AFFINE_ESTIMATE), lambda: bt.set_affine_brightness(None)),
              ("geometric", lambda: bt.set_geometric(), lambda: bt.set_geometric(None)),
              ("geometric", lambda: bt.set_geometric_affine(), lambda: (bt.set_geometric(None), bt.set_affine_brightness(None)))]
    for word, on, off in others:
        on()
        with pytest.raises(dvo.DvoError, match=word):
            bt.set_step_control()
        bt.set_step_control(dvo.LM_OFF)             # turning off is always allowed
        bt.set_step_control(None)
        off()
        bt.set_step_control()
        with pytest.raises(dvo.DvoError, match="step control"):
            on()
        off()                                       # (turning the other term off is allowed while step control is on)
        bt.set_step_control(None)
    g, d, s = tb.frames(SIZE, 0.5)
    t = [tb.dev(x[:2]) for x in (g, d, s)]
    bt.push_device(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr())
    with pytest.raises(dvo.DvoError):
        bt.last_step_control()                      # the push ran without step control
    bt.set_step_control()
    with pytest.raises(dvo.DvoError):
        bt.last_step_control()                      # enabled from the next push on
    t2 = [tb.dev(x[1:3]) for x in (g, d, s)]
    bt.push_device(t2[0].data_ptr(), t2[1].data_ptr(), t2[2].data_ptr())
    assert (bt.last_step_control()["n_first"] == LEVELS).all()
    lg = dvo.LmLog()
    lg.struct_size = 4
    assert L.dvo_batch_last_step_control_log(bt._p, 0, C.byref(lg)) == dvo.DVO_ERR_BAD_ARGUMENT
    lg.struct_size = C.sizeof(dvo.LmLog)
    assert L.dvo_batch_last_step_control_log(bt._p, 2, C.byref(lg)) == dvo.DVO_ERR_BAD_ARGUMENT
    assert L.dvo_batch_last_step_control_log(bt._p, -1, C.byref(lg)) == dvo.DVO_ERR_BAD_ARGUMENT
    assert L.dvo_batch_last_step_control_log(bt._p, 0, None) == dvo.DVO_ERR_BAD_ARGUMENT
    assert L.dvo_batch_last_step_control(bt._p, None) == dvo.DVO_ERR_BAD_ARGUMENT
    bt.set_step_control(None)
    bt.push_device(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr())
    with pytest.raises(dvo.DvoError):
        bt.last_step_control()                      # off again: the last push did not run with it
    bt.close()
    mb = dvo.MonoBatch(2, K640, 640, 480, cfg=dvo.default_config(rng_seed=3))
    mb.set_robust_weights(dvo.ROBUST_HUBER, 1.345)
    with pytest.raises(dvo.DvoError, match="robust weights"):
        mb.set_step_control()
    mb.set_robust_weights(None)
    mb.set_step_control()
    with pytest.raises(dvo.DvoError, match="step control"):
        mb.set_affine_brightness(dvo.AFFINE_ESTIMATE)
    mb.close()


# ------------------------------------------------------------------------------------------------------------------ 8: the outcome
OUTCOME = dict(seeds=range(42, 47), sigma=0.1, sigma_t=0.005, sigma_r_deg=0.3, its=15)


def _truth(poses, k):
    return orc.se3_log((np.linalg.inv(poses[k]) @ poses[0]).astype(np.float32)).astype(np.float64)


def test_step_control_wins_where_the_plain_iteration_diverges():
    """The reference's own constants on sigma 0.1, 5 mm / 0.3 degree motions (over-relaxed): frames 1 and 2 of five scenes
    each tracked against frame 0, ten pairs, the same config on both sides.  The replica on the oracle gives W wins and the ratio R of
    the summed errors and must itself show the effect; the GPU must reach W - 1 wins and (R + 1) / 2, the project's midpoint rule (the
    plain side is chaotic and moves from run to run, the damped side does not).  On the device, also: the accepted residuals of every
    sequence and level never increase, and the returned pose is the last accepted one."""
    orc.set_tracker_params(min_residual=0.0, min_update=MIN_UPDATE)
    obj, refs, truth, reps = [], [], [], dict(plain=[], lm=[])
    P = lr.params()
    for seed in OUTCOME["seeds"]:
        g, d, s, poses = synth.sequence(3, 320, 240, KH, seed=seed, sigma_value=OUTCOME["sigma"], sigma_t=OUTCOME["sigma_t"],
                                        sigma_r_deg=OUTCOME["sigma_r_deg"])
        g, d, s = g.numpy(), d.numpy(), s.numpy()
        ref = orc.OFrame(g[0], d[0], s[0], KH, LEVELS, CULLS)
        for k in (1, 2):
            obj.append((g[k], d[k], s[k])); refs.append((g[0], d[0], s[0])); truth.append(_truth(poses, k))
            sums = lr.oracle_sums(orc.OFrame(g[k], d[k], s[k], KH, LEVELS, CULLS), ref)
            reps["plain"].append(lr.plain_track(sums, LEVELS, OUTCOME["its"], MIN_UPDATE, 0.0)[0])
            reps["lm"].append(lr.lm_track(sums, LEVELS, P, OUTCOME["its"], MIN_UPDATE, 0.0)[0])
    B = len(obj)
    err = lambda xs: np.array([np.linalg.norm(np.asarray(x, np.float64) - t) for x, t in zip(xs, truth)])
    rp, rl = err(reps["plain"]), err(reps["lm"])
    W, R = int((rl < rp).sum()), rl.sum() / rp.sum()
    assert W >= 9 and R <= 0.05, ("the replica alone", W, R, rp, rl)
    cfg = _cfg("ref", max_iterations=OUTCOME["its"])
    got = {}
    for name in ("plain", "lm"):
        bt = dvo.Batch(B, KH, 320, 240, LEVELS, CULLS, cfg=cfg)
        if name == "lm":
            bt.set_step_control()
        for frames in (refs, obj):
            t = [tb.dev(np.stack([f[i] for f in frames])) for i in range(3)]
            bt.push_device(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr())
        xi, _ = bt.last_poses()
        got[name] = xi.copy()
        if name == "lm":
            rec = bt.last_step_control()
            for b in range(B):
                lg, ll = bt.last_track_log(b), bt.last_step_control_log(b)
                last = None
                for l in range(LEVELS):
                    n = int(lg["n_iter"][l])
                    assert n == int(ll["n_iter"][l]) >= 1 and ll["decision"][l][0] == FIRST, (b, l)
                    acc, pose = [], None
                    for it in range(n):
                        if ll["decision"][l][it] != REJECT:
                            acc.append(lg["residual"][l][it])
                            pose = (np.zeros(6, np.float32) if last is None else last) if it == 0 else lg["xi_after"][l][it - 1]
                    assert all(a >= c for a, c in zip(acc, acc[1:])), (b, l, acc)
                    last = np.asarray(lg["xi_after"][l][n - 1], np.float32)
                    assert last.tobytes() == np.asarray(pose, np.float32).tobytes(), (b, l, "the level ends on the last accepted pose")
                assert xi[b].tobytes() == last.tobytes() and F32(rec[b]["residual"]).tobytes() == F32(acc[-1]).tobytes(), b
        bt.close()
    ep, el = err(got["plain"]), err(got["lm"])
    wins, ratio = int((el < ep).sum()), el.sum() / ep.sum()
    print("\nstep control: GPU wins %d of %d, summed error %.4g against plain %.4g (ratio %.4g); replica wins %d, %.4g against %.4g (ratio %.4g); "
          "GPU rejects %d, evaluations %d" % (wins, B, el.sum(), ep.sum(), ratio, W, rl.sum(), rp.sum(), R, int(rec["n_rejected"].sum()),
                                              int((rec["n_first"] + rec["n_accepted"] + rec["n_rejected"]).sum())))
    assert wins >= W - 1 and ratio <= (R + 1) / 2, (wins, ratio, W, R, ep, el)


def test_zz_report_ratios():
    """last in the file: under -s, the largest backward error / bound ratio of the updates this process has replayed"""
    if lr.RATIOS:
        tag, worst = max(lr.RATIOS, key=lambda r: r[1])
        print("\ntest_gpu_step_control: %d updates, largest backward error / TOL_BACKWARD %.3g (%s)" % (len(lr.RATIOS), worst, tag))
    gn_sums.report("test_gpu_step_control")
    assert all(r <= 1.0 for _, r in lr.RATIOS) and all(r <= 1.0 for _, r in gn_sums.RATIOS)
