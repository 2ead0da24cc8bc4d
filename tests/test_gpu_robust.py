"""Robust residual weights of a batch (dvo_batch_set_robust_weights, include/dvo.h) on the GPU, both batch kinds.

Off is today's bits; weights that are 1 everywhere give the plain batch's bits; the operator and every logged iteration of a weighted
batch match the contract restated on the oracle's per-pixel terms (tests/robust_ref.py): the scale follows the rule, n_valid is equal,
the logged update solves the weighted normal equations and the finest level's record sits inside the reduction bound; the schedules give
the same records; and with an occluder in the view both robust kinds beat the plain estimator.

Everything runs on 320x240 frames, 3 levels, culls 1, crop off, 4 pixels per thread: the levels are 40x30 and 80x60 (raster tiles;
gn_tiling takes 16-column tiles only from 128 rows up) and 160x120 (32-column 2-D tiles), with border queues live on all three.  One
case runs at 328x248, where the finest level (164x124) is raster as well.  The step and stop constants are the converging ones of
bench.py (steps 1.0 / 0.75 / 0.5, stop on the update norm), so that a level runs several iterations and the adaptive scale has a
previous residual of the same level to follow."""
import numpy as np
import pytest

import dvo_amd as dvo
import gn_sums
import lockstep
import orc
import robust_ref as rr
import term_batch as tb
from dvo_amd import synth
from term_batch import CULLS, FLOOR, HUBER, KH, LEVELS, PARAM, SIZE, SKIP, RESTART, STARTED, STEPS, STUDENT, TOP, TRACKED
from util import K640

pytestmark = pytest.mark.gpu

ADAPTIVE, GIVEN = dvo.ROBUST_SCALE_ADAPTIVE, dvo.ROBUST_SCALE_GIVEN


@pytest.fixture(scope="module", autouse=True)
def _oracle_steps():
    with tb.oracle_steps():
        yield


def _given_scales(B):
    return (0.012 + 0.004 * np.arange(B)).astype(np.float32)


def _weights(rob=None, scales=None, scales_on_device=False, clear=False):
    """run() keywords of a weighted batch.  rob: set_robust_weights arguments (clear: set, then turned off before the first push);
    scales: GIVEN rows"""
    def setup(bt, keep):
        bt.set_robust_weights(**rob)
        if scales is not None:
            if scales_on_device:
                keep.append(tb.dev(np.asarray(scales, np.float32)))
                bt.set_robust_scales(keep[-1].data_ptr(), on_device=True)
            else:
                bt.set_robust_scales(scales)
        if clear:
            bt.set_robust_weights(dvo.ROBUST_NONE)
    return dict(setup=setup, reads=() if clear else ("robust",)) if rob else {}


# ------------------------------------------------------------------------------------------------------------------ 1: off is today
@pytest.mark.parametrize("mode", ["plain", "actions", "keyframes"])
def test_off_means_today(mode):
    kw = dict(acts=tb.acts(5, 3, 3) if mode == "actions" else None, kf=mode == "keyframes")
    cfg = tb.cfg(keyframe_max_frames=2) if mode == "keyframes" else tb.cfg()
    tb.same(tb.run(cfg, 5, tb.wide_idx(5), **kw), tb.run(cfg, 5, tb.wide_idx(5), **_weights(tb.rob(HUBER), clear=True), **kw))


def _mono_run(rob=None, clear=False):
    g, init, ml = tb.mono_frames()
    mb = dvo.MonoBatch(3, K640, 640, 480, ring_keyframes=16, cfg=dvo.default_config(rng_seed=tb.MONO_SEED))
    mb.setInitialDepth(init, np.full_like(init, ml.INIT_SIGMA))
    mb.set_track_quality(True)
    if rob:
        mb.set_robust_weights(**rob)
        if clear:
            mb.set_robust_weights(None)
    outs = []
    for k in range(len(tb.MIDX)):
        t = tb.dev(g[list(tb.MIDX[k])])
        mb.odometrize_device(t.data_ptr())
        xi, T, key = mb.world_poses()
        outs.append(dict(xi=xi.copy(), T=T.copy(), key=key.copy(), status=mb.last_status(), q=mb.last_track_quality(),
                         logs=[mb.last_track_log(b) for b in range(3)] if k > 0 else []))
    mb.close()
    return outs


def test_mono_off_means_today():
    a, b = _mono_run(), _mono_run(rob=tb.rob(STUDENT), clear=True)
    for k, (x, y) in enumerate(zip(a, b)):
        for f in ("xi", "T", "status", "key"):
            np.testing.assert_array_equal(x[f], y[f], err_msg="call %d %s" % (k, f))
        assert [tb.logbits(l) for l in x["logs"]] == [tb.logbits(l) for l in y["logs"]], k
        assert x["q"].tobytes() == y["q"].tobytes(), k


# ------------------------------------------------------------------------------------------------------------------ 2: rho = 1 is plain
@pytest.mark.parametrize("variant", ["huber_huge_scale", "bad_scales", "student_inf_scale"])
def test_unit_weights_are_the_plain_batch(variant):
    B = 5
    idx = tb.wide_idx(B)
    plain = tb.run(tb.cfg(), B, idx)
    if variant == "huber_huge_scale":
        sc = np.full(B, 1e6, np.float32); rob = tb.rob(HUBER, GIVEN); want = np.float32(1e6) * np.float32(1e6)
    elif variant == "bad_scales":
        sc = np.float32([0.0, -1.0, np.nan, -np.inf, 0.0]); rob = tb.rob(HUBER, GIVEN); want = np.float32(np.inf)
    else:
        sc = np.full(B, np.inf, np.float32); rob = tb.rob(STUDENT, GIVEN); want = np.float32(np.inf)
    got = tb.run(tb.cfg(), B, idx, **_weights(rob, sc))
    tb.same(plain, got, families=())
    for o in got[1:]:
        np.testing.assert_array_equal(o["s2"], np.full(B, want, np.float32))
    assert not got[0]["s2"].any()   # nothing tracked at the first push


# ------------------------------------------------------------------------------------------------------------------ 3: the operator
@pytest.fixture(scope="module")
def plain_run():
    return tb.run(tb.cfg(), 3, tb.wide_idx(3))


def _op(obj, ref, l, xi, kind, param, s2, cfg):
    return dvo.optimize_robust(obj.gray(l), ref.gray(l), ref.depth(l), ref.sigma(l), ref.K(l), xi, l, kind, param, s2, cfg=cfg)


@pytest.mark.parametrize("kind", [HUBER, STUDENT])
def test_operator_matches_the_contract(kind, plain_run):
    cfg = tb.cfg()
    depth = gn_sums.depth_for_cfg(cfg)
    before = rr.nonempty_calls()
    idx = tb.wide_idx(3)
    obj, ref = tb.oframe(idx[1][0]), tb.oframe(idx[0][0])
    poses = tb.level_poses(plain_run[1]["logs"][0])
    for l in range(LEVELS):
        t = orc.optimize_terms(obj.gray(l), ref.gray(l), ref.depth(l), ref.sigma(l), ref.K(l), poses[l], l, crop=False)
        assert t["n_valid"] > 500
        for s2 in (1e-4, 1e-3, 1e-2):
            got = _op(obj, ref, l, poses[l], kind, PARAM[kind], s2, cfg)
            ex = rr.assert_sums(got, t, kind, PARAM[kind], s2, depth, "operator kind %d level %d s2 %g" % (kind, l, s2))
            assert (ex["rho"] != 1).any() or (kind == HUBER and s2 > 1e-4)   # (the smallest scale leaves pixels beyond Huber's threshold)
            assert np.float32(got["residual"]) == np.float32(got["sum_r2"]) / np.float32(got["n_valid"])
    assert rr.nonempty_calls() == before + 9


def test_operator_edge_cases(plain_run):
    cfg = tb.cfg()
    depth = gn_sums.depth_for_cfg(cfg)
    idx = tb.wide_idx(3)
    obj, ref = tb.oframe(idx[1][1]), tb.oframe(idx[0][1])
    poses = tb.level_poses(plain_run[1]["logs"][1])
    for l in range(LEVELS):
        t = orc.optimize_terms(obj.gray(l), ref.gray(l), ref.depth(l), ref.sigma(l), ref.K(l), poses[l], l, crop=False)
        # every pixel beyond the Huber threshold: c = k * sqrt(1e-30)
        assert (np.abs(t["r"]) > np.float32(1.345) * np.sqrt(np.float32(1e-30))).all()
        ex = rr.assert_sums(_op(obj, ref, l, poses[l], HUBER, 1.345, 1e-30, cfg), t, HUBER, 1.345, 1e-30, depth, "all outliers level %d" % l)
        assert (ex["rho"] < 1).all()
        # kind NONE and a scale that is not > 0: the plain operator's bits
        p = dvo.optimize(obj.gray(l), ref.gray(l), ref.depth(l), ref.sigma(l), ref.K(l), poses[l], l, cfg=cfg)
        for kind, s2 in ((dvo.ROBUST_NONE, 1.0), (HUBER, 0.0), (STUDENT, float("nan")), (STUDENT, float("inf"))):
            q = _op(obj, ref, l, poses[l], kind, 1.0, s2, cfg)
            assert q["n_valid"] == p["n_valid"] and q["sum_r2"] == p["sum_r2"] and np.array_equal(q["H"], p["H"]) and np.array_equal(q["g"], p["g"])
            assert np.array_equal(q["xi_update"], p["xi_update"])
    # r = 0 everywhere: a constant image against itself (only the few border pixels whose gradient comes from the fill rule have a
    # non-zero J).  Huber's rho is 1 there and Student-t's (nu + 1) / nu; g and sum_r2 are exact zeros and nothing is NaN.  Then
    # identical frames, whose residuals are zero up to the warp's rounding.
    flat = np.full_like(ref.gray(TOP), 0.5)
    t = orc.optimize_terms(flat, flat, ref.depth(TOP), ref.sigma(TOP), ref.K(TOP), np.zeros(6, np.float32), TOP, crop=False)
    assert t["n_valid"] > 1000 and not t["r"].any()
    for kind in (HUBER, STUDENT):
        got = dvo.optimize_robust(flat, flat, ref.depth(TOP), ref.sigma(TOP), ref.K(TOP), np.zeros(6, np.float32), TOP, kind, PARAM[kind], 1e-3, cfg=cfg)
        ex = rr.assert_sums(got, t, kind, PARAM[kind], 1e-3, depth, "r = 0 kind %d" % kind)
        assert got["sum_r2"] == 0.0 and not got["g"].any() and got["residual"] == 0.0 and np.isfinite(got["H"]).all()
        want = np.float32(1) if kind == HUBER else (np.float32(6) * np.float32(1e-3)) / (np.float32(5) * np.float32(1e-3))
        assert (ex["rho"] == want).all()
    t = orc.optimize_terms(ref.gray(TOP), ref.gray(TOP), ref.depth(TOP), ref.sigma(TOP), ref.K(TOP), np.zeros(6, np.float32), TOP, crop=False)
    assert np.abs(t["r"]).max() < 1e-5
    got = _op(ref, ref, TOP, np.zeros(6, np.float32), STUDENT, 5.0, 1e-3, cfg)
    ex = rr.assert_sums(got, t, STUDENT, 5.0, 1e-3, depth, "identical frames")
    assert np.all(np.abs(ex["rho"] - np.float32(1.2)) <= 2e-7)


# ------------------------------------------------------------------------------------------------------------------ 4: batch lockstep
def _check_sequence(o, b, obj, ref, rob, given, depth, where):
    """one TRACKED sequence of one push: every logged iteration against the contract, the reported scale, the finest level's record"""
    kind, param, mode = rob["kind"], rob["param"], rob["scale_mode"]
    lg = o["logs"][b]
    given_s2 = None
    if mode == GIVEN:
        given_s2 = np.float32(given[b]) * np.float32(given[b])
    last, n_it = rr.replay_call(lg, rr.oracle_terms(obj, ref, False), LEVELS, kind, param, mode, floor2=tb.floor2(), given_s2=given_s2, tag=where,
                                depth=depth)
    t, s2, l, it = last
    assert l == TOP and it == int(lg["n_iter"][TOP]) - 1
    assert np.float32(o["s2"][b]).tobytes() == np.float32(s2).tobytes(), (where, o["s2"][b], s2)
    q = o["q"][b]
    assert q["status"] == TRACKED and q["n_valid"] == int(lg["n_valid"][TOP][it]), where
    assert np.float32(q["residual"]).tobytes() == np.float32(lg["residual"][TOP][it]).tobytes(), where
    rr.assert_sums(q, t, kind, param, s2, gn_sums.at_level(depth, TOP), where)
    return n_it


def _lockstep(cfg, B, rob, acts=None, kf=False, cams=None, size=SIZE, scales_on_device=False, outs=None, min_tracked=None, seqs=None,
              depth=None):
    """seqs: the sequences replayed against the oracle (None: all; the others keep the no-stale-scale check); depth: the reduction depth,
    one value or one per level (None: the config's)"""
    idx = tb.wide_idx(B)
    given = _given_scales(B) if rob["scale_mode"] == GIVEN else None
    if outs is None:
        outs = tb.run(cfg, B, idx, acts=acts, kf=kf, cams=cams, size=size, **_weights(rob, given, scales_on_device))
    depth = gn_sums.depth_for_cfg(cfg) if depth is None else depth
    before = rr.nonempty_calls()

    def check(k, b, kr, o, K):
        return _check_sequence(o, b, tb.oframe(idx[k][b], K, size), tb.oframe(idx[kr][b], K, size), rob, given, depth,
                               "push %d seq %d of %d" % (k, b, B))
    # (SKIPPED / STARTED: no stale scale)
    n, _ = tb.walk(outs, B, check, lambda o, b: o["s2"][b] == 0.0, kf=kf, cams=cams, seqs=seqs, min_tracked=min_tracked)
    assert rr.nonempty_calls() >= before + n // 2
    return outs


@pytest.mark.parametrize("B", [3, 11])
@pytest.mark.parametrize("mode", [ADAPTIVE, GIVEN])
@pytest.mark.parametrize("kind", [HUBER, STUDENT])
def test_batch_lockstep(kind, mode, B):
    """B = 11: k_gn_solve_rw takes 8 sequences per workgroup, so the second workgroup is partly filled"""
    _lockstep(tb.cfg(), B, tb.rob(kind, mode))


def test_batch_lockstep_raster_finest_level():
    _lockstep(tb.cfg(), 3, tb.rob(HUBER), size=(328, 248))


@pytest.fixture(scope="module")
def base5():
    """Huber, adaptive scale, five sequences on the default schedule: what the schedule variants must reproduce bit for bit"""
    return _lockstep(tb.cfg(), 5, tb.rob(HUBER))


@pytest.mark.parametrize("variant", ["adaptive_off", "fused_tiles", "single_launch", "lds_patch", "host_feed"])
def test_schedule_variants_give_the_same_records(variant, base5):
    cfg = tb.cfg(**tb.SCHEDULE_VARIANTS.get(variant, {}))
    other = tb.run(cfg, 5, tb.wide_idx(5), **_weights(tb.rob(HUBER)), feed="host" if variant == "host_feed" else "device")
    tb.same(base5, other)   # (the scales included)
    _lockstep(tb.cfg(), 5, tb.rob(HUBER), outs=other)


def test_two_streams():
    """two sub-batches need more than 16 sequences (19: not a multiple of 8 either); the table is offset per sub-batch"""
    one = _lockstep(tb.cfg(), 19, tb.rob(STUDENT))
    two = tb.run(tb.cfg(track_streams=2), 19, tb.wide_idx(19), **_weights(tb.rob(STUDENT)))
    tb.same(one, two)   # (the scales included)


def test_raw_feed():
    a = tb.run(tb.cfg(), 5, tb.wide_idx(5), feed="raw", **_weights(tb.rob(STUDENT)))
    b = tb.run(tb.cfg(), 5, tb.wide_idx(5), feed="raw_host", **_weights(tb.rob(STUDENT)))
    tb.same(a, b)
    assert all((o["s2"] > 0).all() and np.isfinite(o["s2"]).all() for o in a[1:])


def test_per_sequence_intrinsics():
    _lockstep(tb.cfg(), 5, tb.rob(HUBER), cams=tb.sequence_cams(5))


def test_actions_and_device_scales():
    """SKIP / RESTART leave no stale scale (checked in _lockstep), and device-resident scale rows are read in stream order"""
    for rob, seed, dev in ((tb.rob(STUDENT, GIVEN), 9, True), (tb.rob(HUBER), 4, False)):
        acts = tb.acts(5, 3, seed)
        assert (acts[1:] == SKIP).any() and (acts[1:] == RESTART).any()
        _lockstep(tb.cfg(), 5, rob, acts=acts, scales_on_device=dev, min_tracked=3)


def test_keyframes():
    _lockstep(tb.cfg(keyframe_max_frames=2), 5, tb.rob(HUBER), kf=True)


def test_device_scales_follow_the_stream():
    """rows written on the device before each push are the rows that push uses"""
    import torch
    B = 3
    g, d, s = tb.frames()
    bt = dvo.Batch(B, KH, SIZE[0], SIZE[1], LEVELS, CULLS, cfg=tb.cfg())
    bt.set_robust_weights(**tb.rob(HUBER, GIVEN))
    rows = torch.zeros(B, dtype=torch.float32, device="cuda")
    bt.set_robust_scales(rows.data_ptr(), on_device=True)
    keep = []
    for k, val in enumerate((0.5, 0.02, 0.07)):
        rows.fill_(val)
        torch.cuda.synchronize()
        t = [tb.dev(x[[k, k + 1, k + 2]]) for x in (g, d, s)]
        keep.append(t)
        bt.push_device(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr())
        s2 = bt.last_robust_scales()
        want = np.float32(val) * np.float32(val) if k > 0 else np.float32(0)
        np.testing.assert_array_equal(s2, np.full(B, want, np.float32))
    bt.close()


# ------------------------------------------------------------------------------------------------------------------ 5: mono batch
class RobustReplay(lockstep.Replay):
    """lockstep.Replay whose tracking step restates the weighted contract (tests/robust_ref.py) instead of the plain comparison"""
    rob = None
    last = None
    depth = 17      # reduction depth, one value or one per level (gn_sums.plan_depths of the batch)

    def _track(self, obj, ref, log):
        last, n = rr.replay_call(log, rr.oracle_terms(obj, ref, self.crop), lockstep.LEVELS, self.rob["kind"], self.rob["param"], ADAPTIVE,
                                 floor2=tb.floor2(), tag=self._where("robust"), depth=self.depth)
        self.last = last
        self.n_iterations += n
        return np.asarray(log["xi_after"][lockstep.TOP][int(log["n_iter"][lockstep.TOP]) - 1], np.float32).copy()


def _mono_contract(per_camera):
    """a mono batch with the default tile config (the automatic plan) and Huber weights through tests/lockstep.py; per_camera: the
    k_track_gn_rw_cam kernels"""
    orc.set_tracker_params()    # the mono batch of this test runs the reference's constants
    try:
        g, init, ml = tb.mono_frames()
        B = 2
        orders = [[0, 1, 2, 3], [5, 4, 3, 2]]
        sig = np.full_like(init, ml.INIT_SIGMA)
        rob = tb.rob(HUBER)
        Ks = tb.sequence_cams(B, K640) if per_camera else [K640] * B
        mb = dvo.MonoBatch(B, Ks if per_camera else K640, 640, 480, ring_keyframes=16, cfg=dvo.default_config(rng_seed=tb.MONO_SEED),
                           per_sequence_K=per_camera)
        mb.setInitialDepth(init, sig)
        mb.set_track_quality(True)
        mb.set_robust_weights(**rob)
        depths = tb.mono_plan(mb)
        reps = [RobustReplay(Ks[q], 640, 480, tb.MONO_SEED, init, sig, name="sequence %d" % q) for q in range(B)]
        for r in reps:
            r.depth = depths
        before = rr.nonempty_calls()
        n = 0
        for k in range(len(orders[0])):
            fr = np.stack([g[orders[q][k]] for q in range(B)])
            t = tb.dev(fr)
            mb.odometrize_device(t.data_ptr())
            rec = mb.last_track_quality()
            s2 = mb.last_robust_scales()
            for q, gf in enumerate(lockstep.batch_frames(mb, k == 0)):
                reps[q].rob = rob
                reps[q].last = None
                reps[q].step(fr[q], gf)
                if k == 0:
                    assert rec["status"][q] == STARTED and s2[q] == 0.0
                    continue
                terms, want, l, it = reps[q].last
                assert l == lockstep.TOP
                assert np.float32(s2[q]).tobytes() == np.float32(want).tobytes(), (k, q, s2[q], want)
                rr.assert_sums(rec[q], terms, HUBER, rob["param"], want, depths[lockstep.TOP], "mono%s call %d seq %d" % (" per-camera" if per_camera else "", k, q))
                n += 1
        mb.close()
        assert n == B * (len(orders[0]) - 1) and rr.nonempty_calls() > before
    finally:
        orc.set_tracker_params(step3=STEPS, min_residual=0.0, min_update=2e-5)


def test_mono_records_match_the_contract():
    _mono_contract(False)


def test_mono_records_match_the_contract_per_camera():
    _mono_contract(True)


# ------------------------------------------------------------------------------------------------------------------ 6: it helps
def test_robust_weights_beat_plain_under_an_occluder():
    """Ten object frames with a random-texture rectangle over a fifth to a quarter of the view, one batch of ten sequences per estimator.
    Each robust kind must be closer to the true motion than plain in at least 8 of the 10 cases and its summed error at most 0.7 times
    plain's.  The numpy replica of the contract on the oracle (robust_ref.irls_track) gives 10 of 10 and 0.49 / 0.43; it runs beside
    the GPU here so that a miss can be told from a difference of the two."""
    g, d, s, poses = synth.sequence(3, 320, 240, KH, seed=42, sigma_value=0.5, sigma_t=0.01, sigma_r_deg=0.5)
    g, d, s = g.numpy(), d.numpy(), s.numpy()
    gt = tb.se3_log_rel(poses[1], poses[0])
    cases = [(f, seed) for f in (0.2, 0.25) for seed in range(7, 12)]
    obj = []
    for f, seed in cases:
        hh, ww = int(240 * np.sqrt(f)), int(320 * np.sqrt(f))
        y0, x0 = (240 - hh) // 2 + 10, (320 - ww) // 2 - 15
        im = g[1].copy()
        im[y0:y0 + hh, x0:x0 + ww] = np.random.default_rng(seed).random((hh, ww), np.float32) * 0.9 + 0.05
        obj.append(im)
    obj = np.stack(obj)
    B = len(cases)
    cfg = tb.cfg(max_iterations=15)
    err, rep = {}, {}
    ref = orc.OFrame(g[0], d[0], s[0], KH, LEVELS, CULLS)
    for kind in (dvo.ROBUST_NONE, HUBER, STUDENT):
        bt = dvo.Batch(B, KH, 320, 240, LEVELS, CULLS, cfg=cfg)
        if kind != dvo.ROBUST_NONE:
            bt.set_robust_weights(kind, PARAM[kind], ADAPTIVE, FLOOR)
        t0 = [tb.dev(np.stack([x[0]] * B)) for x in (g, d, s)]
        bt.push_device(t0[0].data_ptr(), t0[1].data_ptr(), t0[2].data_ptr())
        t1 = [tb.dev(obj), tb.dev(np.stack([d[1]] * B)), tb.dev(np.stack([s[1]] * B))]
        bt.push_device(t1[0].data_ptr(), t1[1].data_ptr(), t1[2].data_ptr())
        xi, _ = bt.last_poses()
        bt.close()
        err[kind] = np.array([np.linalg.norm(xi[b].astype(np.float64) - gt) for b in range(B)])
        rep[kind] = np.array([np.linalg.norm(rr.irls_track(orc.OFrame(obj[b], d[1], s[1], KH, LEVELS, CULLS), ref, LEVELS, kind,
                                                           PARAM.get(kind, 1.0), tb.floor2(), False, 15, 2e-5)[0].astype(np.float64) - gt)
                              for b in range(B)])
    for kind in (HUBER, STUDENT):
        wins, ratio = int((err[kind] < err[0]).sum()), err[kind].sum() / err[0].sum()
        rwins, rratio = int((rep[kind] < rep[0]).sum()), rep[kind].sum() / rep[0].sum()
        print("\nkind %d: GPU wins %d of %d, error ratio %.3f; replica wins %d, ratio %.3f" % (kind, wins, B, ratio, rwins, rratio))
        assert rwins >= 8 and rratio <= 0.7, ("replica", kind, rwins, rratio)
        assert wins >= 8 and ratio <= 0.7, (kind, wins, ratio, err, rep)


# ------------------------------------------------------------------------------------------------------------------ 7: errors
def test_errors_are_refused():
    L = dvo.lib()
    import ctypes as C
    bt = dvo.Batch(2, KH, SIZE[0], SIZE[1], LEVELS, CULLS, cfg=tb.cfg())
    RC = dvo.RobustConfig
    sz = C.sizeof(RC)
    bad = [RC(sz, 3, ADAPTIVE, 1.0, 1e-3), RC(sz, -1, ADAPTIVE, 1.0, 1e-3), RC(sz, HUBER, 2, 1.0, 1e-3), RC(sz, HUBER, -1, 1.0, 1e-3),
           RC(sz, HUBER, ADAPTIVE, 0.0, 1e-3), RC(sz, HUBER, ADAPTIVE, -1.0, 1e-3), RC(sz, STUDENT, ADAPTIVE, float("nan"), 1e-3),
           RC(sz, STUDENT, ADAPTIVE, float("inf"), 1e-3), RC(sz, HUBER, ADAPTIVE, 1.0, 0.0), RC(sz, HUBER, ADAPTIVE, 1.0, float("nan")),
           RC(sz, HUBER, ADAPTIVE, 1.0, float("inf")), RC(sz - 4, HUBER, ADAPTIVE, 1.0, 1e-3), RC(0, HUBER, ADAPTIVE, 1.0, 1e-3)]
    for c in bad:
        assert L.dvo_batch_set_robust_weights(bt._p, C.byref(c)) == dvo.DVO_ERR_BAD_ARGUMENT, (c.struct_size, c.kind, c.scale_mode, c.param, c.scale_floor)
    rows = np.ones(2, np.float32)
    with pytest.raises(dvo.DvoError):
        bt.set_robust_scales(rows)                  # weights are off
    with pytest.raises(dvo.DvoError):
        bt.last_robust_scales()                     # nothing pushed
    bt.set_robust_weights(**tb.rob(HUBER, ADAPTIVE))
    with pytest.raises(dvo.DvoError):
        bt.set_robust_scales(rows)                  # rows outside the GIVEN mode
    bt.set_robust_scales(None)                      # clearing is always allowed
    assert L.dvo_batch_last_robust_scales(bt._p, None) == dvo.DVO_ERR_BAD_ARGUMENT
    bt.set_robust_weights(None)
    g, d, s = tb.frames()
    t = [tb.dev(x[:2]) for x in (g, d, s)]
    bt.push_device(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr())
    with pytest.raises(dvo.DvoError):
        bt.last_robust_scales()                     # the push ran without weights
    assert L.dvo_batch_set_robust_weights(bt._p, C.byref(RC(sz, HUBER, GIVEN, 1.345, 0.0))) == dvo.DVO_ERR_BAD_ARGUMENT
    bt.set_robust_weights(**tb.rob(HUBER, GIVEN))
    with pytest.raises(dvo.DvoError):
        bt.last_robust_scales()                     # enabled from the next push on
    bt.set_robust_scales(np.float32([0.05, 0.02]))
    t2 = [tb.dev(x[1:3]) for x in (g, d, s)]
    bt.push_device(t2[0].data_ptr(), t2[1].data_ptr(), t2[2].data_ptr())
    np.testing.assert_array_equal(bt.last_robust_scales(), np.float32([0.05, 0.02]) * np.float32([0.05, 0.02]))
    bt.close()


def test_zz_report_reduction_bound_ratios():
    """last in the file: under -s, the largest error / bound ratio of every weighted comparison of this process"""
    gn_sums.report("test_gpu_robust")
    assert all(r <= 1.0 for _, r in gn_sums.RATIOS)
