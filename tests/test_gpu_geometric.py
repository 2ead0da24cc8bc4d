"""The geometric (depth) term of a sensor-depth batch (dvo_batch_set_geometric, include/dvo.h) on the GPU.

Set-and-cleared is today's bits; the operator with weight 0 is the plain operator on the tracked frame's own depth, bit for bit; the
operator and every logged iteration of a batch match the contract restated in numpy on the oracle's per-pixel terms
(tests/geometric_ref.py): n_valid and n_geo are EQUAL, every sum is inside the reduction bound, the logged update solves the replayed
combined normal equations; holes, NaN, +inf and steps in the reference depth take geometric rows away and nothing else; the schedules
give the same records; sequences that did not track have a zero record and an empty log; every refusal is returned; and on a weakly
textured pair with sensor noise the default config beats the plain batch.

The shapes are tests/term_batch.py's (its fixture and driver are shared): 320x240 frames, 3 levels, culls 1, crop off, 4 pixels per thread --
levels 40x30 and 80x60 (raster tiles) and 160x120 (32-column 2-D tiles), border queues live on all three -- one case at 328x248 (a
raster finest level), B = 5, and B = 17 for a solve workgroup boundary and two sub-batches.  Every instantiated (PPT, G, T2D, cam)
kernel instance runs once on a batch of two."""
import ctypes as C

import numpy as np
import pytest

import dvo_amd as dvo
import geometric_ref as gr
import gn_sums
import term_batch as tb
from term_batch import BAD, CULLS, D_LENS, F32, GEO, KH, LEVELS, SIZE, SKIP, SKIPPED, RESTART, STARTED, TOP, TRACKED

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _oracle_steps():
    with tb.oracle_steps():
        yield


def _wp(cfg=None):
    return gr.weight_params(cfg if cfg is not None else tb.cfg())


def _term(geo, clear=False):
    """run() keywords of a batch with the geometric term.  geo: set_geometric arguments (clear: set, then turned off before the first push)"""
    def setup(bt, keep):
        bt.set_geometric(**geo)
        if clear:
            bt.set_geometric(dvo.GEOMETRIC_OFF)
    return dict(setup=setup, reads=() if clear else ("geometric",))


def _depth_maps(idx, size, ref_depth):
    """maps of run(): ref_depth(k, b, depth) replaces a pushed depth map"""
    frame = tb.frame_maps(idx, size)

    def maps(k, b):
        g, d, s = frame(k, b)
        return g, ref_depth(k, b, d.copy()), s
    return maps if ref_depth is not None else None


# ------------------------------------------------------------------------------------------------------------------ 1: off is today
@pytest.mark.parametrize("mode", ["plain", "actions", "keyframes"])
def test_set_and_cleared_is_never_set(mode):
    kw = dict(acts=tb.acts(5, 3, 3) if mode == "actions" else None, kf=mode == "keyframes")
    cfg = tb.cfg(keyframe_max_frames=2) if mode == "keyframes" else tb.cfg()
    tb.same(tb.run(cfg, 5, tb.wide_idx(5), **kw), tb.run(cfg, 5, tb.wide_idx(5), **_term(GEO, clear=True), **kw), families=())


# ------------------------------------------------------------------------------------------------------------------ 2, 3: the operator
@pytest.fixture(scope="module")
def geo_run():
    """three sequences with the default config: the poses the operator tests evaluate at"""
    return tb.run(tb.cfg(), 3, tb.wide_idx(3), **_term(GEO))


def test_operator_with_weight_zero_is_the_plain_operator_on_own_depth(geo_run):
    cfg = tb.cfg()
    obj, ref = tb.oframe_of(geo_run[1]["maps"][0]), tb.oframe_of(geo_run[0]["maps"][0])
    poses = tb.level_poses(geo_run[1]["logs"][0])
    for l in range(LEVELS):
        got = dvo.op_gn_step_geometric(obj.gray(l), obj.depth(l), obj.sigma(l), ref.gray(l), ref.depth(l), ref.K(l), poses[l], l, 0.0, 0.1, cfg=cfg)
        p = dvo.optimize(obj.gray(l), ref.gray(l), obj.depth(l), obj.sigma(l), ref.K(l), poses[l], l, cfg=cfg)
        assert got["n_valid"] == p["n_valid"] > 500 and got["sum_r2"] == p["sum_r2"], l
        assert np.array_equal(got["H"], p["H"]) and np.array_equal(got["g"], p["g"]), l
        assert got["xi_update"].tobytes() == p["xi_update"].tobytes() and F32(got["residual"]).tobytes() == F32(p["residual"]).tobytes(), l
        assert got["n_geo"] > 0.5 * got["n_valid"] and got["sum_sq"] == 0.0, l


def test_operator_matches_the_contract(geo_run):
    cfg = tb.cfg()
    before = gr.nonempty_calls()
    obj, ref = tb.oframe_of(geo_run[1]["maps"][0]), tb.oframe_of(geo_run[0]["maps"][0])
    poses = tb.level_poses(geo_run[1]["logs"][0])
    at = gr.frame_pixels(obj, ref, False, _wp())
    n = cut = 0
    for l in range(LEVELS):
        for xi in (poses[l], np.zeros(6, F32)):    # the logged pose (nearly converged: small rz) and the start pose (rz of the whole motion)
            px = at(l, xi)
            assert px["n_valid"] > 500
            n_geo = {}
            for weight in (0.0, 1.0, 10.0):
                for max_diff in (0.1, 0.001):
                    got = dvo.op_gn_step_geometric(obj.gray(l), obj.depth(l), obj.sigma(l), ref.gray(l), ref.depth(l), ref.K(l), xi, l, weight, max_diff, cfg=cfg)
                    ex = gr.assert_step(got, px, weight, max_diff, tag="operator level %d weight %g max_diff %g" % (l, weight, max_diff))
                    assert F32(got["residual"]) == F32(got["sum_r2"]) / F32(got["n_valid"])
                    n_geo[max_diff] = ex["n_geo"]
                    n += 1
            assert 0 < n_geo[0.001] <= n_geo[0.1], (l, n_geo)
            cut += n_geo[0.001] < n_geo[0.1]
    assert cut >= LEVELS, "the smaller gate should take rows away at the start pose of every level"
    assert gr.nonempty_calls() == before + n


# ------------------------------------------------------------------------------------------------------------------ 4: replay
def _empty(o, b):
    gl = o["glogs"][b]
    return o["grec"][b]["n_geo"] == 0 and o["grec"][b]["mean_sq"] == 0 and not gl["n_iter"].any() and not gl["n_geo"].any() and not gl["sum_sq"].any()


def _check_sequence(o, b, obj, ref, geo, cfg, ppt, where):
    """one TRACKED sequence of one push: every logged iteration against the contract, last_geometric, the finest level's record"""
    lg, gl = o["logs"][b], o["glogs"][b]
    ex, n_it = gr.replay_call(lg, gl, gr.frame_pixels(obj, ref, False, _wp(cfg)), LEVELS, geo["weight"], geo["max_diff"], ppt=ppt, tag=where)
    it = int(lg["n_iter"][TOP]) - 1
    ppt = gn_sums.at_level(ppt, TOP)   # (from here on: the finest level's record)
    rec = o["grec"][b]
    assert int(rec["n_geo"]) == ex["n_geo"] == int(gl["n_geo"][TOP][it]), (where, rec, ex["n_geo"])
    if ex["n_geo"] > 0:
        fS = gr.depths(ppt)[2] * gn_sums.U32 * gn_sums.SECOND_ORDER
        want = ex["S29"] / ex["n_geo"]
        assert abs(float(rec["mean_sq"]) - want) <= fS * want + float(np.spacing(F32(rec["mean_sq"]))), (where, rec, want)
    q = o["q"][b]
    assert q["status"] == TRACKED and q["n_valid"] == int(lg["n_valid"][TOP][it]) == ex["n"], where
    assert F32(q["residual"]).tobytes() == F32(lg["residual"][TOP][it]).tobytes(), where
    # the finest level's record holds the combined sums of its last iteration
    gr.assert_exact(dict(H=q["H"], g=q["g"], sum_r2=q["sum_r2"], n_valid=q["n_valid"], n_geo=rec["n_geo"], sum_sq=float(gl["sum_sq"][TOP][it]),
                         sum_sq_is_float=True), ex, ppt, where + " record")
    return n_it, ex


def _replay(cfg, B, geo, acts=None, kf=False, cams=None, size=SIZE, outs=None, min_tracked=None, cams_at=None, ref_depth=None, feed="device",
            D=None, ppt=4, seqs=None, frame_of=None):
    idx = tb.wide_idx(B)
    if outs is None:
        outs = tb.run(cfg, B, idx, acts=acts, kf=kf, cams=cams, size=size, cams_at=cams_at, feed=feed, D=D, maps=_depth_maps(idx, size, ref_depth),
                      **_term(geo))
    before = gr.nonempty_calls()
    frame_of = frame_of or tb.oframe_of

    def check(k, b, kr, o, K):
        return _check_sequence(o, b, frame_of(o["maps"][b], K), frame_of(outs[kr]["maps"][b], K), geo, cfg, ppt, "push %d seq %d of %d" % (k, b, B))[0]
    # (SKIPPED / STARTED / BAD_ACTION: a zero record and an empty log)
    _, n_it = tb.walk(outs, B, check, _empty, kf=kf, cams=cams, cams_at=cams_at, seqs=seqs, min_tracked=min_tracked)
    assert gr.nonempty_calls() >= before + n_it // 2   # (the helper really ran: iterations with geometric rows replayed)
    return outs


@pytest.mark.parametrize("B", [5, 17])
def test_replay(B):
    """B = 17: k_gn_solve_z takes 8 sequences per workgroup, so the third workgroup holds one"""
    _replay(tb.cfg(), B, GEO, seqs=None if B == 5 else (0, 7, 8, 15, 16))


def test_replay_raster_finest_level():
    _replay(tb.cfg(), 5, GEO, size=(328, 248), seqs=(0, 3))


def test_replay_other_weight_and_gate():
    _replay(tb.cfg(), 5, dict(weight=1.0, max_diff=0.01), seqs=(1, 4))


def test_replay_keyframes():
    _replay(tb.cfg(keyframe_max_frames=2), 5, GEO, kf=True)


def test_replay_per_sequence_intrinsics():
    _replay(tb.cfg(), 5, GEO, cams=tb.sequence_cams(5))


def test_replay_sensor_undistortion():
    """the frames the batch tracks are dvo_op_undistort of the pushed maps (tests/test_gpu_sensor_undistort.py holds that equality)"""
    und = lambda m, K: tb.oframe_of(tuple(dvo.undistort(x, K, D_LENS) for x in m), K)
    _replay(tb.cfg(), 5, GEO, D=D_LENS, seqs=(0, 2), frame_of=und)


def test_replay_raw_feed():
    """raw frames: the maps are dvo_op_ingest of the u8 / u16 frames, and every contributing pixel carries the one weight of sigma 0.1"""
    raw = lambda m, K: tb.oframe_of(dvo.ingest(*tb.raw_of(m)), K)
    a = _replay(tb.cfg(), 5, GEO, feed="raw", seqs=(0, 3), frame_of=raw)
    tb.same(a, tb.run(tb.cfg(), 5, tb.wide_idx(5), feed="raw_host", **_term(GEO)))


@pytest.mark.parametrize("cam", [False, True])
@pytest.mark.parametrize("ppt,group", [(1, 1), (2, 1), (2, 2), (4, 1), (4, 2), (4, 4), (8, 1), (8, 2), (8, 4)])
def test_every_kernel_instance(ppt, group, cam):
    """each (PPT, G) pair of k_track_gn_z and k_track_gn_z_cam on a batch of two: the 160x120 level takes the 2-D tiles of PPT = 4, the
    two coarser levels the raster tiles"""
    cfg = tb.cfg(gn_gather_group=group)
    cfg.gn_pixels_per_thread = ppt    # (_cfg fixes 4 pixels per thread)
    cams = np.stack([KH, KH]).astype(F32) if cam else None
    if cam:
        cams[1, 0, 0] *= 1.01
    _replay(cfg, 2, GEO, cams=cams, ppt=ppt, seqs=(1,))


# ------------------------------------------------------------------------------------------------------------------ 5: the gates
@pytest.mark.parametrize("defect", ["hole", "nan", "inf", "step"])
def test_gates_of_the_reference_depth(defect, geo_run):
    """A block of the reference's depth is a hole (zeros), NaN, +inf or a step of 0.5 m (> max_diff): at every level n_geo equals the
    replica's and is below the clean reference's by about the block, n_valid and sum_r2 are the clean ones, every sum is finite."""
    cfg = tb.cfg()
    before = gr.nonempty_calls()
    obj, ref = tb.oframe_of(geo_run[1]["maps"][0]), tb.oframe_of(geo_run[0]["maps"][0])
    poses = tb.level_poses(geo_run[1]["logs"][0])
    for l in range(LEVELS):
        bad = ref.depth(l).copy()
        n_blk = tb.defect(bad, defect)
        clean = dvo.op_gn_step_geometric(obj.gray(l), obj.depth(l), obj.sigma(l), ref.gray(l), ref.depth(l), ref.K(l), poses[l], l, 10.0, 0.1, cfg=cfg)
        got = dvo.op_gn_step_geometric(obj.gray(l), obj.depth(l), obj.sigma(l), ref.gray(l), bad, ref.K(l), poses[l], l, 10.0, 0.1, cfg=cfg)
        px = gr.pixels(obj.gray(l), obj.depth(l), obj.sigma(l), ref.gray(l), bad, ref.K(l), poses[l], l, False, _wp())
        gr.assert_step(got, px, 10.0, 0.1, tag="gate %s level %d" % (defect, l))
        assert got["n_valid"] == clean["n_valid"] and got["sum_r2"] == clean["sum_r2"], (defect, l)
        assert got["n_geo"] < clean["n_geo"] - n_blk // 2, (defect, l, got["n_geo"], clean["n_geo"], n_blk)
        assert np.isfinite(got["H"]).all() and np.isfinite(got["g"]).all() and np.isfinite(got["sum_sq"]) and np.isfinite(got["xi_update"]).all()
    assert gr.nonempty_calls() == before + LEVELS


@pytest.mark.parametrize("defect", ["hole", "step"])
def test_gates_in_a_batch(defect):
    """the same defects in the frames a batch is given (every push, so in the tracked frame's own depth as well): the replay holds"""
    def ref_depth(k, b, d):
        tb.defect(d, defect)
        return d
    _replay(tb.cfg(), 5, GEO, ref_depth=ref_depth, seqs=(0, 2))


# ------------------------------------------------------------------------------------------------------------------ 6: the schedules
@pytest.fixture(scope="module")
def base5():
    return tb.run(tb.cfg(), 5, tb.wide_idx(5), **_term(GEO))


@pytest.mark.parametrize("variant", ["adaptive_off", "fused_tiles", "single_launch", "host_feed"])
def test_schedule_variants_give_the_same_records(variant, base5):
    other = tb.run(tb.cfg(**tb.SCHEDULE_VARIANTS.get(variant, {})), 5, tb.wide_idx(5), feed="host" if variant == "host_feed" else "device",
                   **_term(GEO))
    tb.same(base5, other)
    assert all((o["grec"]["n_geo"] > 1000).all() for o in base5[1:])


def test_two_streams():
    """two sub-batches need more than 16 sequences (17: not a multiple of 8 either); the depth base, the record and the log are offset
    per sub-batch"""
    one = tb.run(tb.cfg(), 17, tb.wide_idx(17), **_term(GEO))
    two = tb.run(tb.cfg(track_streams=2), 17, tb.wide_idx(17), **_term(GEO))
    tb.same(one, two)
    assert all((o["grec"]["n_geo"] > 1000).all() for o in one[1:])


# ------------------------------------------------------------------------------------------------------------------ 7: lifecycle
def test_actions_leave_no_stale_record():
    """SKIP, RESTART and a bad action give a zero record and an empty log (checked in _replay); the tracked ones replay"""
    acts = tb.acts(5, 3, 9)
    assert (acts[1:] == SKIP).any() and (acts[1:] == RESTART).any()
    acts[2][1] = 7   # an action outside the set: BAD_ACTION, handled as SKIP
    outs = _replay(tb.cfg(), 5, GEO, acts=acts, min_tracked=3)
    assert outs[2]["status"][1] == BAD and (np.concatenate([o["status"] for o in outs]) == SKIPPED).any()


def test_camera_change_restarts_the_sequence():
    cams = np.stack([KH] * 5).astype(F32)
    new = cams.copy()
    new[2, 0, 0] *= 1.02
    outs = _replay(tb.cfg(), 5, GEO, cams=cams, cams_at=(2, new), min_tracked=8)
    assert outs[2]["status"][2] == STARTED and (outs[2]["status"][[0, 1, 3, 4]] == TRACKED).all()


# ------------------------------------------------------------------------------------------------------------------ 8: refusals
def test_errors_are_refused():
    L = dvo.lib()
    bt = dvo.Batch(2, KH, SIZE[0], SIZE[1], LEVELS, CULLS, cfg=tb.cfg())
    GC = dvo.GeometricConfig
    sz = C.sizeof(GC)
    bad = [GC(sz, 2, 10.0, 0.1), GC(sz, -1, 10.0, 0.1), GC(sz, 1, -1.0, 0.1), GC(sz, 1, float("nan"), 0.1), GC(sz, 1, float("inf"), 0.1),
           GC(sz, 1, 10.0, 0.0), GC(sz, 1, 10.0, -0.1), GC(sz, 1, 10.0, float("nan")), GC(sz, 1, 10.0, float("inf")), GC(sz - 4, 1, 10.0, 0.1),
           GC(0, 1, 10.0, 0.1)]
    for c in bad:
        assert L.dvo_batch_set_geometric(bt._p, C.byref(c)) == dvo.DVO_ERR_BAD_ARGUMENT, (c.struct_size, c.mode, c.weight, c.max_diff)
    assert L.dvo_batch_set_geometric(bt._p, C.byref(GC(sz, 1, 0.0, 0.1))) == 0       # weight 0 is allowed
    bt.set_geometric(None)
    with pytest.raises(dvo.DvoError):
        bt.last_geometric()                         # nothing pushed
    with pytest.raises(dvo.DvoError):
        bt.last_geometric_log(0)
    # robust weights or affine compensation on, in either order of the two calls
    bt.set_robust_weights(dvo.ROBUST_HUBER, param=1.345, scale_mode=dvo.ROBUST_SCALE_ADAPTIVE, scale_floor=1e-3)
    with pytest.raises(dvo.DvoError):
        bt.set_geometric(**GEO)
    bt.set_robust_weights(dvo.ROBUST_NONE)
    bt.set_affine_brightness(dvo.AFFINE_ESTIMATE)
    with pytest.raises(dvo.DvoError):
        bt.set_geometric(**GEO)
    bt.set_geometric(dvo.GEOMETRIC_OFF)             # turning it off is always allowed
    bt.set_affine_brightness(None)
    bt.set_geometric(**GEO)
    with pytest.raises(dvo.DvoError):
        bt.set_robust_weights(dvo.ROBUST_HUBER, param=1.345, scale_mode=dvo.ROBUST_SCALE_ADAPTIVE, scale_floor=1e-3)
    with pytest.raises(dvo.DvoError):
        bt.set_affine_brightness(dvo.AFFINE_ESTIMATE)
    bt.set_robust_weights(dvo.ROBUST_NONE)          # (turning the others off stays allowed)
    bt.set_affine_brightness(None)
    assert L.dvo_batch_last_geometric(bt._p, None) == dvo.DVO_ERR_BAD_ARGUMENT
    lg = dvo.GeometricLog()
    assert L.dvo_batch_last_geometric_log(bt._p, 0, C.byref(lg)) == dvo.DVO_ERR_BAD_ARGUMENT    # struct_size not set
    bt.set_geometric(None)
    g, d, s = tb.frames()
    t = [tb.dev(x[:2]) for x in (g, d, s)]
    bt.push_device(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr())
    with pytest.raises(dvo.DvoError):
        bt.last_geometric()                         # the push ran without the feature
    bt.set_geometric(**GEO)
    with pytest.raises(dvo.DvoError):
        bt.last_geometric()                         # enabled from the next push on
    t2 = [tb.dev(x[1:3]) for x in (g, d, s)]
    bt.push_device(t2[0].data_ptr(), t2[1].data_ptr(), t2[2].data_ptr())
    assert (bt.last_geometric()["n_geo"] > 1000).all()
    with pytest.raises(dvo.DvoError):
        bt.last_geometric_log(2)                    # seq out of range
    bt.close()
    # a mono handle
    from util import K640
    mb = dvo.MonoBatch(2, K640, 640, 480, cfg=dvo.default_config(rng_seed=3))
    c = dvo.geometric_default_config()
    assert L.dvo_batch_set_geometric(mb._p, C.byref(c)) == dvo.DVO_ERR_BAD_ARGUMENT
    assert L.dvo_batch_set_geometric(mb._p, None) == dvo.DVO_ERR_BAD_ARGUMENT
    rec = (dvo.GeometricRecord * 2)()
    assert L.dvo_batch_last_geometric(mb._p, rec) == dvo.DVO_ERR_NOT_READY
    mb.close()


# ------------------------------------------------------------------------------------------------------------------ 9: it helps
# The numpy replica of the contract on the oracle (geometric_ref.geometric_track on geometric_ref.outcome_pair): with
# the default config it is closer to the true motion than orc.track in 4 of 4 cases, summed error 0.001464 against 0.2419; the cap on
# the GPU's ratio is the midpoint between that ratio and 1 (plain's own error varies by tens of percent from seed to seed)
REPLICA_WINS = (True, True, True, True)
REPLICA_RATIO = 0.00605
OUTCOME_CAP = 0.5 * (REPLICA_RATIO + 1.0)


def test_default_config_beats_plain_on_a_weakly_textured_pair():
    """Gray contrast 0.1, gray noise 0.01, depth noise 0.002 z^2, motion 0.03 / 1.0 deg, four seeds: frame 1 tracked against frame 0,
    one batch of four sequences per estimator.  The geometric batch must win wherever the replica wins and its summed error must be at
    most OUTCOME_CAP times plain's."""
    o = gr.OUTCOME
    cfg = dvo.default_config(gn_pixels_per_thread=4, crop_enable=0, step_default=o["steps"][0], step_level1=o["steps"][1], step_level2=o["steps"][2],
                             min_residual=o["min_residual"], min_update=o["min_update"], max_iterations=o["max_iterations"])
    pairs = [gr.outcome_pair(seed) for seed in o["seeds"]]
    B = len(pairs)
    K = pairs[0][3]
    err = {}
    for on in (False, True):
        bt = dvo.Batch(B, K, o["width"], o["height"], o["levels"], o["culls"], cfg=cfg)
        if on:
            c = dvo.geometric_default_config()
            bt.set_geometric(c.mode, c.weight, c.max_diff)
        for k in (0, 1):
            t = [tb.dev(np.stack([p[j][k] for p in pairs])) for j in (0, 1, 2)]
            bt.push_device(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr())
            bt.synchronize()
        xi, _ = bt.last_poses()
        if on:
            assert (bt.last_geometric()["n_geo"] > 10000).all()
        bt.close()
        err[on] = np.array([gr.pose_error(xi[b], pairs[b][4]) for b in range(B)])
    wins = err[True] < err[False]
    ratio = err[True].sum() / err[False].sum()
    print("\ngeometric: GPU wins %s, summed error %.4g against plain %.4g, ratio %.4f (replica %.4f, cap %.3f)"
          % (wins.tolist(), err[True].sum(), err[False].sum(), ratio, REPLICA_RATIO, OUTCOME_CAP))
    assert all(w or not r for w, r in zip(wins, REPLICA_WINS)) and ratio <= OUTCOME_CAP, (wins, ratio, err)


def test_zz_report_reduction_bound_ratios():
    """last in the file: under -s, the largest error / bound ratio of every comparison of this process"""
    gn_sums.report("test_gpu_geometric")
    assert all(r <= 1.0 for _, r in gn_sums.RATIOS)
