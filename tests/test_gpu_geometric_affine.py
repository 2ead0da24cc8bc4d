"""The geometric term composed with affine brightness compensation (dvo_batch_set_geometric_affine, include/dvo.h) on
the GPU.

The identity entry gives the geometric batch's bits; the operator with weight 0 is the affine operator on the tracked frame's own
depth and with (a, b) = (1, 0) the geometric operator, bit for bit; the operator and every logged iteration of a composed batch match
the contract restated on the oracle's per-pixel terms (tests/geometric_affine_ref.py): n_valid and n_geo are EQUAL, every sum and
moment is inside its reduction bound, the logged update solves the replayed combined normal equations and every entry is the closed
form of the moments of the iteration before it inside the propagated bound; defects of the reference depth take geometric rows away
and nothing else; the schedules give the same records and logs; sequences that did not track have zero records and empty logs;
turning one term off leaves the other family's batch; every refusal is returned; and under an exposure change on a weakly textured
pair the composed batch beats the geometric one.

The shapes are tests/term_batch.py's (its fixture and driver are shared): 320x240 frames, 3 levels, culls 1, crop off, 4 pixels per thread --
levels 40x30 and 80x60 (raster tiles) and 160x120 (32-column 2-D tiles), border queues live on all three -- one case at 328x248 (a
raster finest level), B = 5, and B = 17 for a solve workgroup boundary and two sub-batches.  The frames a batch sees carry an exposure
change per push and sequence (tests/term_batch.py's EXPO), so that the entries are far from (1, 0).  Every instantiated (PPT, G,
T2D, cam) kernel instance runs once on a batch of two."""
import ctypes as C

import numpy as np
import pytest

import dvo_amd as dvo
import geometric_affine_ref as ga
import geometric_ref as gr
import gn_sums
import term_batch as tb
from term_batch import BAD, CULLS, D_LENS, F32, GEO, KH, LEVELS, SIZE, SKIP, SKIPPED, RESTART, STARTED, TOP, TRACKED

pytestmark = pytest.mark.gpu

ESTIMATE, GIVEN = dvo.AFFINE_ESTIMATE, dvo.AFFINE_GIVEN


@pytest.fixture(scope="module", autouse=True)
def _oracle_steps():
    with tb.oracle_steps():
        yield


def _wp(cfg=None):
    return gr.weight_params(cfg if cfg is not None else tb.cfg())


def _zab(mode=ESTIMATE, rows=None, **geo):
    """setup of a composed batch"""
    geo = geo or GEO

    def setup(bt, keep):
        bt.set_geometric_affine(affine_mode=mode, **geo)
        if rows is not None:
            bt.set_affine_rows(rows)
    return setup


def _z(bt, keep):
    bt.set_geometric(**GEO)


def _ab(bt, keep):
    bt.set_affine_brightness(ESTIMATE)


def _term(idx, setup, reads=("geometric", "affine"), size=SIZE, ref_depth=None):
    """run() keywords of a batch with the terms of setup, whose records are read after every push: the gray it is given is under the
    exposure of the push and sequence; ref_depth(k, b, depth) replaces a pushed depth map"""
    g, d, s = tb.frames(size)

    def maps(k, b):
        i = idx[k][b]
        return tb.expose(g[i], k, b), d[i] if ref_depth is None else ref_depth(k, b, d[i].copy()), s[i]
    return dict(setup=setup, reads=reads, maps=maps)


# ------------------------------------------------------------------------------------------------------------------ 1: identity is geometric
@pytest.mark.parametrize("variant", ["no_rows", "ones"])
def test_identity_entry_is_the_geometric_batch(variant):
    B = 5
    idx = tb.wide_idx(B)
    rows = np.tile(F32([1.0, 0.0]), (B, 1)) if variant == "ones" else None
    geo = tb.run(tb.cfg(), B, idx, **_term(idx, _z, reads=("geometric",)))
    got = tb.run(tb.cfg(), B, idx, **_term(idx, _zab(GIVEN, rows)))
    tb.same(geo, got, families=("geometric",))
    assert all((o["grec"]["n_geo"] > 1000).all() for o in got[1:])
    for o in got[1:]:
        np.testing.assert_array_equal(o["ab"], np.tile(F32([1.0, 0.0]), (B, 1)))
        for al in o["alogs"]:
            n = [int(x) for x in al["n_iter"][:LEVELS]]
            assert min(n) >= 1 and all((al["a"][l][:n[l]] == 1).all() and not al["b"][l][:n[l]].any() for l in range(LEVELS))
            assert al["prime_a"] == 0 and al["prime_b"] == 0
    assert not got[0]["ab"].any() and not got[0]["grec"]["n_geo"].any()   # nothing tracked at the first push


# ------------------------------------------------------------------------------------------------------------------ 2, 3, 4: the operator
@pytest.fixture(scope="module")
def zab_run():
    """three sequences with the default config, ESTIMATE: the poses the operator tests evaluate at"""
    return tb.run(tb.cfg(), 3, tb.wide_idx(3), **_term(tb.wide_idx(3), _zab()))


def _op(obj, ref, l, xi, weight, max_diff, a, b, cfg, ref_depth=None):
    return dvo.op_gn_step_geometric_affine(obj.gray(l), obj.depth(l), obj.sigma(l), ref.gray(l), ref.depth(l) if ref_depth is None else ref_depth,
                                           ref.K(l), xi, l, weight, max_diff, a, b, cfg=cfg)


def _same_result(got, p, where):
    assert got["n_valid"] == p["n_valid"] > 500 and got["sum_r2"] == p["sum_r2"], where
    assert np.array_equal(got["H"], p["H"]) and np.array_equal(got["g"], p["g"]), where
    assert got["xi_update"].tobytes() == p["xi_update"].tobytes() and got["xi_next"].tobytes() == p["xi_next"].tobytes(), where
    assert F32(got["residual"]).tobytes() == F32(p["residual"]).tobytes(), where


def test_operator_with_weight_zero_is_the_affine_operator_on_own_depth(zab_run):
    cfg = tb.cfg()
    obj, ref = tb.oframe_of(zab_run[1]["maps"][0]), tb.oframe_of(zab_run[0]["maps"][0])
    poses = tb.level_poses(zab_run[1]["logs"][0])
    for l in range(LEVELS):
        for a, b in ((0.9, 0.03), (1.2, -0.05)):
            got = _op(obj, ref, l, poses[l], 0.0, 0.1, a, b, cfg)
            p = dvo.op_gn_step_affine(obj.gray(l), ref.gray(l), obj.depth(l), obj.sigma(l), ref.K(l), poses[l], l, a, b, cfg=cfg)
            _same_result(got, p, (l, a, b))
            assert got["moments"].tobytes() == p["moments"].tobytes() and got["next_ab"].tobytes() == p["next_ab"].tobytes(), (l, a, b)
            assert got["moments"][0] == got["n_valid"] and got["n_geo"] > 0.5 * got["n_valid"] and got["sum_sq"] == 0.0, (l, a, b)


def test_operator_with_the_identity_entry_is_the_geometric_operator(zab_run):
    cfg = tb.cfg()
    obj, ref = tb.oframe_of(zab_run[1]["maps"][0]), tb.oframe_of(zab_run[0]["maps"][0])
    poses = tb.level_poses(zab_run[1]["logs"][0])
    for l in range(LEVELS):
        for weight, max_diff in ((10.0, 0.1), (1.0, 0.001)):
            got = _op(obj, ref, l, poses[l], weight, max_diff, 1.0, 0.0, cfg)
            p = dvo.op_gn_step_geometric(obj.gray(l), obj.depth(l), obj.sigma(l), ref.gray(l), ref.depth(l), ref.K(l), poses[l], l, weight, max_diff, cfg=cfg)
            _same_result(got, p, (l, weight, max_diff))
            assert got["n_geo"] == p["n_geo"] > 0 and got["sum_sq"] == p["sum_sq"] > 0.0, (l, weight, max_diff)


@pytest.mark.parametrize("entry", ["0.9_0.03", "1.2_-0.05", "guard"])
def test_operator_matches_the_contract(entry, zab_run):
    """guard: the tracked frame's gray is one value, so det = 0 fails the contrast guard and the next entry is the entry given"""
    cfg = tb.cfg()
    before = ga.nonempty_calls()
    mo = zab_run[1]["maps"][0]
    if entry == "guard":
        a, b = 1.1, 0.02
        mo = (np.full_like(mo[0], 0.5), mo[1], mo[2])
    else:
        a, b = (float(v) for v in entry.split("_"))
    obj, ref = tb.oframe_of(mo), tb.oframe_of(zab_run[0]["maps"][0])
    poses = tb.level_poses(zab_run[1]["logs"][0])
    at = ga.frame_pixels(obj, ref, False, _wp())
    n = 0
    for l in range(LEVELS):
        for xi in (poses[l], np.zeros(6, F32)):    # the logged pose of a real run and the start pose
            px = at(l, xi)
            assert px["n_valid"] > 500
            for weight in (0.0, 1.0, 10.0):
                for max_diff in (0.1, 0.001):
                    got = _op(obj, ref, l, xi, weight, max_diff, a, b, cfg)
                    ex = ga.assert_step(got, px, weight, max_diff, a, b, tag="operator level %d weight %g max_diff %g entry %s" % (l, weight, max_diff, entry))
                    assert F32(got["residual"]) == F32(got["sum_r2"]) / F32(got["n_valid"]) and ex["n_geo"] > 0
                    if entry == "guard":
                        assert got["next_ab"].tobytes() == F32([a, b]).tobytes()
                    else:
                        assert got["next_ab"].tobytes() != F32([a, b]).tobytes()
                    n += 1
    assert ga.nonempty_calls() == before + n


# ------------------------------------------------------------------------------------------------------------------ 5: replay
def _empty(o, b):
    gl, al = o["glogs"][b], o["alogs"][b]
    return (o["grec"][b]["n_geo"] == 0 and o["grec"][b]["mean_sq"] == 0 and not gl["n_iter"].any() and not gl["n_geo"].any() and not gl["sum_sq"].any()
            and not o["ab"][b].any() and not al["n_iter"].any() and not al["a"].any() and not al["b"].any() and al["prime_a"] == 0 and al["prime_b"] == 0)


def _check_sequence(o, b, obj, ref, geo, mode, given, cfg, ppt, where):
    """one TRACKED sequence of one push: every logged iteration against the contract, both records, the finest level's quality record"""
    lg, gl, al = o["logs"][b], o["glogs"][b], o["alogs"][b]
    (ex, ab), n_it = ga.replay_call(lg, gl, al, ga.frame_pixels(obj, ref, False, _wp(cfg)), LEVELS, geo["weight"], geo["max_diff"], mode,
                                    given_ab=None if given is None else given[b], ppt=ppt, tag=where)
    it = int(lg["n_iter"][TOP]) - 1
    ppt = gn_sums.at_level(ppt, TOP)   # (from here on: the finest level's record)
    assert o["ab"][b].tobytes() == np.array(ab, F32).tobytes(), (where, o["ab"][b], ab)   # the entry the finest level's last iteration used
    rec = o["grec"][b]
    assert int(rec["n_geo"]) == ex["n_geo"] == int(gl["n_geo"][TOP][it]), (where, rec, ex["n_geo"])
    if ex["n_geo"] > 0:
        fS = gr.depths(ppt)[2] * gn_sums.U32 * gn_sums.SECOND_ORDER
        want = ex["S29"] / ex["n_geo"]
        assert abs(float(rec["mean_sq"]) - want) <= fS * want + float(np.spacing(F32(rec["mean_sq"]))), (where, rec, want)
    q = o["q"][b]
    assert q["status"] == TRACKED and q["n_valid"] == int(lg["n_valid"][TOP][it]) == ex["n"], where
    assert F32(q["residual"]).tobytes() == F32(lg["residual"][TOP][it]).tobytes(), where
    gr.assert_exact(dict(H=q["H"], g=q["g"], sum_r2=q["sum_r2"], n_valid=q["n_valid"], n_geo=rec["n_geo"], sum_sq=float(gl["sum_sq"][TOP][it]),
                         sum_sq_is_float=True), ex, ppt, where + " record")
    return n_it


def _replay(cfg, B, mode=ESTIMATE, given=None, geo=GEO, acts=None, kf=False, cams=None, size=SIZE, outs=None, min_tracked=None, cams_at=None,
            ref_depth=None, feed="device", D=None, ppt=4, seqs=None, frame_of=None):
    idx = tb.wide_idx(B)
    if outs is None:
        outs = tb.run(cfg, B, idx, acts=acts, kf=kf, cams=cams, size=size, cams_at=cams_at, feed=feed, D=D,
                      **_term(idx, _zab(mode, given, **geo), size=size, ref_depth=ref_depth))
    before = ga.nonempty_calls()
    frame_of = frame_of or tb.oframe_of

    def check(k, b, kr, o, K):
        return _check_sequence(o, b, frame_of(o["maps"][b], K), frame_of(outs[kr]["maps"][b], K), geo, mode, given, cfg, ppt,
                               "push %d seq %d of %d" % (k, b, B))
    # (SKIPPED / STARTED / BAD_ACTION: zero records and empty logs)
    _, n_it = tb.walk(outs, B, check, _empty, kf=kf, cams=cams, cams_at=cams_at, seqs=seqs, min_tracked=min_tracked)
    assert ga.nonempty_calls() >= before + n_it // 2   # (the helper really ran: iterations with geometric rows replayed)
    return outs


def _rows(B):
    return np.stack([F32([0.85 + 0.05 * b, 0.03 - 0.01 * b]) for b in range(B)])


@pytest.mark.parametrize("mode", ["estimate", "given"])
@pytest.mark.parametrize("B", [5, 17])
def test_replay(B, mode):
    """B = 17: k_gn_solve_zab takes 8 sequences per workgroup, so the third workgroup holds one"""
    seqs = (0, 3) if B == 5 else (7, 8, 16)
    if mode == "estimate":
        outs = _replay(tb.cfg(), B, seqs=seqs)
        assert all(abs(float(o["alogs"][b]["prime_a"]) - 1.0) > 0.02 for o in outs[1:] for b in seqs)   # the exposure change is seen
    else:
        _replay(tb.cfg(), B, GIVEN, _rows(B), seqs=seqs)


def test_replay_raster_finest_level():
    _replay(tb.cfg(), 5, size=(328, 248), seqs=(1,))


def test_replay_keyframes():
    _replay(tb.cfg(keyframe_max_frames=2), 5, kf=True, seqs=(0, 4))


def test_replay_per_sequence_intrinsics():
    _replay(tb.cfg(), 5, GIVEN, _rows(5), cams=tb.sequence_cams(5), seqs=(2, 4))


def test_replay_sensor_undistortion():
    """the frames the batch tracks are dvo_op_undistort of the pushed maps (tests/test_gpu_sensor_undistort.py holds that equality)"""
    und = lambda m, K: tb.oframe_of(tuple(dvo.undistort(x, K, D_LENS) for x in m), K)
    _replay(tb.cfg(), 5, D=D_LENS, seqs=(2,), frame_of=und)


def test_replay_raw_feed():
    """raw frames: the maps are dvo_op_ingest of the u8 / u16 frames, and every contributing pixel carries the one weight of sigma 0.1"""
    raw = lambda m, K: tb.oframe_of(dvo.ingest(*tb.raw_of(m)), K)
    a = _replay(tb.cfg(), 5, feed="raw", seqs=(3,), frame_of=raw)
    tb.same(a, tb.run(tb.cfg(), 5, tb.wide_idx(5), feed="raw_host", **_term(tb.wide_idx(5), _zab())))


# ------------------------------------------------------------------------------------------------------------------ 6: every instance
@pytest.mark.parametrize("cam", [False, True])
@pytest.mark.parametrize("ppt,group", [(1, 1), (2, 1), (2, 2), (4, 1), (4, 2), (4, 4), (8, 1), (8, 2), (8, 4)])
def test_every_kernel_instance(ppt, group, cam):
    """each (PPT, G) pair of k_track_gn_zab and k_track_gn_zab_cam on a batch of two: the 160x120 level takes the 2-D tiles of PPT = 4,
    the two coarser levels the raster tiles"""
    cfg = tb.cfg(gn_gather_group=group)
    cfg.gn_pixels_per_thread = ppt    # (_cfg fixes 4 pixels per thread)
    cams = np.stack([KH, KH]).astype(F32) if cam else None
    if cam:
        cams[1, 0, 0] *= 1.01
    _replay(cfg, 2, cams=cams, ppt=ppt, seqs=(1,))


# ------------------------------------------------------------------------------------------------------------------ 7: the gates
@pytest.mark.parametrize("defect", ["hole", "nan", "inf", "step"])
def test_gates_of_the_reference_depth(defect, zab_run):
    """A block of the reference's depth is a hole (zeros), NaN, +inf or a step of 0.5 m (> max_diff): at every level n_geo equals the
    replica's and is below the clean reference's by about the block; n_valid, sum_r2, the moments and the next entry are the clean
    ones; every sum is finite."""
    cfg = tb.cfg()
    before = ga.nonempty_calls()
    obj, ref = tb.oframe_of(zab_run[1]["maps"][0]), tb.oframe_of(zab_run[0]["maps"][0])
    poses = tb.level_poses(zab_run[1]["logs"][0])
    a, b = 0.9, 0.03
    for l in range(LEVELS):
        bad = ref.depth(l).copy()
        n_blk = tb.defect(bad, defect)
        clean = _op(obj, ref, l, poses[l], 10.0, 0.1, a, b, cfg)
        got = _op(obj, ref, l, poses[l], 10.0, 0.1, a, b, cfg, ref_depth=bad)
        px = ga.pixels(obj.gray(l), obj.depth(l), obj.sigma(l), ref.gray(l), bad, ref.K(l), poses[l], l, False, _wp())
        ga.assert_step(got, px, 10.0, 0.1, a, b, tag="gate %s level %d" % (defect, l))
        assert got["n_valid"] == clean["n_valid"] and got["sum_r2"] == clean["sum_r2"], (defect, l)
        assert got["moments"].tobytes() == clean["moments"].tobytes() and got["next_ab"].tobytes() == clean["next_ab"].tobytes(), (defect, l)
        assert got["n_geo"] < clean["n_geo"] - n_blk // 2, (defect, l, got["n_geo"], clean["n_geo"], n_blk)
        assert np.isfinite(got["H"]).all() and np.isfinite(got["g"]).all() and np.isfinite(got["sum_sq"]) and np.isfinite(got["xi_update"]).all()
        assert np.isfinite(got["moments"]).all() and np.isfinite(got["next_ab"]).all()
    assert ga.nonempty_calls() == before + LEVELS


# ------------------------------------------------------------------------------------------------------------------ 8: the schedules
@pytest.fixture(scope="module")
def base17():
    return tb.run(tb.cfg(), 17, tb.wide_idx(17), **_term(tb.wide_idx(17), _zab()))


@pytest.mark.parametrize("variant", ["adaptive_off", "fused_tiles", "single_launch", "host_feed", "two_streams"])
def test_schedule_variants_give_the_same_records(variant, base17):
    """17 sequences: two sub-batches with track_streams = 2, and a third solve workgroup of one"""
    idx = tb.wide_idx(17)
    other = tb.run(tb.cfg(**tb.SCHEDULE_VARIANTS.get(variant, {})), 17, idx, feed="host" if variant == "host_feed" else "device", **_term(idx, _zab()))
    tb.same(base17, other)
    assert all((o["grec"]["n_geo"] > 1000).all() and (np.abs(o["ab"][:, 0] - 1.0) > 0.02).all() for o in base17[1:])


# ------------------------------------------------------------------------------------------------------------------ 9: lifecycle
def test_actions_leave_no_stale_record():
    """SKIP, RESTART and a bad action give zero records and empty logs in both families (checked in _replay); the tracked ones replay"""
    acts = tb.acts(5, 3, 9)
    assert (acts[1:] == SKIP).any() and (acts[1:] == RESTART).any()
    acts[2][1] = 7   # an action outside the set: BAD_ACTION, handled as SKIP
    outs = _replay(tb.cfg(), 5, acts=acts, min_tracked=2, seqs=(0, 2, 3))
    assert outs[2]["status"][1] == BAD and (np.concatenate([o["status"] for o in outs]) == SKIPPED).any()


def test_camera_change_restarts_the_sequence():
    cams = np.stack([KH] * 5).astype(F32)
    new = cams.copy()
    new[2, 0, 0] *= 1.02
    outs = _replay(tb.cfg(), 5, cams=cams, cams_at=(2, new), min_tracked=3, seqs=(2, 3))
    assert outs[2]["status"][2] == STARTED and (outs[2]["status"][[0, 1, 3, 4]] == TRACKED).all()


@pytest.mark.parametrize("off", ["geometric", "affine"])
def test_turning_one_term_off_leaves_the_other_family(off):
    """two pushes composed, then one term is turned off through its own setter: from the next push on the batch is bit for bit the batch
    that only ever had the other term"""
    B = 5
    idx = tb.wide_idx(B, pushes=4)
    if off == "geometric":
        got = tb.run(tb.cfg(), B, idx, at={2: lambda bt: bt.set_geometric(dvo.GEOMETRIC_OFF)}, **_term(idx, _zab(), reads=("affine",)))
        only = tb.run(tb.cfg(), B, idx, **_term(idx, _ab, reads=("affine",)))
        tb.same(only, got, families=("affine",), pushes=(2, 3))
        assert all((np.abs(o["ab"][:, 0] - 1.0) > 0.02).all() for o in got[2:])
    else:
        got = tb.run(tb.cfg(), B, idx, at={2: lambda bt: bt.set_affine_brightness(None)}, **_term(idx, _zab(), reads=("geometric",)))
        only = tb.run(tb.cfg(), B, idx, **_term(idx, _z, reads=("geometric",)))
        tb.same(only, got, families=("geometric",), pushes=(2, 3))
        assert all((o["grec"]["n_geo"] > 1000).all() for o in got[2:])
    # (while both were on, the batch was neither)
    assert any(not np.array_equal(got[1]["xi"][b], only[1]["xi"][b]) for b in range(B))


# ------------------------------------------------------------------------------------------------------------------ 10: refusals
def test_errors_are_refused():
    L = dvo.lib()
    bt = dvo.Batch(2, KH, SIZE[0], SIZE[1], LEVELS, CULLS, cfg=tb.cfg())
    GC, AC = dvo.GeometricConfig, dvo.AffineConfig
    gs, as_ = C.sizeof(GC), C.sizeof(AC)
    good_g, good_a = GC(gs, 1, 10.0, 0.1), AC(as_, ESTIMATE, 64, 1e-3, 0.25, 4.0)
    call = lambda g, a: L.dvo_batch_set_geometric_affine(bt._p, C.byref(g) if g is not None else None, C.byref(a) if a is not None else None)
    assert call(None, good_a) == dvo.DVO_ERR_BAD_ARGUMENT and call(good_g, None) == dvo.DVO_ERR_BAD_ARGUMENT and call(None, None) == dvo.DVO_ERR_BAD_ARGUMENT
    assert L.dvo_batch_set_geometric_affine(None, C.byref(good_g), C.byref(good_a)) == dvo.DVO_ERR_BAD_ARGUMENT
    bad_g = [GC(gs, 0, 10.0, 0.1), GC(gs, 2, 10.0, 0.1), GC(gs, 1, -1.0, 0.1), GC(gs, 1, float("nan"), 0.1), GC(gs, 1, float("inf"), 0.1),
             GC(gs, 1, 10.0, 0.0), GC(gs, 1, 10.0, float("nan")), GC(gs, 1, 10.0, float("inf")), GC(gs - 4, 1, 10.0, 0.1), GC(0, 1, 10.0, 0.1)]
    bad_a = [AC(as_, 0, 64, 1e-3, 0.25, 4.0), AC(as_, 3, 64, 1e-3, 0.25, 4.0), AC(as_, ESTIMATE, 1, 1e-3, 0.25, 4.0), AC(as_, ESTIMATE, 64, -0.1, 0.25, 4.0),
             AC(as_, ESTIMATE, 64, 1.0, 0.25, 4.0), AC(as_, GIVEN, 64, 1e-3, 0.0, 4.0), AC(as_, GIVEN, 64, 1e-3, 2.0, 1.0),
             AC(as_, ESTIMATE, 64, 1e-3, 0.25, float("inf")), AC(as_ - 4, ESTIMATE, 64, 1e-3, 0.25, 4.0), AC(0, ESTIMATE, 64, 1e-3, 0.25, 4.0)]
    for g in bad_g:
        assert call(g, good_a) == dvo.DVO_ERR_BAD_ARGUMENT, (g.struct_size, g.mode, g.weight, g.max_diff)
    for a in bad_a:
        assert call(good_g, a) == dvo.DVO_ERR_BAD_ARGUMENT, (a.struct_size, a.mode, a.min_pixels, a.min_contrast, a.gain_min, a.gain_max)
    assert not bt._p is None
    with pytest.raises(dvo.DvoError):
        bt.last_geometric()                         # a refused call turned nothing on, and nothing was pushed
    # robust weights on: refused; and robust weights stay refused while the pair is on
    bt.set_robust_weights(dvo.ROBUST_HUBER, param=1.345, scale_mode=dvo.ROBUST_SCALE_ADAPTIVE, scale_floor=1e-3)
    with pytest.raises(dvo.DvoError):
        bt.set_geometric_affine()
    bt.set_robust_weights(dvo.ROBUST_NONE)
    bt.set_geometric_affine()
    with pytest.raises(dvo.DvoError):
        bt.set_robust_weights(dvo.ROBUST_HUBER, param=1.345, scale_mode=dvo.ROBUST_SCALE_ADAPTIVE, scale_floor=1e-3)
    # the call may be repeated, whatever the state of the two terms; weight 0 is allowed; rows need the GIVEN mode
    bt.set_geometric_affine(weight=0.0, max_diff=0.05, affine_mode=GIVEN)
    bt.set_affine_rows(np.tile(F32([1.1, 0.0]), (2, 1)))
    bt.set_geometric_affine()
    with pytest.raises(dvo.DvoError):
        bt.set_affine_rows(np.tile(F32([1.1, 0.0]), (2, 1)))
    bt.set_geometric(dvo.GEOMETRIC_OFF)
    bt.set_geometric_affine()                       # only the affine family was on
    bt.set_affine_brightness(None)
    bt.set_geometric_affine()                       # only the geometric family was on
    # the two setters keep refusing each other while the pair is on
    with pytest.raises(dvo.DvoError):
        bt.set_affine_brightness(ESTIMATE)
    bt.set_geometric(dvo.GEOMETRIC_OFF)
    with pytest.raises(dvo.DvoError):
        bt.set_geometric(**GEO)
    bt.set_geometric_affine()
    with pytest.raises(dvo.DvoError):
        bt.last_affine()                            # enabled from the next push on
    g, d, s = tb.frames()
    for k in (0, 1):
        t = [tb.dev(x[k:k + 2]) for x in (g, d, s)]
        bt.push_device(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr())
        bt.synchronize()
    assert (bt.last_geometric()["n_geo"] > 1000).all() and (bt.last_affine()[:, 0] > 0.5).all()   # both terms are ready
    assert bt.last_geometric_log(1)["n_iter"][:LEVELS].min() >= 1 and bt.last_affine_log(1)["n_iter"][:LEVELS].min() >= 1
    bt.close()
    # a mono handle
    from util import K640
    mb = dvo.MonoBatch(2, K640, 640, 480, cfg=dvo.default_config(rng_seed=3))
    assert L.dvo_batch_set_geometric_affine(mb._p, C.byref(good_g), C.byref(good_a)) == dvo.DVO_ERR_BAD_ARGUMENT
    mb.close()


# ------------------------------------------------------------------------------------------------------------------ 11: it helps
# The numpy replica of the contract on the oracle (geometric_affine_ref.geometric_affine_track against geometric_ref.geometric_track
# on geometric_affine_ref.outcome_pair): the tracked frame's gray is 1.10 g + 0.02.  Pose error per seed 42..45:
REPLICA_GEOMETRIC = (0.008315, 0.014043, 0.009077, 0.014535)     # summed 0.045970
REPLICA_COMPOSED = (0.0009442, 0.0007864, 0.0004131, 0.0005518)  # summed 0.0026955
REPLICA_WINS = tuple(c < g for c, g in zip(REPLICA_COMPOSED, REPLICA_GEOMETRIC))
REPLICA_RATIO = 0.05864
OUTCOME_CAP = 0.5 * (REPLICA_RATIO + 1.0)


def test_composed_beats_geometric_under_an_exposure_change():
    """geometric_ref's weakly textured pair with the tracked frame's gray replaced by 1.10 g + 0.02, four seeds: frame 1 tracked against
    frame 0, one batch of four sequences per estimator.  The composed batch must win wherever the replica wins and its summed error
    must be at most OUTCOME_CAP times the geometric batch's (the midpoint between the replica's ratio and 1: the losing estimator's
    error moves by tens of percent from seed to seed)."""
    assert REPLICA_WINS == (True, True, True, True)
    o = gr.OUTCOME
    cfg = dvo.default_config(gn_pixels_per_thread=4, crop_enable=0, step_default=o["steps"][0], step_level1=o["steps"][1], step_level2=o["steps"][2],
                             min_residual=o["min_residual"], min_update=o["min_update"], max_iterations=o["max_iterations"])
    pairs = [ga.outcome_pair(seed) for seed in o["seeds"]]
    B = len(pairs)
    K = pairs[0][3]
    err = {}
    for composed in (False, True):
        bt = dvo.Batch(B, K, o["width"], o["height"], o["levels"], o["culls"], cfg=cfg)
        if composed:
            bt.set_geometric_affine()
        else:
            bt.set_geometric()
        for k in (0, 1):
            t = [tb.dev(np.stack([p[j][k] for p in pairs])) for j in (0, 1, 2)]
            bt.push_device(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr())
            bt.synchronize()
        xi, _ = bt.last_poses()
        assert (bt.last_geometric()["n_geo"] > 10000).all()
        if composed:
            assert (bt.last_affine()[:, 0] < 0.95).all()      # the tracked frame is the brighter one
        bt.close()
        err[composed] = np.array([gr.pose_error(xi[b], pairs[b][4]) for b in range(B)])
    wins = err[True] < err[False]
    ratio = err[True].sum() / err[False].sum()
    print("\ngeometric + affine: GPU wins %s, errors %s against geometric only %s, summed %.4g against %.4g, ratio %.4f (replica %.4f, cap %.3f)"
          % (wins.tolist(), err[True].tolist(), err[False].tolist(), err[True].sum(), err[False].sum(), ratio, REPLICA_RATIO, OUTCOME_CAP))
    assert all(w or not r for w, r in zip(wins, REPLICA_WINS)) and ratio <= OUTCOME_CAP, (wins, ratio, err)


def test_zz_report_reduction_bound_ratios():
    """last in the file: under -s, the largest error / bound ratio of every comparison of this process"""
    gn_sums.report("test_gpu_geometric_affine")
    assert all(r <= 1.0 for _, r in gn_sums.RATIOS)
