"""NaN and +-inf pixels in the maps the Gauss-Newton kernels read, against the oracle (tests/nonfinite_cases.py, DESIGN.md §6
"Non-finite pixels").

The kernels restate the reference's is_valid / is_invalid rules (both false for NaN) with selects, bitwise ANDs and raw ISA, and the
solve / pose update promise a refused update when a sum is not finite.  Here every such path sees such pixels: the operator on every
kernel variant and tile shape, a single handle on every schedule, sensor-depth batches with the quality record, the opt-in families
and the mono pipeline.  Finite classes go through the suite's usual comparison (mask bit-exact, per-entry reduction bound); poison
classes through gn_sums.assert_gn_sums_classes (the bound on every finite entry, the exact sum's class on every other)."""
import functools

import numpy as np
import pytest

import dvo_amd as dvo
import gn_sums
import nonfinite_cases as nf
import orc
from test_gpu_parity import _gn_compare

pytestmark = pytest.mark.gpu

VARIANTS = [(0, 1, 1), (0, 2, 2), (0, 4, 1), (0, 4, 4), (0, 8, 4), (8, 1, 0), (8, 4, 0), (2, 2, 0), (16, 8, 0)]   # test_gn_kernel_variants_match_oracle's
TRACKED, STARTED = dvo.SEQ_TRACKED, dvo.SEQ_STARTED
CONVERGED, CAPPED, NOT_FINITE = dvo.QUALITY_CONVERGED, dvo.QUALITY_CAPPED, dvo.QUALITY_NOT_FINITE


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


UPDATE_KINDS = {}           # how often an update of a poison case was the oracle's NaN pattern, its zero, or D13's NaN
RESIDUAL_BITS = [0, 0]      # finite residuals of poison cases (ref_sigma NaN): how many equal the oracle's bit for bit, of how many


def same_class(a, b):
    return nf.classes(a) == nf.classes(b)


def assert_residual(got, want, depth, tag):
    """A finite residual (float(sum_r2) / float(n_valid), optimize.cpp:98) against the oracle's.  Every term of sum_r2 is >= 0, so the
    device's sum is within depth * 2^-24 * (1 + 2^-10) of the exact one RELATIVELY (the reduction bound of tests/gn_sums.py with A = the
    sum itself); each side then rounds the sum to float and divides: four more roundings of 2^-24.  No number of its own."""
    bound = (depth + 4) * gn_sums.U32 * gn_sums.SECOND_ORDER * abs(float(want))
    assert abs(float(got) - float(want)) <= bound, (tag, "residual %.9g, oracle %.9g, bound %.3g" % (got, want, bound))


# ---------------------------------------------------------------------------------------------------------------- operator level
def _poison_compare(where, value, placement, size, level, cfg, group):
    c, o, t = nf.reference(where, value, placement, size, level)
    tag = "%s: %dx%d level %d %s %s %s" % (group, size[0], size[1], level, where, value, placement)
    r = dvo.optimize(*nf.maps_of(c), level, cfg=cfg, want_mask=True)
    np.testing.assert_array_equal(r["mask"], o["mask"], err_msg=tag)
    assert r["n_valid"] == o["n_valid"], tag
    gn_sums.assert_gn_sums_classes(r, t, gn_sums.depth_for_cfg(cfg), tag)
    if o["n_valid"] == 0:      # optimize.cpp:92-93 (the crop of level 2 leaves no pixel of the 5 x 7 pair)
        assert r["residual"] == np.float32(-1) and not r["xi_update"].any(), tag
        return r, o
    assert same_class([r["residual"]], [o["residual"]]), (tag, r["residual"], o["residual"])
    if np.isfinite(o["residual"]):
        RESIDUAL_BITS[0] += int(r["residual"] == o["residual"]); RESIDUAL_BITS[1] += 1
        # the quotient of optimize.cpp:98 in float, of a sum inside its bound: the oracle's value to the rounding of that sum
        assert r["residual"] == np.float32(np.float32(r["sum_r2"]) / np.float32(r["n_valid"])), tag
        assert_residual(r["residual"], o["residual"], gn_sums.depth_for_cfg(cfg), tag)
    # the oracle's NaN pattern; its exact zero where no diagonal sum is > 0 (no pseudo-inverse); all NaN where D13 says so
    kind = nf.assert_update_class(r["xi_update"], o, t, tag)
    UPDATE_KINDS[kind] = UPDATE_KINDS.get(kind, 0) + 1
    if np.isnan(r["xi_update"]).any():
        np.testing.assert_array_equal(bits(r["xi_next"]), bits(c["xi"]), err_msg=tag)      # refused whole: the pose keeps its bits
    else:
        np.testing.assert_allclose(r["xi_next"], orc.se3_concatenate(c["xi"], r["xi_update"]), rtol=2e-6, atol=1e-9, err_msg=tag)
    return r, o


def _operator_cases(cfg, sizes, group):
    n = 0
    for size in sizes:
        for placement in (nf.PLACEMENTS if size in nf.BIG else ("full",)):
            for level in nf.LEVELS:
                for where, value in nf.CASES:
                    if (where, value) in nf.FINITE:
                        c = nf.build(where, value, placement, size)
                        _gn_compare(*nf.maps_of(c), level, cfg=cfg, group=group)
                    else:
                        _poison_compare(where, value, placement, size, level, cfg, group)
                    n += 1
        if size in nf.BIG:      # one +inf pixel in the sampled image: a diagonal sum of H is +inf, not NaN (D13)
            for level in nf.LEVELS:
                _poison_compare("ref_gray", "+inf", "single", size, level, cfg, group)
                n += 1
    return n


@pytest.mark.parametrize("lds,ppt,group", VARIANTS)
@gn_sums.must_be_used
def test_operator_every_class_on_every_kernel_variant(lds, ppt, group):
    """the fast path, the deferred queue at 1 / 2 / 4 / 8 pixels per thread, every gather group and k_track_gn_tile's in-place sampler
    on raster tiles (96 x 50) and on 64-column 2-D tiles with a partial last tile (128 x 33), at levels 0, 1 and 2 (the crop)"""
    cfg = dvo.default_config(gn_use_lds_patch=lds, gn_pixels_per_thread=ppt, gn_gather_group=group)
    assert _operator_cases(cfg, nf.BIG, "nonfinite kernel variants") == 2 * (2 * 3 * 12 + 3)


@gn_sums.must_be_used
def test_operator_every_class_on_the_default_plan_and_a_single_partial_tile():
    assert _operator_cases(None, nf.SIZES, "nonfinite default plan") == (2 * 2 + 1) * 3 * 12 + 2 * 3
    assert UPDATE_KINDS.get("nan", 0) >= 4 and UPDATE_KINDS.get("zero", 0) >= 12 and UPDATE_KINDS.get("oracle", 0) >= 36, UPDATE_KINDS


# ---------------------------------------------------------------------------------------------------------------- single handle
TRACK_CFGS = {"pairs": dict(track_single_launch=-1), "per_iteration": dict(track_single_launch=1), "default": dict(),
              "level_kernel": dict(track_fused_tiles=8)}
EVERY_LEVEL = ("obj_gray", "+inf", (52, 36))     # a multiple of 4 and +inf is_valid: the pixel survives both culls, so every level refuses


def _replay(obj, ref, lg, levels=3, start=None, tag="", depth=None, kinds=None):
    """every logged iteration against orc.optimize at the GPU's input pose of that iteration (obj, ref: orc.OFrame).  depth: the
    reduction depth of the plan that ran, one value or one per level (default: 4 pixels per thread, which every caller's config fixes);
    kinds: a dict that counts the iterations whose H was not finite by nonfinite_cases.assert_update_class's answer."""
    depth = gn_sums.reduction_depth(4) if depth is None else depth
    xi = np.zeros(6, np.float32) if start is None else np.array(start, np.float32)
    n = 0
    for l in range(levels):
        for it in range(lg["n_iter"][l]):
            o = orc.optimize(obj.gray(l), ref.gray(l), ref.depth(l), ref.sigma(l), ref.K(l), xi, l)
            where = (tag, l, it)
            assert lg["n_valid"][l][it] == o["n_valid"], where
            assert same_class([lg["residual"][l][it]], [o["residual"]]), (where, lg["residual"][l][it], o["residual"])
            if np.isfinite(o["residual"]):
                assert_residual(lg["residual"][l][it], o["residual"], gn_sums.at_level(depth, l), where)
            upd = lg["xi_update"][l][it]
            t = None if np.isfinite(o["H"]).all() else orc.optimize_terms(obj.gray(l), ref.gray(l), ref.depth(l), ref.sigma(l), ref.K(l), xi, l)
            if t is None:
                assert np.array_equal(np.isnan(upd), np.isnan(o["xi_update"])), (where, upd, o["xi_update"])
                assert o["xi_update"].any() or not upd.any(), where
            else:
                kind = nf.assert_update_class(upd, o, t, where)
                if kinds is not None:
                    kinds[kind] = kinds.get(kind, 0) + 1
            if not np.isfinite(orc.se3_concatenate(xi, upd)).all():
                np.testing.assert_array_equal(bits(lg["xi_after"][l][it]), bits(xi), err_msg=str(where))     # refused: bit for bit the twist before it
            xi = lg["xi_after"][l][it]
            n += 1
    return n


def _replay_track(c, lg, levels=3, culls=0, tag="", kinds=None):
    obj, ref = nf.oracle_frames(c, levels, culls)
    return _replay(obj, ref, lg, levels, tag=tag, kinds=kinds)


def _logs_equal(a, b, levels, tag):
    assert a["n_iter"] == b["n_iter"], tag
    for l in range(levels):
        for key in ("xi_after", "xi_update", "residual"):
            np.testing.assert_array_equal(bits(a[key][l]), bits(b[key][l]), err_msg="%s %s level %d" % (tag, key, l))
        np.testing.assert_array_equal(a["n_valid"][l], b["n_valid"][l])


@pytest.mark.parametrize("where,value,pixel", [(w, v, nf.TRACK_PIXEL) for w, v in nf.TRACK_CASES] + [EVERY_LEVEL])
def test_track_one_marked_pixel_on_every_schedule(where, value, pixel):
    """dvo.track at 128 x 96, 3 levels, culls = 0 on launch pairs, k_track_gn_fused and k_track_level (the coarsest level): each has
    its own copy of "update rejected".  The same bits from all of them, and every iteration matches the oracle at its input pose."""
    c = nf.build_track(where, value, pixel)
    runs = {}
    for name, kw in TRACK_CFGS.items():
        cfg = dvo.default_config(gn_pixels_per_thread=4, **kw)
        runs[name] = dvo.track(c["obj_gray"], c["ref_gray"], c["ref_depth"], c["ref_sigma"], c["K"], 3, 0, cfg=cfg)
    xi, lg = runs["pairs"]
    for name in ("per_iteration", "default", "level_kernel"):
        np.testing.assert_array_equal(bits(runs[name][0]), bits(xi), err_msg=name)
        _logs_equal(runs[name][1], lg, 3, name)
    assert _replay_track(c, lg, tag="%s %s" % (where, value)) == sum(lg["n_iter"])
    obj, ref = nf.oracle_frames(c)
    _, lo = orc.track(obj, ref)
    if pixel != nf.TRACK_PIXEL:
        assert lg["n_iter"] == [15, 15, 15] == lo["n_iter"] and not xi.any()      # refused on every level: the twist stays zero
        return
    before = lg["xi_after"][1][-1]
    if (where, value) in nf.REFUSED:
        assert lg["n_iter"][2] == 15 == lo["n_iter"][2]
        assert np.isnan(lg["upd_norm"][2]).all()
        for it in range(15):
            np.testing.assert_array_equal(bits(lg["xi_after"][2][it]), bits(before))
        np.testing.assert_array_equal(bits(xi), bits(before))
    elif (where, value) == ("ref_gray", "+inf"):
        # the oracle: a zero update, "converged" after one iteration with an infinite residual.  One +inf pixel leaves +inf, not NaN, on
        # the diagonal of H, so the device answers NaN (D13): refused, and the level runs to the cap
        assert lo["n_iter"][2] == 1 and lo["residual"][2][0] == np.inf
        t = orc.optimize_terms(obj.gray(2), ref.gray(2), ref.depth(2), ref.sigma(2), ref.K(2), before, 2)
        assert nf.device_update_class(t) == "nan"
        assert lg["n_iter"][2] == 15 and (lg["residual"][2] == np.inf).all() and np.isnan(lg["upd_norm"][2]).all()
        np.testing.assert_array_equal(bits(xi), bits(before))
    else:
        assert np.isfinite(xi).all() and np.isfinite(lg["residual"][2]).all() and lg["n_iter"][2] > 1


@pytest.mark.parametrize("where", ["obj_gray", "ref_gray"])
def test_handle_schedules_refuse_the_same_bits(monkeypatch, where):
    """A dvo_vo handle (4 levels, 1 cull) at 256 x 192 with a +inf gray pixel (NaN would not survive the cull) on k_track_persist, its
    give-up path, k_track_gn_fused and launch pairs.  In the tracked frame it poisons g: the finest level refuses 15 updates.  In
    the reference frame it poisons H with +inf on the diagonal: the device's solve answers NaN where the oracle answers zero (D13),
    so that copy of the refusal is reached through a non-finite H.  The same bits on every schedule."""
    size = (256, 192)
    c = nf.build_track(where, "+inf", (102, 74), size)      # (51, 37) of the 128 x 96 top level: the finest level only
    runs = {}
    for name, (sl, limit) in {"persist": (0, None), "per_iteration": (1, None), "pairs": (-1, None), "persist_gives_up": (0, "0")}.items():
        if limit is None:
            monkeypatch.delenv("DVO_PERSIST_SPIN_LIMIT", raising=False)
        else:
            monkeypatch.setenv("DVO_PERSIST_SPIN_LIMIT", limit)
        vo = dvo.VisualOdometry(c["K"], size[0], size[1], cfg=dvo.default_config(track_single_launch=sl, gn_pixels_per_thread=4))
        vo.odometrizeUsingDepth(c["ref_gray"], c["ref_depth"], c["ref_sigma"])
        T = vo.odometrizeUsingDepth(c["obj_gray"], c["ref_depth"], c["ref_sigma"])
        runs[name] = (T.copy(), vo.lastTrackLog())
        vo.close()
    monkeypatch.delenv("DVO_PERSIST_SPIN_LIMIT", raising=False)
    T, lg = runs["pairs"]
    for name in ("persist", "per_iteration", "persist_gives_up"):
        np.testing.assert_array_equal(bits(runs[name][0]), bits(T), err_msg=name)
        _logs_equal(runs[name][1], lg, 4, name)
    kinds = {}
    assert _replay_track(c, lg, 4, 1, "handle " + where, kinds) == sum(lg["n_iter"])
    before = lg["xi_after"][2][-1]
    assert np.isnan(lg["xi_update"][3]).all() and np.isfinite(T).all()
    for it in range(lg["n_iter"][3]):
        np.testing.assert_array_equal(bits(lg["xi_after"][3][it]), bits(before))
    if where == "obj_gray":
        obj, ref = nf.oracle_frames(c, 4, 1)
        _, lo = orc.track(obj, ref)
        assert lg["n_iter"][3] == 15 == lo["n_iter"][3] and (lg["residual"][3] == np.inf).all() and not kinds
    else:
        # every finest-level iteration is D13's: NaN where the oracle answers zero.  A NaN norm never stops the level; the
        # (repeated) residual does, if it is finite and below min_residual (tracker.cpp:68-69)
        assert kinds == {"nan": lg["n_iter"][3]}, kinds
        early = bool(lg["residual"][3][0] < np.float32(dvo.default_config().min_residual))
        assert lg["n_iter"][3] == (1 if early else 15), (lg["n_iter"], lg["residual"][3])


# ---------------------------------------------------------------------------------------------------------------- sensor-depth batch
ROBUST = {"huber": (dvo.ROBUST_HUBER, 1.345), "student_t": (dvo.ROBUST_STUDENT_T, 5.0)}
B, MARKED, TOP = 11, (3, 8), 2            # one marked sequence in each solve workgroup (DVO_SOLVE_SEQ = 8)


def _batch_cfg(**kw):
    # keyframes live longer than the three pushes: with keyframe tracking the first frame stays the reference
    return dvo.default_config(gn_pixels_per_thread=4, keyframe_min_translation=1.0, keyframe_max_frames=8, **kw)


@functools.lru_cache(maxsize=None)
def _batch_maps(gray_value):
    """[push][(gray, depth, sigma)] as [B, h, w] arrays (read only).  Push 0, 1, 2 = the reference image, the object image, the
    reference image of nonfinite_cases.build_track; sequence b's gray is scaled by 1 - 0.02 b so that no two sequences agree.
    Sequence 3: `gray_value` at TRACK_PIXEL of its push-1 gray (the tracked frame of push 1, the frame-to-frame reference of push 2).
    Sequence 8: NaN at TRACK_PIXEL of its push-0 sigma (the reference of push 1 in both modes; with keyframes of push 2 as well).
    gray_value None: the clean batch."""
    c = nf.build_track("obj_gray", None)
    x, y = nf.TRACK_PIXEL
    pushes = []
    for k in range(3):
        src = c["obj_gray"] if k == 1 else c["ref_gray"]
        g = np.stack([src * np.float32(1 - 0.02 * b) for b in range(B)]).astype(np.float32)
        d = np.stack([c["ref_depth"]] * B); s = np.stack([c["ref_sigma"]] * B)
        if gray_value is not None:
            if k == 1:
                g[3, y, x] = nf.VALUES[gray_value]
            if k == 0:
                s[8, y, x] = np.nan
        for a in (g, d, s):
            a.setflags(write=False)
        pushes.append((g, d, s))
    return tuple(pushes), c["K"]


def _batch_run(gray_value, kf, fusion=False, robust=None):
    maps, K = _batch_maps(gray_value)
    bt = dvo.Batch(B, K, nf.TRACK_SIZE[0], nf.TRACK_SIZE[1], 3, 0, cfg=_batch_cfg())
    try:
        if kf:
            bt.set_keyframe_tracking(True)
        if fusion:
            bt.set_keyframe_fusion(dvo.KF_FUSION_ON, 0.05, 16)
        if robust:
            bt.set_robust_weights(*ROBUST[robust])
        bt.set_track_quality(True)
        depths = gn_sums.plan_depths(bt, 3)
        outs = []
        for k, (g, d, s) in enumerate(maps):
            bt.push_host(g, d, s)
            o = dict(status=bt.last_status().copy(), q=bt.last_track_quality().copy(), depths=depths)
            if k > 0 or kf:
                xi, T = bt.last_poses()
                o.update(xi=xi.copy(), T=T.copy(), logs=[bt.last_track_log(b) for b in range(B)], start=bt.last_start_poses().copy())
            if kf:
                o["key"] = bt.world_poses()[2].copy()
            if fusion:
                o["kf_depth"] = [[bt.keyframe(b, l)["depth"] for l in range(3)] for b in range(B)]
                o["counts"] = [bt.keyframe_fusion_counts(b) for b in range(B)]
                o["rec"] = bt.last_keyframe_fusion().copy()
                o["frame_top"] = [bt.frame(b, TOP)[1] for b in range(B)]
            if k == 1:
                o["frame3"] = [bt.frame(3, l) for l in range(3)]
            outs.append(o)
        return outs
    finally:
        bt.close()


@functools.lru_cache(maxsize=None)
def _clean_run(kf, robust=None):
    """the batch fed clean frames: run once per mode and only read"""
    return _batch_run(None, kf, robust=robust)


def _oframe(maps, K, k, b, with_depth=True):
    g, d, s = maps[k]
    return orc.OFrame(g[b], d[b] if with_depth else None, s[b] if with_depth else None, K, 3, 0)


def _logbits(lg):
    return (tuple(lg["n_iter"][:3]),) + tuple(bits(lg[key][l]).tobytes() for key in ("residual", "xi_after", "xi_update", "upd_norm") for l in range(3)) \
        + tuple(np.asarray(lg["n_valid"][l]).tobytes() for l in range(3))


def _check_refused_record(q, lg, obj, ref, depth, start, tag, may_stop_early=False):
    """the record of a sequence whose finest level refused every update (include/dvo.h, "per-sequence tracking quality")"""
    assert q["status"] == TRACKED, tag
    # a NaN norm never passes the min_update test, so the level runs to the cap -- unless its (repeated) residual is finite and below
    # min_residual (tracker.cpp:68-69), which ends it after one refused iteration
    n = lg["n_iter"][TOP]
    # (may_stop_early: only where the caller says the tracked frame may sit on its reference; push 1 demands the cap)
    early = may_stop_early and bool(lg["residual"][TOP][0] < np.float32(dvo.default_config().min_residual))
    assert n == (1 if early else 15) and list(q["n_iter"][:3]) == lg["n_iter"][:3], (tag, n, lg["residual"][TOP])
    for it in range(n):
        np.testing.assert_array_equal(bits(lg["xi_after"][TOP][it]), bits(start), err_msg=tag)
    assert q["flags"] == NOT_FINITE | (CONVERGED if early else CAPPED), (tag, q["flags"])
    assert np.isnan(q["update_norm"]) and np.isnan(lg["upd_norm"][TOP]).all(), tag
    assert bits(q["residual"]).tobytes() == bits(lg["residual"][TOP][n - 1]).tobytes(), tag
    before = start
    assert np.isnan(q["covariance"]).all() and np.isnan(q["eigenvalues"]).all(), tag      # "NaN ... when a sum is not finite"
    # the sums at the record's input pose: the twist the level kept
    t = orc.optimize_terms(obj.gray(TOP), ref.gray(TOP), ref.depth(TOP), ref.sigma(TOP), ref.K(TOP), before, TOP)
    assert not np.isfinite(t["rw"]).all(), tag
    gn_sums.assert_gn_sums_classes(q, t, depth, "nonfinite batch records: " + tag)


@pytest.mark.parametrize("gray_value", ["nan", "+inf"])
@pytest.mark.parametrize("kf", [False, True], ids=["frame_to_frame", "keyframes"])
@gn_sums.must_be_used
def test_sensor_batch_marked_sequences(kf, gray_value):
    maps, K = _batch_maps(gray_value)
    outs = _batch_run(gray_value, kf)
    clean = _clean_run(kf)
    # every other sequence: the clean batch bit for bit (poses, logs, records) -- nothing leaks through the solve's shared LDS
    for k in range(3):
        for b in range(B):
            if b in MARKED:
                continue
            tag = "push %d seq %d" % (k, b)
            assert outs[k]["status"][b] == clean[k]["status"][b], tag
            assert outs[k]["q"][b].tobytes() == clean[k]["q"][b].tobytes(), tag
            if "xi" not in outs[k]:
                continue
            assert outs[k]["xi"][b].tobytes() == clean[k]["xi"][b].tobytes() and outs[k]["T"][b].tobytes() == clean[k]["T"][b].tobytes(), tag
            assert _logbits(outs[k]["logs"][b]) == _logbits(clean[k]["logs"][b]), tag
    assert (outs[0]["status"] == STARTED).all()
    if kf:
        assert not outs[1]["key"].any() and not outs[2]["key"].any()
    # the device's level maps of the marked frame are the oracle pyramid's, NaN position included
    of = _oframe(maps, K, 1, 3)
    for l in range(3):
        np.testing.assert_array_equal(bits(outs[1]["frame3"][l][0]), bits(of.gray(l)))
        np.testing.assert_array_equal(bits(outs[1]["frame3"][l][1]), bits(of.depth(l)))
    assert not np.isfinite(outs[1]["frame3"][TOP][0]).all() and np.isfinite(outs[1]["frame3"][1][0]).all()
    n = 0
    for k in (1, 2):
        o = outs[k]
        for b in MARKED:
            tag = "%s %s push %d seq %d" % ("keyframes" if kf else "frame to frame", gray_value, k, b)
            ref_k = 0 if kf else k - 1
            obj, ref = _oframe(maps, K, k, b, with_depth=False), _oframe(maps, K, ref_k, b)
            lg, q = o["logs"][b], o["q"][b]
            assert o["status"][b] == TRACKED, tag
            n += _replay(obj, ref, lg, 3, start=o["start"][b], tag=tag, depth=o["depths"])
            refused = k == 1 or (kf and b == 8)            # the tracked frame's gray (push 1) or the reference's sigma is marked
            if refused:
                # (push 2 with keyframes: sequence 8's frame is its keyframe's image again, so its finite residual may end the level)
                _check_refused_record(q, lg, obj, ref, o["depths"][TOP], lg["xi_after"][TOP - 1][-1], tag, may_stop_early=k == 2)
            elif not kf and b == 3 and gray_value == "+inf":
                # +inf in the reference's gray.  The oracle: a zero update, "converged" after one iteration with an infinite residual.
                # One such pixel leaves +inf on the diagonal of H, so the device's solve answers NaN (D13): the level is refused too
                before = lg["xi_after"][TOP - 1][-1]
                t = orc.optimize_terms(obj.gray(TOP), ref.gray(TOP), ref.depth(TOP), ref.sigma(TOP), ref.K(TOP), before, TOP)
                assert nf.device_update_class(t) == "nan" and not orc.solve6(t["H"], t["g"]).any(), tag
                # (RANK_DEFICIENT as include/dvo.h defines it: the largest diagonal entry, +inf, is > 0 and a pivot fails the test)
                assert lg["n_iter"][TOP] == 15 and q["flags"] == NOT_FINITE | CAPPED | dvo.QUALITY_RANK_DEFICIENT and q["residual"] == np.inf, (tag, q["flags"])
                assert np.isnan(q["update_norm"]) and np.isnan(q["covariance"]).all() and np.isnan(q["eigenvalues"]).all(), tag
                gn_sums.assert_gn_sums_classes(q, t, o["depths"][TOP], "nonfinite batch records: " + tag)
            else:
                # NaN in the reference's gray is filled by the sampler; a clean pair: ordinary finite tracks
                assert np.isfinite(lg["residual"][TOP]).all() and np.isfinite(o["xi"][b]).all() and not q["flags"] & NOT_FINITE, tag
    assert n >= 4 * 3


@pytest.mark.parametrize("robust", ["huber", "student_t"])
def test_sensor_batch_robust_weights_turn_the_refusal_into_a_zero_update(robust):
    """With robust weights on (ADAPTIVE scale), the weight of a NaN residual is NaN (include/dvo.h: |r| <= c is false, c / |r| is
    NaN; A / fmaf(r, r, B) is NaN), so H is poisoned as well as g: no diagonal sum is > 0 and the solve returns the zero update without
    a pseudo-inverse.  Sequence 3 at push 1 therefore "converges" after ONE finest-level iteration with a NaN residual and without
    NOT_FINITE, where the plain batch refuses 15 updates.  The other sequences keep the clean robust batch's bits."""
    outs = _batch_run("nan", False, robust=robust)
    clean = _clean_run(False, robust)
    for k in (1, 2):
        for b in range(B):
            if b not in MARKED:
                assert outs[k]["xi"][b].tobytes() == clean[k]["xi"][b].tobytes() and outs[k]["q"][b].tobytes() == clean[k]["q"][b].tobytes(), (k, b)
                assert _logbits(outs[k]["logs"][b]) == _logbits(clean[k]["logs"][b]), (k, b)
    lg, q = outs[1]["logs"][3], outs[1]["q"][3]
    assert lg["n_iter"][TOP] == 1 and not lg["xi_update"][TOP][0].any() and np.isnan(lg["residual"][TOP][0]), (lg["n_iter"], lg["xi_update"][TOP])
    assert q["flags"] == CONVERGED and q["update_norm"] == 0.0 and np.isnan(q["residual"]), q["flags"]
    assert np.isnan(q["H"]).all() and np.isnan(q["g"]).all() and np.isnan(q["covariance"]).all() and np.isnan(q["eigenvalues"]).all()
    assert np.isfinite(outs[1]["xi"][3]).all()


def test_sensor_batch_one_cull_pyramid_and_track():
    """culls = 1 at 256 x 192: NaN and -inf at even coordinates reach the tracker as INVALID (getPixel's is_valid), +inf survives, odd
    coordinates vanish.  The level maps equal the oracle pyramid's bit for bit and the track replays on the oracle."""
    size = (256, 192)
    c = nf.build_track("obj_gray", None, size=size)
    g1 = c["obj_gray"].copy()
    g1[40, 60] = np.nan; g1[42, 64] = -np.inf; g1[74, 102] = np.inf; g1[41, 61] = np.nan; g1[43, 65] = np.inf
    g = [np.stack([c["ref_gray"]] * 2), np.stack([c["obj_gray"], g1])]
    d = np.stack([c["ref_depth"]] * 2); s = np.stack([c["ref_sigma"]] * 2)
    bt = dvo.Batch(2, c["K"], size[0], size[1], 3, 1, cfg=_batch_cfg())
    try:
        bt.push_host(g[0], d, s)
        bt.push_host(g[1], d, s)
        logs = [bt.last_track_log(b) for b in range(2)]
        start = bt.last_start_poses()
        for b in range(2):
            of = orc.OFrame(g[1][b], d[b], s[b], c["K"], 3, 1)
            for l in range(3):
                got = bt.frame(b, l)
                np.testing.assert_array_equal(bits(got[0]), bits(of.gray(l)))
                np.testing.assert_array_equal(bits(got[1]), bits(of.depth(l)))
            if b == 1:
                top = of.gray(TOP)
                assert top[20, 30] == orc.INVALID and top[21, 32] == orc.INVALID and top[37, 51] == np.inf and not np.isnan(top).any()
            ref = orc.OFrame(g[0][b], d[b], s[b], c["K"], 3, 1)
            assert _replay(of, ref, logs[b], 3, start=start[b], tag="one cull seq %d" % b) == sum(logs[b]["n_iter"])
        assert logs[1]["n_iter"][TOP] == 15 and (logs[1]["residual"][TOP] == np.inf).all()      # the surviving +inf refuses the finest level
        assert np.isfinite(logs[0]["residual"][TOP]).all()
    finally:
        bt.close()


def test_keyframe_fusion_after_a_refused_level():
    """With keyframe fusion on, a sequence whose finest level refused every update still holds a finite twist (the coarser levels'),
    so it fuses like any other: keyframe depth of every level, counts and records equal tests/kf_fusion_ref.py's replica."""
    import kf_fusion_ref as kref
    maps, K = _batch_maps("nan")
    outs = _batch_run("nan", True, fusion=True)
    min_depth = dvo.default_config().min_depth
    for b in range(B):
        levels = [orc.cull_image(maps[0][1][b], TOP - l) for l in range(3)]
        counts = np.zeros(levels[TOP].shape, np.uint8)
        for l in range(3):
            assert outs[0]["kf_depth"][b][l].tobytes() == levels[l].tobytes()
        for k in (1, 2):
            o = outs[k]
            tag = "push %d seq %d" % (k, b)
            assert o["status"][b] == TRACKED and not o["key"][b] and np.isfinite(o["xi"][b]).all(), tag
            levels, counts, rec = kref.fuse(levels, counts, o["frame_top"][b], K.reshape(3, 3), o["T"][b], dvo.se3.exp(-o["xi"][b]),
                                            min_depth, 0.05, 16)
            assert {key: int(o["rec"][b][key]) for key in rec} == rec, (tag, o["rec"][b], rec)
            for l in range(3):
                assert o["kf_depth"][b][l].tobytes() == np.ascontiguousarray(levels[l], np.float32).tobytes(), (tag, "level", l)
            assert o["counts"][b].tobytes() == counts.tobytes(), tag
            assert rec["n_fused"] > 1000, (tag, rec)
    for b in MARKED:      # the marked sequences did refuse their finest level at push 1
        assert outs[1]["q"][b]["flags"] == NOT_FINITE | CAPPED and outs[1]["logs"][b]["n_iter"][TOP] == 15


# ---------------------------------------------------------------------------------------------------------------- opt-in families
FAMILY_FINITE = [("ref_gray", "nan"), ("ref_gray", "-inf"), ("ref_depth", "nan"), ("ref_depth", "+inf"), ("ref_sigma", "+inf"), ("ref_sigma", "-inf")]
FAMILIES = ["huber", "student_t", "affine", "geometric", "geometric_affine"]
S2, AB, GEO_W, GEO_D = 1e-3, (0.8, 0.05), 10.0, 0.1


def _family_step(family, c, level, cfg, s2=S2):
    """(device result, n_valid of orc.optimize on the maps the family reads, check) of one operator call.  The geometric families read
    the tracked frame's own depth and sigma (here the case's) and sample the reference depth (the same map: its marks are tap holes)."""
    import affine_ref as ar
    import geometric_affine_ref as gar
    import geometric_ref as gr
    import robust_ref as rr
    og, rg, rd, rs, K, xi = nf.maps_of(c)
    n_orc = orc.optimize(og, rg, rd, rs, K, xi, level)["n_valid"]
    depth = gn_sums.depth_for_cfg(cfg)
    if family in ROBUST:
        kind, param = ROBUST[family]
        got = dvo.optimize_robust(og, rg, rd, rs, K, xi, level, kind, param, s2, cfg=cfg)
        check = lambda tag: rr.assert_sums(got, orc.optimize_terms(og, rg, rd, rs, K, xi, level), kind, param, s2, depth, tag)
    elif family == "affine":
        got = dvo.op_gn_step_affine(og, rg, rd, rs, K, xi, level, AB[0], AB[1], cfg=cfg)
        check = lambda tag: ar.assert_step(got, got["moments"], got["next_ab"], ar.pixels(og, rg, rd, rs, K, xi, level, True, ar.weight_params(cfg)),
                                           AB[0], AB[1], rr.NONE, 1.0, rr.INF, depth, tag=tag)
    elif family == "geometric":
        got = dvo.op_gn_step_geometric(og, rd, rs, rg, rd, K, xi, level, GEO_W, GEO_D, cfg=cfg)
        check = lambda tag: gr.assert_step(got, gr.pixels(og, rd, rs, rg, rd, K, xi, level, True, gr.weight_params(cfg)), GEO_W, GEO_D, tag=tag)
    else:
        got = dvo.op_gn_step_geometric_affine(og, rd, rs, rg, rd, K, xi, level, GEO_W, GEO_D, AB[0], AB[1], cfg=cfg)
        check = lambda tag: gar.assert_step(got, gar.pixels(og, rd, rs, rg, rd, K, xi, level, True, gr.weight_params(cfg)), GEO_W, GEO_D,
                                            AB[0], AB[1], tag=tag)
    return got, n_orc, check


@pytest.mark.parametrize("family", FAMILIES)
def test_opt_in_families(family):
    """Robust Huber / Student-t, affine brightness, the geometric term and geometric + affine on the operator.  Finite classes: n_valid
    is the plain oracle's and the sums, records and next entries pass the family's own replica comparison.  NaN in the tracked frame's
    gray: what include/dvo.h states -- n_valid as the oracle, the update refused and the pose kept, and the state the next iteration
    would start from is the one the family's guards name."""
    cfg = dvo.default_config(gn_pixels_per_thread=4)
    n = 0
    for level in nf.LEVELS:
        for where, value in FAMILY_FINITE:
            c = nf.build(where, value, "full", (96, 50))
            got, n_orc, check = _family_step(family, c, level, cfg)
            tag = "nonfinite families: %s level %d %s %s" % (family, level, where, value)
            assert got["n_valid"] == n_orc > 1000, tag
            check(tag)
            assert np.isfinite(got["xi_update"]).all() and np.isfinite(got["H"]).all(), tag
            n += 1
        c = nf.build("obj_gray", "nan", "full", (96, 50))
        got, n_orc, _ = _family_step(family, c, level, cfg)
        tag = "%s obj_gray nan level %d" % (family, level)
        assert got["n_valid"] == n_orc > 1000, tag
        upd = got["xi_update"]
        if family not in ROBUST:
            # H finite, g NaN: the update is NaN and refused, the pose keeps its bits
            assert np.isnan(upd).all() and np.isfinite(got["H"]).all() and nf.classes(got["g"]) == "n" * 6, (tag, upd)
            np.testing.assert_array_equal(bits(got["xi_next"]), bits(c["xi"]), err_msg=tag)
        else:
            # the weight of a NaN residual is NaN by the formulas of include/dvo.h, so H is poisoned as well: no diagonal sum is
            # > 0 and the solve returns the ZERO update without a pseudo-inverse -- applied, which keeps the pose to rounding
            assert not upd.any() and np.isnan(got["H"]).all() and np.isnan(got["g"]).all(), (tag, upd)
            np.testing.assert_allclose(got["xi_next"], orc.se3_concatenate(c["xi"], upd), rtol=2e-6, atol=1e-9, err_msg=tag)
        assert np.isnan(got["residual"]), tag
        if family in ROBUST:
            # ADAPTIVE would take s2 from this residual: it is not > 0, so the next iteration is plain -- the plain operator's bits
            kind, param = ROBUST[family]
            nxt = dvo.optimize_robust(*nf.maps_of(c), level, kind, param, got["residual"], cfg=cfg)
            plain = dvo.optimize(*nf.maps_of(c), level, cfg=cfg)
            for key in ("H", "g"):
                assert np.array_equal(nxt[key], plain[key], equal_nan=True), (tag, key)
            assert np.isfinite(plain["H"]).all() and nf.classes(plain["g"]) == "n" * 6 and nxt["n_valid"] == plain["n_valid"], tag
        if "affine" in family:
            # the closed form of NaN moments is not finite: the finite guard keeps the entry
            assert bits(got["next_ab"]).tobytes() == bits(AB).tobytes(), (tag, got["next_ab"])
    assert n == 3 * len(FAMILY_FINITE)


# ---------------------------------------------------------------------------------------------------------------- mono
def test_mono_lockstep_through_a_frame_with_nonfinite_pixels():
    """A one-camera MonoBatch at 320 x 240 in lockstep with the oracle (tests/lockstep.py).  Frame 2 carries NaN, +inf and -inf gray
    pixels at multiples of 4, so they survive both culls as INVALID, +inf and INVALID; the lockstep assertions hold for that frame and
    the three after it (tracking per iteration, keyframe decision, mapping and the keyframe's maps bit for bit)."""
    import test_gpu_mono_lockstep as ml
    w, h = 320, 240
    K = ml._scaled(ml.K640, w, h)
    g, _ = ml.render(K, w, h)
    marked = g[2].copy()
    marked[100, 120] = np.nan; marked[120, 160] = np.inf; marked[140, 200] = -np.inf
    top = orc.cull_image(marked, 2)
    assert top[25, 30] == orc.INVALID and top[30, 40] == np.inf and top[35, 50] == orc.INVALID and not np.isnan(top).any()
    order = ml.orders(1)[0][:6]
    assert order[2] == 2
    reps = ml._run_batch([K], w, h, lambda q, k: marked if k == 2 else g[order[k]], 6)
    cov = reps[0].coverage()
    print("mono lockstep with non-finite pixels:", cov)
    assert reps[0].frame_id == 5 and cov["iterations"] >= 15
    # the marked frame was tracked with +inf in the per-pixel image and was then, as a keyframe or through the next frame's
    # reference, sampled: iterations with non-finite sums were replayed, D13's among them
    assert cov["nonfinite_iterations"] > 0 and cov["d13_iterations"] > 0, cov


def test_zz_report_reduction_bound_ratios():
    """last in the file: under -s, the largest error / bound ratio of every assert_gn_sums* call of this file"""
    gn_sums.report("test_gpu_nonfinite_pixels")
    print("updates of the operator's poison cases:", UPDATE_KINDS)
    print("finite residuals of poison cases equal to the oracle's bit for bit: %d of %d" % tuple(RESIDUAL_BITS))
