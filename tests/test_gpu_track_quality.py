"""Per-sequence tracking quality of a batch (dvo_batch_set_track_quality, include/dvo.h) on the GPU, both batch kinds.

Off is today's bits; every TRACKED record is the finest level's last solve (the track log's residual, update norm, pixel count and
iterations bit for bit, the logged update solves the record's H, g) and matches the oracle at the GPU's own input pose; eigenvalues,
covariance and flags follow from the record; a sequence that did not track reports the empty record; the schedules give the same
records; and a device-side rule on a device copy restarts exactly the sequences fed an unusable frame.  One tile size throughout
(gn_pixels_per_thread = 4), as tests/test_gpu_pose_guess.py."""
import ctypes as C
import functools

import numpy as np
import pytest

import dvo_amd as dvo
import gn_sums
import lockstep
import orc
from dvo_amd import synth
from util import K640, TOL_BACKWARD, TOL_H_REL, backward_error, frames

pytestmark = pytest.mark.gpu

SKIP, TRACK, RESTART = dvo.SEQ_SKIP, dvo.SEQ_TRACK, dvo.SEQ_RESTART
TRACKED, SKIPPED, STARTED, BAD = dvo.SEQ_TRACKED, dvo.SEQ_SKIPPED, dvo.SEQ_STARTED, dvo.SEQ_BAD_ACTION
CONVERGED, CAPPED, NO_VALID, NOT_FINITE, RANK_DEF = (dvo.QUALITY_CONVERGED, dvo.QUALITY_CAPPED, dvo.QUALITY_NO_VALID,
                                                    dvo.QUALITY_NOT_FINITE, dvo.QUALITY_RANK_DEFICIENT)
EIG_C = 64                 # |eigenvalue - numpy's| <= EIG_C * eps * lambda_max (two Jacobi / LAPACK decompositions in float64)
COV_C = 256                # |H cov / s2 - I| <= COV_C * eps * cond(H)
SUM_R2_REL = 2e-5


def _cfg(**kw):
    return dvo.default_config(gn_pixels_per_thread=4, **kw)


def converging_cfg(**kw):
    """bench.py's converging constants (as tests/test_gpu_pose_guess.py): halved step literals, stop on the update norm only"""
    return _cfg(step_default=1.0, step_level1=0.75, step_level2=0.5, min_residual=0.0, **kw)


def _dev(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return t


def _logbits(lg, L):
    return (tuple(int(n) for n in lg["n_iter"][:L]), tuple(np.asarray(r, np.float32).tobytes() for r in lg["residual"][:L]),
            tuple(np.asarray(x, np.float32).tobytes() for x in lg["xi_after"][:L]))


# ------------------------------------------------------------------------------------------------------------------ sensor depth
IDX = [[0, 1, 2, 3, 4], [1, 2, 3, 4, 5], [2, 3, 4, 5, 0], [3, 2, 5, 4, 1], [4, 1, 4, 3, 2]]


@functools.lru_cache(maxsize=None)
def _frames_of(size, sigma):
    """six frames and their intrinsics: util.frames() at 640x480, the same scene rendered smaller otherwise"""
    w, h = size
    if size == (640, 480):
        return frames(6, sigma=sigma)[:3] + (K640,)
    K = np.array(K640, np.float32).copy()
    K[0] *= w / 640.0; K[1] *= h / 480.0
    g, d, s, _ = synth.sequence(6, width=w, height_px=h, K=K, seed=42, sigma_value=sigma)
    return g.numpy(), d.numpy(), s.numpy(), K


def _sensor_run(cfg, B, idx, quality=True, acts=None, kf=False, feed="device", bad=None, cams=None, sigma=0.1, size=(640, 480), K=None):
    """idx[k][b]: frame of sequence b at push k; acts[k] or None; bad[k]: sequences fed an all-invalid frame at push k; cams: {k: K
    table}; K: the batch's camera (None: the frames').  Returns per push dict(xi, T, status, logs, q, world, plan); plan = level_plan of
    the four levels."""
    g, d, s, K0 = _frames_of(size, sigma)
    bt = dvo.Batch(B, K0 if K is None else K, size[0], size[1], 4, 1, cfg=cfg)
    if kf:
        bt.set_keyframe_tracking(True)
    if quality:
        bt.set_track_quality(True)
    plan = [bt.level_plan(l) for l in range(4)]
    outs, keep = [], []
    for k in range(len(idx)):
        sel = list(idx[k])
        gi, di, si = g[sel].copy(), d[sel].copy(), s[sel].copy()
        for b in (bad or {}).get(k, ()):
            gi[b] = dvo.INVALID; di[b] = 0.0
        if acts is not None:
            bt.set_actions(np.asarray(acts[k], np.uint8))
        if cams and k in cams:
            bt.set_intrinsics(cams[k])
        if feed == "host":
            bt.push_host(gi, di, si)
        elif feed == "raw_host":
            g8 = np.clip(np.rint(gi * 255), 0, 255).astype(np.uint8); d16 = np.clip(np.rint(di * 5000), 0, 65535).astype(np.uint16)
            bt.push_raw_host(g8, d16)
        elif feed == "raw":
            import torch
            g8 = np.clip(np.rint(gi * 255), 0, 255).astype(np.uint8); d16 = np.clip(np.rint(di * 5000), 0, 65535).astype(np.uint16)
            tg = _dev(g8); td = torch.from_numpy(d16.view(np.int16)).cuda()
            torch.cuda.synchronize()
            keep.append((tg, td))
            bt.push_raw_device(tg.data_ptr(), 1, td.data_ptr())
        else:
            t = [_dev(x) for x in (gi, di, si)]
            keep.append(t)
            bt.push_device(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr())
        o = dict(status=bt.last_status(), q=bt.last_track_quality() if quality else None, plan=plan)
        if k > 0 or acts is not None or kf:
            xi, T = bt.last_poses()
            o.update(xi=xi.copy(), T=T.copy(), logs=[bt.last_track_log(b) for b in range(B)])
            if kf:
                o["world"] = bt.world_poses()
        outs.append(o)
    bt.close()
    return outs


def _same_poses(a, b):
    for k, (x, y) in enumerate(zip(a, b)):
        np.testing.assert_array_equal(x["status"], y["status"], err_msg="push %d" % k)
        if "xi" in x:
            np.testing.assert_array_equal(x["xi"], y["xi"], err_msg="push %d" % k)
            np.testing.assert_array_equal(x["T"], y["T"], err_msg="push %d" % k)
            assert [_logbits(l, 4) for l in x["logs"]] == [_logbits(l, 4) for l in y["logs"]], k
        if "world" in x:
            for u, v in zip(x["world"], y["world"]):
                np.testing.assert_array_equal(u, v, err_msg="push %d world" % k)


def _acts(B, n, seed):
    rng = np.random.RandomState(seed)
    a = rng.choice([SKIP, TRACK, RESTART], size=(n, B), p=(0.2, 0.65, 0.15)).astype(np.uint8)
    a[0] = TRACK
    return a


def test_sensor_off_means_today():
    _same_poses(_sensor_run(_cfg(), 5, IDX, quality=False), _sensor_run(_cfg(), 5, IDX))
    acts = _acts(5, len(IDX), 3)
    _same_poses(_sensor_run(_cfg(), 5, IDX, quality=False, acts=acts), _sensor_run(_cfg(), 5, IDX, acts=acts))
    _same_poses(_sensor_run(_cfg(), 5, IDX, quality=False, kf=True), _sensor_run(_cfg(), 5, IDX, kf=True))


def _check_record(q, lg, cfg, L, where):
    """a TRACKED record against the track log and the derivations of include/dvo.h"""
    n_it = int(lg["n_iter"][L]); it = n_it - 1
    assert q["struct_size"] == 496, where
    assert list(q["n_iter"][:L + 1]) == [int(n) for n in lg["n_iter"][:L + 1]] and not q["n_iter"][L + 1:].any(), where
    assert q["n_valid"] == int(lg["n_valid"][L][it]), where
    assert np.float32(q["residual"]).tobytes() == np.float32(lg["residual"][L][it]).tobytes(), where
    assert np.float32(q["update_norm"]).tobytes() == np.float32(lg["upd_norm"][L][it]).tobytes(), where
    upd = lg["xi_update"][L][it]
    if q["n_valid"] > 0:
        assert backward_error(q["H"], q["g"], upd) <= TOL_BACKWARD, where
    # flags, derived on the host from the record, the log and the config
    nrm = float(np.sqrt(np.sum(upd.astype(np.float64) ** 2)))
    f = NO_VALID if q["n_valid"] == 0 else 0
    f |= 0 if np.all(np.isfinite(upd)) else NOT_FINITE
    if cfg.fixed_iterations <= 0:
        if nrm < float(np.float32(cfg.min_update)) or np.float32(q["residual"]) < np.float32(cfg.min_residual):
            f |= CONVERGED
        elif n_it >= cfg.max_iterations:
            f |= CAPPED
    H = orc.upper_to_full(q["H"])
    if q["n_valid"] > 0 and np.all(np.isfinite(H)) and np.abs(H).max() > 0:
        lam = np.linalg.eigvalsh(H)
        if lam[0] <= 1e-9 * lam[-1]:   # (near the 1e-12 pivot test the host cannot restate it: the GPU's word; well away, no flag)
            f |= q["flags"] & RANK_DEF
        np.testing.assert_allclose(q["eigenvalues"], lam, rtol=0, atol=EIG_C * np.finfo(np.float64).eps * abs(lam[-1]), err_msg=where)
        assert np.all(np.diff(q["eigenvalues"]) >= 0), where
        if q["n_valid"] > 6 and not q["flags"] & RANK_DEF and lam[0] > 0:
            s2 = q["sum_r2"] / (q["n_valid"] - 6)
            cov = orc.upper_to_full(q["covariance"])
            cond = lam[-1] / lam[0]
            np.testing.assert_allclose(H @ cov / s2, np.eye(6), rtol=0, atol=COV_C * np.finfo(np.float64).eps * cond, err_msg=where)
        else:
            assert np.isnan(q["covariance"]).all(), where
    else:
        assert np.isnan(q["covariance"]).all(), where
    assert q["flags"] == f, (where, q["flags"], f)


def _check_empty(q, status, where):
    assert q["status"] == status and q["flags"] == 0 and q["n_valid"] == 0 and not q["n_iter"].any(), where
    assert q["residual"] == -1.0 and q["update_norm"] == 0.0 and q["sum_r2"] == 0.0, where
    assert not q["H"].any() and not q["g"].any(), where
    assert np.isnan(q["eigenvalues"]).all() and np.isnan(q["covariance"]).all(), where


def _check_run(outs, cfg, L=3):
    n_tracked = 0
    for k, o in enumerate(outs):
        for b, q in enumerate(o["q"]):
            where = "push %d seq %d" % (k, b)
            assert q["status"] == o["status"][b], where
            if q["status"] != TRACKED:
                _check_empty(q, q["status"], where)
                continue
            _check_record(q, o["logs"][b], cfg, L, where)
            n_tracked += 1
    return n_tracked


@pytest.mark.parametrize("mode", ["plain", "actions", "keyframes"])
def test_sensor_record_is_the_last_solve(mode):
    acts = _acts(5, len(IDX), 5) if mode == "actions" else None
    cfg = _cfg()
    outs = _sensor_run(cfg, 5, IDX, acts=acts, kf=mode == "keyframes")
    assert _check_run(outs, cfg) >= 10
    assert all(q["status"] == STARTED for q in outs[0]["q"]) or acts is not None


def _wide_idx(B):
    """four pushes for B sequences: IDX itself up to five; beyond, sequence b sees frame (k + b) mod 6 at push k, so that neighbouring
    sequences and sequences 8 apart (the same slot of the next solve workgroup) are on different frames at every push -- a partial
    row, a solve slot or a record picked up from another sequence cannot go unnoticed"""
    if B <= 5:
        return [r[:B] for r in IDX[:4]]
    idx = [[(k + b) % 6 for b in range(B)] for k in range(4)]
    for r in idx:
        assert all(r[b] != r[b + 1] for b in range(B - 1)) and all(r[b] != r[b + 8] for b in range(B - 8))
    return idx


def _sensor_oracle(cfg, kf=False, B=3, size=(640, 480), sigma=0.1, cams=None, depth=None, tag="sensor batch "):
    """the record of every TRACKED sequence against the oracle at the input pose of the finest level's last iteration (from the log):
    the max-scaled comparison with orc.optimize, then the one that binds -- H, g, sum_r2 per entry inside the reduction bound of the
    exact sums of orc.optimize_terms (tests/gn_sums.py).  cams: a K table [B, 3, 3] set before the first push (the _cam kernels; the
    oracle takes sequence b's row); depth: the finest level's reduction depth (None: the config's).  Returns the run.  The records are the batch path's own sums (k_track_gn or the LDS-patch /
    fused / one-workgroup kernels over many sequences, then sum_partial_rows / sum_partial_class in the solve), observable nowhere
    else.  With keyframes, the reference is the frame that started or last promoted the sequence."""
    g, d, s, K0 = _frames_of(size, sigma)
    idx = _wide_idx(B)
    outs = _sensor_run(cfg, B, idx, kf=kf, size=size, sigma=sigma, cams=None if cams is None else {0: cams})
    ref_of = list(idx[0])
    crop = bool(cfg.crop_enable)
    depth = gn_sums.depth_for_cfg(cfg) if depth is None else depth
    before = gn_sums.nonempty_calls()
    n = 0
    for k in range(1, len(idx)):
        o = outs[k]
        for b in range(B):
            ref_i, obj_i = (ref_of[b] if kf else idx[k - 1][b]), idx[k][b]
            q, lg = o["q"][b], o["logs"][b]
            L = 3
            it = int(lg["n_iter"][L]) - 1
            x_in = lg["xi_after"][L][it - 1] if it > 0 else lg["xi_after"][L - 1][int(lg["n_iter"][L - 1]) - 1]
            K = K0 if cams is None else cams[b]
            ref = orc.OFrame(g[ref_i], d[ref_i], s[ref_i], K, 4, 1)
            obj = orc.OFrame(g[obj_i], d[obj_i], s[obj_i], K, 4, 1)
            r = orc.optimize(obj.gray(L), ref.gray(L), ref.depth(L), ref.sigma(L), ref.K(L), x_in, L, crop=crop)
            where = "push %d seq %d of %d (%dx%d)" % (k, b, B, size[0], size[1])
            assert r["n_valid"] == q["n_valid"], where
            np.testing.assert_allclose(q["H"], r["H"], rtol=0, atol=TOL_H_REL * np.abs(r["H"]).max(), err_msg=where)
            np.testing.assert_allclose(q["g"], r["g"], rtol=0, atol=TOL_H_REL * max(np.abs(r["g"]).max(), 1e-30), err_msg=where)
            np.testing.assert_allclose(q["sum_r2"], r["sum_r2"], rtol=SUM_R2_REL, err_msg=where)
            t = orc.optimize_terms(obj.gray(L), ref.gray(L), ref.depth(L), ref.sigma(L), ref.K(L), x_in, L, crop=crop)
            gn_sums.assert_gn_sums(q, t, depth, tag + where)
            n += 1
        if kf:
            key = o["world"][2]
            for b in range(B):
                if key[b] or o["status"][b] == STARTED:
                    ref_of[b] = idx[k][b]
    assert n == B * (len(idx) - 1)
    assert gn_sums.nonempty_calls() >= before + n // 2, "the reduction bound saw too few non-empty term lists"
    return outs


def test_sensor_pairs_match_the_oracle():
    _sensor_oracle(_cfg())


def test_keyframe_pairs_match_the_oracle():
    _sensor_oracle(_cfg(keyframe_max_frames=2), kf=True)


def test_lds_patch_matches_the_oracle():
    _sensor_oracle(_cfg(gn_use_lds_patch=1))


def test_batch_size_off_the_solve_workgroup_matches_the_oracle():
    """11 sequences: k_gn_solve takes 8 per workgroup, so the second workgroup is partly empty and sequences 8 .. 10 sit in other slots
    of it than 0 .. 2 of the first"""
    _sensor_oracle(_cfg(), B=11)


@pytest.mark.parametrize("variant", ["adaptive_off", "streams", "fused_tiles", "single_launch"])
def test_schedule_variants_match_the_oracle(variant):
    """The schedules of test_schedules_give_the_same_records, each with its own sums inside the reduction bound.  Two streams need more
    than 16 sequences (19: not a multiple of 8 either).  k_track_level (track_fused_tiles) and k_track_gn_fused (track_single_launch)
    only take levels of a few tiles, and the record is the FINEST level's: those two run on 160x120 frames (finest level 80 x 60,
    five raster tiles), crop off so that the 40 x 30 level keeps its pixels, and sigma 0.5: at 0.1 the ten-fold over-relaxed iteration
    throws half of these small sequences out of the image, and a record without a contributing pixel tests no sum."""
    if variant == "adaptive_off":
        _sensor_oracle(_cfg(track_adaptive=-1))
    elif variant == "streams":
        _sensor_oracle(_cfg(track_streams=2), B=19)
    elif variant == "fused_tiles":
        _sensor_oracle(_cfg(track_fused_tiles=8, crop_enable=0), size=(160, 120), sigma=0.5)
    else:
        _sensor_oracle(_cfg(track_single_launch=1, crop_enable=0), size=(160, 120), sigma=0.5)


def test_flags_capped_fixed_and_no_valid():
    cfg = _cfg(max_iterations=2)
    outs = _sensor_run(cfg, 5, IDX, bad={2: [1, 3]})
    _check_run(outs, cfg)
    flags = np.concatenate([o["q"]["flags"] for o in outs[1:]])
    assert (flags & CAPPED).any(), flags
    assert outs[2]["q"]["flags"][1] & NO_VALID and outs[2]["q"]["flags"][3] & NO_VALID, outs[2]["q"]["flags"]
    assert outs[2]["q"]["n_valid"][1] == 0 and outs[2]["q"]["residual"][1] == -1.0
    cfg = _cfg(fixed_iterations=3)
    outs = _sensor_run(cfg, 5, IDX)
    _check_run(outs, cfg)
    for o in outs[1:]:
        assert not (o["q"]["flags"] & (CONVERGED | CAPPED)).any()
    cfg = converging_cfg()
    outs = _sensor_run(cfg, 5, IDX, sigma=0.5)
    _check_run(outs, cfg)
    assert any((o["q"]["flags"] & CONVERGED).any() for o in outs[1:])


@pytest.mark.parametrize("kind", ["ramp", "stripes"])
def test_rank_deficient_frames(kind):
    import test_gpu_parity_scale as ps
    obj, ref, depth, sigma, K = ps._rank_deficient_case(kind)
    h, w = ref.shape
    bt = dvo.Batch(2, K, w, h, 1, 0, cfg=_cfg(crop_enable=0))
    bt.set_track_quality(True)
    keep = []
    for gray in (ref, obj):
        t = [_dev(np.stack([x, x])) for x in (gray, depth, sigma)]
        keep.append(t)
        bt.push_device(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr())
    q = bt.last_track_quality()
    lg = bt.last_track_log(0)
    bt.close()
    for b in range(2):
        assert q["status"][b] == TRACKED and q["n_valid"][b] > 1000
        assert q["flags"][b] & RANK_DEF, q["flags"]
        assert np.isnan(q["covariance"][b]).all()
        assert np.abs(q["eigenvalues"][b][0]) <= 1e-12 * q["eigenvalues"][b][-1] and q["eigenvalues"][b][-1] > 0
    assert np.float32(q["update_norm"][0]).tobytes() == np.float32(lg["upd_norm"][0][-1]).tobytes()


def test_no_stale_records():
    B = 5
    K2 = np.stack([K640] * B).astype(np.float32)
    K2[3, 0, 0] *= 1.05
    acts = [[TRACK] * B, [TRACK] * B, [SKIP, RESTART, 7, TRACK, TRACK]]
    outs = _sensor_run(_cfg(), B, IDX[:3], acts=acts, cams={2: K2})
    assert (outs[1]["q"]["status"] == TRACKED).all() and (outs[1]["q"]["n_valid"] > 0).all()
    q = outs[2]["q"]
    for b, st in enumerate([SKIPPED, STARTED, BAD, STARTED]):
        _check_empty(q[b], st, "seq %d" % b)
    assert q["status"][4] == TRACKED and q["n_valid"][4] > 0


@pytest.mark.parametrize("variant", ["adaptive_off", "streams", "fused_tiles", "single_launch", "host_feed", "raw_feed"])
def test_schedules_give_the_same_records(variant):
    acts = _acts(5, len(IDX), 9)
    feed = {"host_feed": "host", "raw_feed": "raw_host"}.get(variant, "device")
    kw = {"adaptive_off": dict(track_adaptive=-1), "streams": dict(track_streams=2), "fused_tiles": dict(track_fused_tiles=8),
          "single_launch": dict(track_single_launch=1)}.get(variant, {})
    base = _sensor_run(_cfg(), 5, IDX, acts=acts, feed="raw" if variant == "raw_feed" else "device")
    other = _sensor_run(_cfg(**kw), 5, IDX, acts=acts, feed=feed)
    _same_poses(base, other)
    for k, (x, y) in enumerate(zip(base, other)):
        assert x["q"].tobytes() == y["q"].tobytes(), "push %d" % k


def test_errors_are_refused():
    bt = dvo.Batch(2, K640, 640, 480, 4, 1, cfg=_cfg())
    with pytest.raises(dvo.DvoError):
        bt.last_track_quality()                     # nothing pushed
    g, d, s, _ = frames(3, sigma=0.1)
    t = [_dev(x[:2]) for x in (g, d, s)]
    bt.push_device(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr())
    with pytest.raises(dvo.DvoError):
        bt.last_track_quality()                     # the push ran without quality
    bt.set_track_quality(True)
    with pytest.raises(dvo.DvoError):
        bt.last_track_quality()                     # enabled from the next push on
    t = [_dev(x[1:3]) for x in (g, d, s)]
    bt.push_device(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr())
    a = bt.last_track_quality()
    assert (a["status"] == TRACKED).all()
    bt.set_track_quality(False)
    assert bt.last_track_quality().tobytes() == a.tobytes()   # still the last push
    bt.push_device(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr())
    with pytest.raises(dvo.DvoError):
        bt.last_track_quality()
    assert dvo.lib().dvo_batch_last_track_quality(bt._p, None) == dvo.DVO_ERR_BAD_ARGUMENT
    assert dvo.lib().dvo_batch_copy_track_quality_device(bt._p, None) == dvo.DVO_ERR_BAD_ARGUMENT
    bt.close()


# ------------------------------------------------------------------------------------------------------------------ mono
MONO_SEED = 3
MIDX = [[0, 1, 2], [1, 2, 3], [2, 3, 4], [3, 4, 5], [4, 5, 0], [5, 0, 1]]


def _mono_frames():
    import test_gpu_mono_lockstep as ml
    g, _ = ml.render(K640)
    return g, ml.init_depth(K640), ml


def _mono_run(B, idx, quality=True, acts=None, cfg=None):
    g, init, ml = _mono_frames()
    mb = dvo.MonoBatch(B, K640, 640, 480, ring_keyframes=16, cfg=cfg or dvo.default_config(rng_seed=MONO_SEED))
    mb.setInitialDepth(init, np.full_like(init, ml.INIT_SIGMA))
    if quality:
        mb.set_track_quality(True)
    outs = []
    for k in range(len(idx)):
        fr = g[list(idx[k])].copy()
        if acts is not None:
            mb.set_actions(np.asarray(acts[k], np.uint8))
        t = _dev(fr)
        mb.odometrize_device(t.data_ptr())
        xi, T, key = mb.world_poses()
        outs.append(dict(xi=xi.copy(), T=T.copy(), key=key.copy(), status=mb.last_status(),
                         logs=[mb.last_track_log(b) for b in range(B)] if k > 0 else [],
                         q=mb.last_track_quality() if quality else None))
    mb.close()
    return outs


def _mono_same(a, b):
    for k, (x, y) in enumerate(zip(a, b)):
        for f in ("xi", "T", "status", "key"):
            np.testing.assert_array_equal(x[f], y[f], err_msg="call %d %s" % (k, f))
        assert [_logbits(l, 3) for l in x["logs"]] == [_logbits(l, 3) for l in y["logs"]], k


def test_mono_off_means_today_and_records():
    cfg = dvo.default_config(rng_seed=MONO_SEED)
    on = _mono_run(3, MIDX)
    _mono_same(_mono_run(3, MIDX, quality=False), on)
    assert all(q["status"] == STARTED for q in on[0]["q"])
    assert _check_run(on[1:], cfg, L=2) == 3 * (len(MIDX) - 1)
    acts = np.array([[TRACK] * 3, [TRACK] * 3, [SKIP, TRACK, RESTART], [TRACK, 7, TRACK], [TRACK] * 3, [RESTART, SKIP, TRACK]], np.uint8)
    off = _mono_run(3, MIDX, quality=False, acts=acts)
    on = _mono_run(3, MIDX, acts=acts)
    _mono_same(off, on)
    _check_run(on[1:], cfg, L=2)
    _check_empty(on[2]["q"][0], SKIPPED, "skip"); _check_empty(on[2]["q"][2], STARTED, "restart")
    _check_empty(on[3]["q"][1], BAD, "bad action"); _check_empty(on[5]["q"][0], STARTED, "restart")


class QualityReplay(lockstep.Replay):
    """lockstep.Replay that keeps orc.optimize's result of the finest level's last iteration (at the GPU's logged input pose)"""
    last = None

    def _track(self, obj, ref, log):
        xi = np.zeros(6, np.float32)
        for l in range(lockstep.LEVELS):
            for it in range(int(log["n_iter"][l])):
                o = orc.optimize(obj.gray(l), ref.gray(l), ref.depth(l), ref.sigma(l), ref.K(l), xi, l, crop=self.crop)
                assert o["n_valid"] == int(log["n_valid"][l][it]), self._where("level %d iteration %d" % (l, it))
                if l == lockstep.TOP:
                    self.last = o
                    self.last_args = (obj.gray(l), ref.gray(l), ref.depth(l), ref.sigma(l), ref.K(l), xi.copy(), l, self.crop)
                xi = np.asarray(log["xi_after"][l][it], np.float32).copy()
                self.n_iterations += 1
        return xi


@gn_sums.must_be_used
def test_mono_records_match_the_oracle():
    g, init, ml = _mono_frames()
    B = 2
    orders = [[0, 1, 2, 3, 4, 5], [5, 4, 3, 2, 1, 0]]
    sig = np.full_like(init, ml.INIT_SIGMA)
    mb = dvo.MonoBatch(B, K640, 640, 480, ring_keyframes=16, cfg=dvo.default_config(rng_seed=MONO_SEED))
    mb.setInitialDepth(init, sig)
    mb.set_track_quality(True)
    reps = [QualityReplay(K640, 640, 480, MONO_SEED, init, sig, name="sequence %d" % q) for q in range(B)]
    n = 0
    for k in range(len(orders[0])):
        fr = np.stack([g[orders[q][k]] for q in range(B)])
        t = _dev(fr)
        mb.odometrize_device(t.data_ptr())
        rec = mb.last_track_quality()
        for q, gf in enumerate(lockstep.batch_frames(mb, k == 0)):
            reps[q].last = None
            reps[q].step(fr[q], gf)
            if k == 0:
                assert rec["status"][q] == STARTED
                continue
            r, o = rec[q], reps[q].last
            where = "call %d seq %d" % (k, q)
            assert r["n_valid"] == o["n_valid"], where
            np.testing.assert_allclose(r["H"], o["H"], rtol=0, atol=TOL_H_REL * np.abs(o["H"]).max(), err_msg=where)
            np.testing.assert_allclose(r["g"], o["g"], rtol=0, atol=TOL_H_REL * max(np.abs(o["g"]).max(), 1e-30), err_msg=where)
            np.testing.assert_allclose(r["sum_r2"], o["sum_r2"], rtol=SUM_R2_REL, err_msg=where)
            a = reps[q].last_args      # ... and per entry inside the reduction bound of the exact sums at the same inputs
            t = orc.optimize_terms(*a[:7], crop=a[7])
            gn_sums.assert_gn_sums(r, t, gn_sums.depth_for_cfg(None), "mono batch " + where)
            n += 1
    mb.close()
    assert n == B * (len(orders[0]) - 1)


# ------------------------------------------------------------------------------------------------------------------ on the device
def _restart_rule(qt, n_seq):
    """RESTART where the finest level had no valid pixel, or too few, or a non-finite update; TRACK elsewhere"""
    import torch
    words = qt.view(torch.int32).view(n_seq, C.sizeof(dvo.TrackQuality) // 4)
    flags = words[:, dvo.TrackQuality.flags.offset // 4]
    n_valid = words[:, dvo.TrackQuality.n_valid.offset // 4]
    status = words[:, dvo.TrackQuality.status.offset // 4]
    lost = (status == TRACKED) & (((flags & (NO_VALID | NOT_FINITE)) != 0) | (n_valid < 100))
    return torch.where(lost, torch.full_like(flags, RESTART), torch.full_like(flags, TRACK)).to(torch.uint8)


def test_device_rule_restarts_the_lost_sequences():
    import torch
    B = 6
    g, d, s, _ = frames(6, sigma=0.5)
    bad = [1, 4]
    bt = dvo.Batch(B, K640, 640, 480, 4, 1, cfg=converging_cfg())
    bt.set_track_quality(True)
    qt = torch.empty(B * C.sizeof(dvo.TrackQuality), dtype=torch.uint8, device="cuda")
    keep = []
    statuses = []
    for k in range(4):
        sel = [(b + k) % 6 for b in range(B)]
        gi, di, si = g[sel].copy(), d[sel].copy(), s[sel].copy()
        if k == 2:
            for b in bad:
                gi[b] = dvo.INVALID; di[b] = 0.0
        t = [_dev(x) for x in (gi, di, si)]
        keep.append(t)
        if k >= 1:
            bt.copy_track_quality_device(qt.data_ptr())       # the previous push's records, in stream order
            act = _restart_rule(qt, B)
            keep.append(act)
            bt.set_actions(act.data_ptr(), on_device=True)
        bt.push_device(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr())
        if k == 2:   # (a host read only to check the device copy; the rule above never left the device)
            bt.copy_track_quality_device(qt.data_ptr())
            host = bt.last_track_quality()
            assert qt.cpu().numpy().tobytes() == host.tobytes()
            assert all(host["flags"][b] & NO_VALID for b in bad) and host["n_valid"][[0, 2, 3, 5]].min() > 1000, host["n_valid"]
        statuses.append(bt.last_status())
    bt.close()
    exp = np.full(B, TRACKED); exp[bad] = STARTED
    np.testing.assert_array_equal(statuses[3], exp)
    np.testing.assert_array_equal(statuses[2], np.full(B, TRACKED))


def test_zz_report_reduction_bound_ratios():
    """last in the file: under -s, the largest error / bound ratio of every assert_gn_sums call of this process"""
    gn_sums.report("test_gpu_track_quality")
    assert all(r <= 1.0 for _, r in gn_sums.RATIOS)
