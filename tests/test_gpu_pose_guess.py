"""Per-sequence start pose of a batch's tracking (dvo_batch_set_pose_guess_mode, include/dvo.h) on the GPU, both batch kinds.

Off is today's bits; a non-zero start is checked against the oracle iteration by iteration; a sequence's guess never touches another;
CONSTANT_VELOCITY equals GIVEN fed a host model built on dvo.se3.concatenate; every schedule gives the same bits with the same
guesses; device rows follow the rules of host rows; and on a smooth trajectory with large per-frame motion a guess keeps track where
the zero start loses it.  One tile size throughout (gn_pixels_per_thread = 4), as tests/test_gpu_batch_lifecycle.py."""
import numpy as np
import pytest

import dvo_amd as dvo
import lockstep
import orc
from dvo_amd import synth
from util import K640, TOL_BACKWARD, assert_composed, backward_error, frames

pytestmark = pytest.mark.gpu

SKIP, TRACK, RESTART = dvo.SEQ_SKIP, dvo.SEQ_TRACK, dvo.SEQ_RESTART
TRACKED, SKIPPED, STARTED = dvo.SEQ_TRACKED, dvo.SEQ_SKIPPED, dvo.SEQ_STARTED
NONE, GIVEN, CV = dvo.GUESS_NONE, dvo.GUESS_GIVEN, dvo.GUESS_CONSTANT_VELOCITY
cat = dvo.se3.concatenate


def _cfg(**kw):
    return dvo.default_config(gn_pixels_per_thread=4, **kw)


def _bits(lg):
    L = int(lg["levels"]) if "levels" in lg else 4
    return (tuple(int(n) for n in lg["n_iter"][:L]), tuple(np.asarray(r, np.float32).tobytes() for r in lg["residual"][:L]),
            tuple(np.asarray(x, np.float32).tobytes() for x in lg["xi_after"][:L]))


def _dev(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return t


def _gt_rel(poses, ref, obj):
    """relative twist of frame obj against frame ref, in the convention of dvo_batch_last_poses (bench.py: exp(xi) = inv(P_obj) P_ref)"""
    return dvo.se3.log(np.linalg.inv(poses[obj]) @ poses[ref]).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------ sensor depth
def _sensor_run(cfg, B, idx, mode=None, rows=None, acts=None, feed="device", prefetch=False, cams=None, dists=None, B_log=None):
    """idx[k][b]: frame of sequence b at push k.  rows(k, outs) -> [B, 6] or None; acts[k] or None; cams / dists: {k: K table / D}
    set before push k.  Returns per push dict(xi, T, status, start, logs)."""
    g, d, s, _ = frames(6, sigma=0.1)
    bt = dvo.Batch(B, K640, 640, 480, 4, 1, cfg=cfg)
    if mode is not None:
        bt.set_pose_guess_mode(mode)
    outs = []
    tens = []
    for k in range(len(idx)):
        sel = list(idx[k])
        gi, di, si = g[sel].copy(), d[sel].copy(), s[sel].copy()
        if acts is not None:
            skip = np.array([a == SKIP for a in acts[k]])
            gi[skip] = np.nan; di[skip] = np.nan; si[skip] = np.nan
            bt.set_actions(np.asarray(acts[k], np.uint8))
        if cams and k in cams:
            bt.set_intrinsics(cams[k])
        if dists and k in dists:
            bt.set_distortion(dists[k])
        r = rows(k, outs) if rows is not None else None
        if r is not None:
            bt.set_pose_guess(r)
        if feed == "host":
            bt.push_host(gi, di, si)
        else:
            t = [_dev(x) for x in (gi, di, si)]
            tens.append(t)
            if prefetch:
                bt.prefetch_device(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr())
            bt.push_device(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr())
        if k == 0 and acts is None:   # (a plain first push only stores the reference: no poses yet)
            outs.append(dict(xi=np.zeros((B, 6), np.float32), T=np.zeros((B, 4, 4), np.float32), status=bt.last_status(),
                             start=bt.last_start_poses(), logs=[]))
            continue
        xi, T = bt.last_poses()
        outs.append(dict(xi=xi.copy(), T=T.copy(), status=bt.last_status(), start=bt.last_start_poses(),
                         logs=[_bits(bt.last_track_log(b)) for b in range(B_log or B)]))
    bt.close()
    return outs


def _same(a, b, sl=slice(None), start=True):
    assert len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        np.testing.assert_array_equal(x["xi"][sl], y["xi"][sl], err_msg="push %d" % k)
        np.testing.assert_array_equal(x["T"][sl], y["T"][sl], err_msg="push %d" % k)
        np.testing.assert_array_equal(x["status"][sl], y["status"][sl], err_msg="push %d" % k)
        if start:
            np.testing.assert_array_equal(x["start"][sl], y["start"][sl], err_msg="push %d" % k)
        assert x["logs"][sl] == y["logs"][sl], k


IDX4 = [[0, 1, 2, 3], [1, 2, 3, 4], [2, 3, 4, 5], [3, 2, 5, 4], [4, 1, 4, 3]]


def _gt_rows(idx):
    _, _, _, poses = frames(6, sigma=0.1)

    def rows(k, outs):
        if k == 0:
            return None
        return np.stack([_gt_rel(poses, idx[k - 1][b], idx[k][b]) for b in range(len(idx[k]))])
    return rows


def test_sensor_off_means_today():
    base = _sensor_run(_cfg(), 4, IDX4)
    _same(base, _sensor_run(_cfg(), 4, IDX4, mode=NONE))
    _same(base, _sensor_run(_cfg(), 4, IDX4, mode=GIVEN, rows=lambda k, o: np.zeros((4, 6), np.float32)))
    for o in base:
        assert not np.any(o["start"])


def test_sensor_nonzero_start_matches_the_oracle():
    _oracle_at_the_start(_cfg())


def _oracle_at_the_start(cfg):
    """every Gauss-Newton iteration of a push that starts from a non-zero row, re-run by orc.optimize at the GPU's input pose"""
    g, d, s, poses = frames(6, sigma=0.1)
    idx = [[0, 2], [2, 0]]
    rows = _gt_rows(idx)
    out = _sensor_run(cfg, 2, idx, mode=GIVEN, rows=rows)
    bt = dvo.Batch(2, K640, 640, 480, 4, 1, cfg=cfg)   # (a second run for the full logs)
    bt.set_pose_guess_mode(GIVEN)
    r1 = rows(1, None)
    for k in range(2):
        t = [_dev(x[idx[k]]) for x in (g, d, s)]
        if k == 1:
            bt.set_pose_guess(r1)
        bt.push_device(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr())
    start = bt.last_start_poses()
    np.testing.assert_array_equal(start, r1)                      # the start is the row, bit for bit
    np.testing.assert_array_equal(start, out[1]["start"])
    crop = bool(cfg.crop_enable)
    for b in range(2):
        log = bt.last_track_log(b)
        ref = orc.OFrame(g[idx[0][b]], d[idx[0][b]], s[idx[0][b]], K640, 4, 1)
        obj = orc.OFrame(g[idx[1][b]], d[idx[1][b]], s[idx[1][b]], K640, 4, 1)
        xi = r1[b].copy()
        n_it = 0
        for l in range(4):
            for it in range(int(log["n_iter"][l])):
                where = "seq %d level %d iteration %d" % (b, l, it)
                o = orc.optimize(obj.gray(l), ref.gray(l), ref.depth(l), ref.sigma(l), ref.K(l), xi, l, crop=crop)
                upd, after = log["xi_update"][l][it], log["xi_after"][l][it]
                assert o["n_valid"] == int(log["n_valid"][l][it]), where
                if o["n_valid"] > 0:
                    np.testing.assert_allclose(log["residual"][l][it], o["residual"], rtol=lockstep.RESIDUAL_RTOL, err_msg=where)
                    assert backward_error(o["H"], o["g"], upd) <= TOL_BACKWARD, where
                assert_composed(xi, upd, after, tag=where)
                xi = np.asarray(after, np.float32).copy()
                n_it += 1
        assert n_it >= 4
        np.testing.assert_array_equal(xi, out[1]["xi"][b])
    bt.close()


def test_sensor_sequences_are_independent():
    rows = _gt_rows(IDX4)
    many = _sensor_run(_cfg(), 4, IDX4, mode=GIVEN, rows=rows)
    for b in range(4):
        one = _sensor_run(_cfg(), 1, [[r[b]] for r in IDX4], mode=GIVEN,
                          rows=lambda k, o, b=b: None if k == 0 else rows(k, o)[b:b + 1])
        for k in range(1, len(IDX4)):
            np.testing.assert_array_equal(many[k]["xi"][b], one[k]["xi"][0], err_msg="push %d seq %d" % (k, b))
            np.testing.assert_array_equal(many[k]["start"][b], one[k]["start"][0])
            assert many[k]["logs"][b] == one[k]["logs"][0], (k, b)


def _sensor_schedule(B=6, n_push=9, seed=11):
    rng = np.random.RandomState(seed)
    acts = rng.choice([SKIP, TRACK, RESTART], size=(n_push, B), p=(0.2, 0.65, 0.15)).astype(np.uint8)
    acts[0] = TRACK
    idx = [[int(rng.randint(6)) for _ in range(B)] for _ in range(n_push)]
    K2 = np.stack([K640] * B).astype(np.float32)
    K2[1, 0, 0] *= np.float32(1.02)
    cams = {4: K2}
    dists = {6: np.array([0.01, -0.005, 0.0, 0.0, 0.0], np.float32)}
    return idx, acts, cams, dists


def _velocity_rows(B):
    """host model of CONSTANT_VELOCITY (sensor depth): the relative twist of the last TRACKED push since the last start"""
    vel = np.zeros((B, 6), np.float32)

    def rows(k, outs):
        if k > 0:
            o = outs[k - 1]
            for b in range(B):
                if o["status"][b] == TRACKED:
                    vel[b] = o["xi"][b]
                elif o["status"][b] == STARTED:
                    vel[b] = 0.0
        return vel.copy()
    return rows


def test_sensor_constant_velocity_matches_the_host_model():
    idx, acts, cams, dists = _sensor_schedule()
    cv = _sensor_run(_cfg(), 6, idx, mode=CV, acts=acts, cams=cams, dists=dists)
    given = _sensor_run(_cfg(), 6, idx, mode=GIVEN, rows=_velocity_rows(6), acts=acts, cams=cams, dists=dists)
    _same(cv, given)
    n_nonzero = sum(int(np.any(o["start"], axis=1).sum()) for o in cv)
    assert n_nonzero >= 8, n_nonzero
    assert any((o["status"] == STARTED).any() for o in cv[1:]) and any((o["status"] == SKIPPED).any() for o in cv)


@pytest.mark.parametrize("variant", ["adaptive_off", "fused_tiles", "streams", "lds_patch", "single_launch", "host_feed", "prefetch"])
def test_sensor_schedules_give_the_same_bits(variant):
    B = 4
    if variant == "lds_patch":   # (another tile shape, so other bits than the default: its own non-zero starts against the oracle)
        _oracle_at_the_start(_cfg(gn_use_lds_patch=1))
        return
    rows = _gt_rows(IDX4)
    base = _sensor_run(_cfg(), B, IDX4, mode=GIVEN, rows=rows)
    kw = dict(adaptive_off=dict(track_adaptive=-1), fused_tiles=dict(track_fused_tiles=8), streams=dict(track_streams=2),
              lds_patch=dict(gn_use_lds_patch=1), single_launch=dict(track_single_launch=1)).get(variant, {})
    other = _sensor_run(_cfg(**kw), B, IDX4, mode=GIVEN, rows=rows, feed="host" if variant == "host_feed" else "device",
                        prefetch=variant == "prefetch")
    _same(base, other)


def test_sensor_raw_feeds_give_the_same_bits():
    import torch
    g, d, _, poses = frames(6, sigma=0.1)
    g8 = np.clip(np.rint(g * 255), 0, 255).astype(np.uint8)
    d16 = np.clip(np.rint(d * 5000), 0, 65535).astype(np.uint16)
    rows = _gt_rows(IDX4)
    res = []
    for feed in ("device", "host"):
        bt = dvo.Batch(4, K640, 640, 480, 4, 1, cfg=_cfg())
        bt.set_pose_guess_mode(GIVEN)
        out = []
        for k, sel in enumerate(IDX4):
            r = rows(k, None)
            if r is not None:
                bt.set_pose_guess(r)
            if feed == "host":
                bt.push_raw_host(g8[sel], d16[sel])
            else:
                tg = _dev(g8[sel]); td = torch.from_numpy(d16[sel].view(np.int16)).cuda()
                torch.cuda.synchronize()
                bt.push_raw_device(tg.data_ptr(), 1, td.data_ptr())
            if k:
                out.append((bt.last_poses()[0].copy(), bt.last_start_poses()))
        bt.close()
        res.append(out)
    for (x0, s0), (x1, s1) in zip(*res):
        np.testing.assert_array_equal(x0, x1); np.testing.assert_array_equal(s0, s1)
    assert np.any(res[0][-1][1])


def test_sensor_device_rows():
    import torch
    rows = _gt_rows(IDX4)
    host = _sensor_run(_cfg(), 4, IDX4, mode=GIVEN, rows=rows)
    g, d, s, _ = frames(6, sigma=0.1)
    acts = np.array([TRACK, SKIP, TRACK, TRACK], np.uint8)
    bt = dvo.Batch(4, K640, 640, 480, 4, 1, cfg=_cfg())
    bt.set_pose_guess_mode(GIVEN)
    keep = []
    for k, sel in enumerate(IDX4):
        r = rows(k, None)
        if r is not None:
            tr = torch.from_numpy(r).cuda() * 1.0          # rows written by a torch kernel
            torch.cuda.synchronize()
            keep.append(tr)
            bt.set_pose_guess(tr.data_ptr(), on_device=True)
        t = [_dev(x[sel]) for x in (g, d, s)]
        bt.push_device(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr())
        if k == 0:
            continue
        np.testing.assert_array_equal(bt.last_poses()[0], host[k]["xi"], err_msg="push %d" % k)
        np.testing.assert_array_equal(bt.last_start_poses(), host[k]["start"])
    # NaN rows of a skipped sequence are never read; a non-finite TRACK row starts from zero and is reported as zero
    r = np.zeros((4, 6), np.float32)
    r[1] = np.nan
    r[2] = [0.01, 0.0, 0.0, np.inf, 0.0, 0.0]
    r[3] = rows(1, None)[3]
    tr = _dev(r)
    bt.set_actions(acts)
    bt.set_pose_guess(tr.data_ptr(), on_device=True)
    t = [_dev(x[[1, 2, 3, 4]]) for x in (g, d, s)]
    bt.push_device(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr())
    xi, _ = bt.last_poses()
    st = bt.last_status()
    start = bt.last_start_poses()
    assert list(st) == [TRACKED, SKIPPED, TRACKED, TRACKED]
    assert np.all(np.isfinite(xi))
    assert not np.any(start[:3]), start
    np.testing.assert_array_equal(start[3], r[3])
    bt.close()


def test_errors_are_refused():
    bt = dvo.Batch(2, K640, 640, 480, 4, 1, cfg=_cfg())
    with pytest.raises(dvo.DvoError):
        bt.last_start_poses()                                     # before the first push
    with pytest.raises(dvo.DvoError):
        bt.set_pose_guess_mode(3)
    with pytest.raises(dvo.DvoError):
        bt.set_pose_guess(np.zeros((2, 6), np.float32))           # mode is not GIVEN
    bt.set_pose_guess_mode(CV)
    with pytest.raises(dvo.DvoError):
        bt.set_pose_guess(np.zeros((2, 6), np.float32))
    bt.close()


# ------------------------------------------------------------------------------------------------------------------ mono
MONO_SEED = 3


def _mono_frames():
    import test_gpu_mono_lockstep as ml
    g, _ = ml.render(K640)
    return g, ml.init_depth(K640), ml


def _mono_run(B, idx, mode=None, rows=None, acts=None, per_camera=False, feed="device", with_logs=True):
    """idx[k][b]: frame of sequence b at call k.  rows(k, outs) -> [B, 6] world twists or None.  Returns per call dict."""
    g, init, ml = _mono_frames()
    K = np.stack([K640] * B) if per_camera else K640
    mb = dvo.MonoBatch(B, K, 640, 480, ring_keyframes=16, cfg=dvo.default_config(rng_seed=MONO_SEED), per_sequence_K=per_camera)
    mb.setInitialDepth(init, np.full_like(init, ml.INIT_SIGMA))
    if mode is not None:
        mb.set_pose_guess_mode(mode)
    outs = []
    for k in range(len(idx)):
        fr = g[list(idx[k])].copy()
        if acts is not None:
            fr[np.asarray(acts[k]) == SKIP] = np.nan
            mb.set_actions(np.asarray(acts[k], np.uint8))
        r = rows(k, outs) if rows is not None else None
        if r is not None:
            mb.set_pose_guess(r)
        if feed == "host":
            mb.odometrize_host(fr)
        else:
            t = _dev(fr)
            mb.odometrize_device(t.data_ptr())
        xi, T, key = mb.world_poses()
        outs.append(dict(xi=xi.copy(), T=T.copy(), status=mb.last_status(), key=key.copy(), start=mb.last_start_poses(),
                         logs=[_bits(mb.last_track_log(b)) for b in range(B)] if (with_logs and k > 0) else []))
    mb.close()
    return outs


def _mono_same(a, b, start=True):
    for k, (x, y) in enumerate(zip(a, b)):
        for f in ("xi", "T", "status", "key") + (("start",) if start else ()):
            np.testing.assert_array_equal(x[f], y[f], err_msg="call %d %s" % (k, f))
        assert x["logs"] == y["logs"], k


def _mono_model_rows(B):
    """host model of CONSTANT_VELOCITY (mono) as GIVEN rows: g = concatenate(w1, concatenate(-w2, w1)) from the world twists of the
    last two calls that tracked or started the sequence; NaN (a zero start) while only w1 exists"""
    w1 = np.zeros((B, 6), np.float32); w2 = np.zeros((B, 6), np.float32); n = np.zeros(B, int)

    def rows(k, outs):
        if k > 0:
            o = outs[k - 1]
            for b in range(B):
                if o["status"][b] == TRACKED:
                    w2[b] = w1[b]; w1[b] = o["xi"][b]; n[b] = min(n[b] + 1, 2)
                elif o["status"][b] == STARTED:
                    w1[b] = o["xi"][b]; n[b] = 1
        r = np.full((B, 6), np.nan, np.float32)
        for b in range(B):
            if n[b] >= 2:
                r[b] = cat(w1[b], cat(-w2[b], w1[b]))
        return r
    return rows


MIDX = [[0, 1, 2], [1, 2, 3], [2, 3, 4], [3, 4, 5], [4, 5, 0], [5, 0, 1], [0, 1, 2], [1, 2, 3]]


def test_mono_off_means_today():
    idx = [[0, 1, 2]] * 5          # static sequences: no keyframe after the first, ref_xi stays zero
    base = _mono_run(3, idx)
    for o in base[1:]:
        assert not o["key"].any(), o["key"]
    _mono_same(base, _mono_run(3, idx, mode=NONE))
    _mono_same(base, _mono_run(3, idx, mode=GIVEN, rows=lambda k, o: np.zeros((3, 6), np.float32)))


class GuessReplay(lockstep.Replay):
    """lockstep.Replay whose tracking starts from concatenate(-ref.xi, g) (the world guess g of the frame), not from zero"""
    guess = None
    start = None

    def _track(self, obj, ref, log):
        x0 = cat(-np.asarray(ref.xi, np.float32), self.guess)
        np.testing.assert_array_equal(self.start, x0, err_msg=self._where("start pose"))   # last_start_poses, bit for bit
        assert log is not None
        xi = x0.copy()
        for l in range(lockstep.LEVELS):
            for it in range(int(log["n_iter"][l])):
                where = self._where("level %d iteration %d" % (l, it))
                o = orc.optimize(obj.gray(l), ref.gray(l), ref.depth(l), ref.sigma(l), ref.K(l), xi, l, crop=self.crop)
                upd, after = log["xi_update"][l][it], log["xi_after"][l][it]
                assert o["n_valid"] == int(log["n_valid"][l][it]), where
                if o["n_valid"] > 0:
                    np.testing.assert_allclose(log["residual"][l][it], o["residual"], rtol=lockstep.RESIDUAL_RTOL, err_msg=where)
                    assert backward_error(o["H"], o["g"], upd) <= TOL_BACKWARD, where
                assert_composed(xi, upd, after, tag=where)
                xi = np.asarray(after, np.float32).copy()
                self.n_iterations += 1
        return xi


def test_mono_nonzero_start_matches_the_oracle():
    g, init, ml = _mono_frames()
    B = 2
    orders = [[0, 1, 2, 3, 4, 5, 4, 3], [5, 4, 3, 2, 1, 0, 1, 2]]
    sig = np.full_like(init, ml.INIT_SIGMA)
    mb = dvo.MonoBatch(B, K640, 640, 480, ring_keyframes=16, cfg=dvo.default_config(rng_seed=MONO_SEED))
    mb.setInitialDepth(init, sig)
    mb.set_pose_guess_mode(GIVEN)
    reps = [GuessReplay(K640, 640, 480, MONO_SEED, init, sig, name="sequence %d" % q) for q in range(B)]
    hist = []
    n_nonzero = 0
    for k in range(len(orders[0])):
        fr = np.stack([g[orders[q][k]] for q in range(B)])
        rows = None
        if len(hist) >= 2:
            rows = np.stack([cat(hist[-1][q], cat(-hist[-2][q], hist[-1][q])) for q in range(B)])
        elif hist:
            rows = hist[-1].copy()                                    # the last world pose as the guess
        if rows is not None:
            mb.set_pose_guess(rows)
        t = _dev(fr)
        mb.odometrize_device(t.data_ptr())
        mb.synchronize()
        start = mb.last_start_poses()
        for q, gf in enumerate(lockstep.batch_frames(mb, k == 0)):
            if k > 0:
                reps[q].guess, reps[q].start = rows[q], start[q]
                n_nonzero += int(np.any(start[q]))
            reps[q].step(fr[q], gf)
        hist.append(mb.world_poses()[0].copy())
    mb.close()
    assert n_nonzero >= B * (len(orders[0]) - 2), n_nonzero
    assert sum(r.coverage()["iterations"] for r in reps) > 0


def test_mono_sequences_are_independent():
    many = _mono_run(3, MIDX, mode=CV)
    for b in range(3):
        one = _mono_run(1, [[r[b]] for r in MIDX], mode=CV)
        for k in range(len(MIDX)):
            np.testing.assert_array_equal(many[k]["xi"][b], one[k]["xi"][0], err_msg="call %d seq %d" % (k, b))
            np.testing.assert_array_equal(many[k]["start"][b], one[k]["start"][0])
            if k:
                assert many[k]["logs"][b] == one[k]["logs"][0], (k, b)


def test_mono_constant_velocity_matches_the_host_model():
    rng = np.random.RandomState(4)
    B, n = 4, 12
    acts = rng.choice([SKIP, TRACK, RESTART], size=(n, B), p=(0.2, 0.7, 0.1)).astype(np.uint8)
    acts[0] = TRACK
    idx = [[(b + k) % 6 for b in range(B)] for k in range(n)]
    cv = _mono_run(B, idx, mode=CV, acts=acts)
    given = _mono_run(B, idx, mode=GIVEN, rows=_mono_model_rows(B), acts=acts)
    _mono_same(cv, given)
    assert sum(int(np.any(o["start"], axis=1).sum()) for o in cv) >= 8


@pytest.mark.parametrize("variant", ["per_camera", "host_feed", "adaptive_off"])
def test_mono_schedules_give_the_same_bits(variant):
    base = _mono_run(3, MIDX, mode=CV)
    if variant == "adaptive_off":
        g, init, ml = _mono_frames()
        mb_cfg = dvo.default_config(rng_seed=MONO_SEED, track_adaptive=-1)
        mb = dvo.MonoBatch(3, K640, 640, 480, ring_keyframes=16, cfg=mb_cfg)
        mb.setInitialDepth(init, np.full_like(init, ml.INIT_SIGMA))
        mb.set_pose_guess_mode(CV)
        for k, sel in enumerate(MIDX):
            t = _dev(g[sel])
            mb.odometrize_device(t.data_ptr())
            np.testing.assert_array_equal(mb.world_poses()[0], base[k]["xi"], err_msg="call %d" % k)
            np.testing.assert_array_equal(mb.last_start_poses(), base[k]["start"])
        mb.close()
        return
    other = _mono_run(3, MIDX, mode=CV, per_camera=variant == "per_camera", feed="host" if variant == "host_feed" else "device")
    _mono_same(base, other)


def test_mono_errors_and_device_rows():
    import torch
    g, init, ml = _mono_frames()
    rows = _mono_model_rows(3)
    host = _mono_run(3, MIDX, mode=GIVEN, rows=rows)
    mb = dvo.MonoBatch(3, K640, 640, 480, ring_keyframes=16, cfg=dvo.default_config(rng_seed=MONO_SEED))
    mb.setInitialDepth(init, np.full_like(init, ml.INIT_SIGMA))
    with pytest.raises(dvo.DvoError):
        mb.last_start_poses()
    with pytest.raises(dvo.DvoError):
        mb.set_pose_guess(np.zeros((3, 6), np.float32))
    mb.set_pose_guess_mode(GIVEN)
    rows = _mono_model_rows(3)
    outs, keep = [], []
    for k, sel in enumerate(MIDX):
        r = rows(k, outs)
        tr = torch.from_numpy(r).cuda() + 0.0
        torch.cuda.synchronize()
        keep.append(tr)
        mb.set_pose_guess(tr.data_ptr(), on_device=True)
        t = _dev(g[sel])
        mb.odometrize_device(t.data_ptr())
        xi, T, key = mb.world_poses()
        outs.append(dict(xi=xi.copy(), status=mb.last_status()))
        np.testing.assert_array_equal(xi, host[k]["xi"], err_msg="call %d" % k)
        np.testing.assert_array_equal(mb.last_start_poses(), host[k]["start"])
    mb.close()


# ------------------------------------------------------------------------------------------------------------------ the point
# A smooth trajectory with large per-frame motion (tools/bench_pose_guess.py renders the same one): per sequence a constant twist v in
# a random direction, reached over the first RAMP frames (P_k = P_{k-1} exp(min(1, k / RAMP) v)), tracked with the converging
# configuration of bench.py's side leg (step literals halved, sigma 0.5, stop on the update norm only: the reference's own constants
# do not converge at sigma 0.1, bench.py).
SMOOTH_B, SMOOTH_N, RAMP = 8, 10, 3
SMOOTH_T, SMOOTH_R_DEG = 0.2, 6.0


def converging_cfg():
    return _cfg(step_default=1.0, step_level1=0.75, step_level2=0.5, min_residual=0.0)


def smooth_poses(B=SMOOTH_B, n=SMOOTH_N, step_t=SMOOTH_T, step_r_deg=SMOOTH_R_DEG, seed=21):
    rng = np.random.RandomState(seed)
    out = []
    for _ in range(B):
        dt = rng.normal(size=3); dt *= step_t / np.linalg.norm(dt)
        dr = rng.normal(size=3); dr *= np.radians(step_r_deg) / np.linalg.norm(dr)
        v = np.concatenate([dt, dr])
        P = [np.eye(4)]
        for k in range(1, n):
            P.append(P[-1] @ synth.se3_exp_np(min(1.0, k / RAMP) * v))
        out.append(P)
    return out


def smooth_run(mode, B=SMOOTH_B, n=SMOOTH_N, step_t=SMOOTH_T, step_r_deg=SMOOTH_R_DEG, cfg=None):
    """(mean relative translation error m, mean rotation error deg, iterations per tracked frame) of a sensor-depth batch on the
    smooth trajectory, over the frames after the ramp; GIVEN feeds the ground-truth relative twist"""
    import torch
    P = smooth_poses(B, n, step_t, step_r_deg)
    g, d = synth.render_batch([P[b][k] for k in range(n) for b in range(B)], K640, 640, 480, device="cuda")
    g = g.reshape(n, B, 480, 640).contiguous(); d = d.reshape(n, B, 480, 640).contiguous()
    s = torch.full_like(d, 0.5)
    torch.cuda.synchronize()
    bt = dvo.Batch(B, K640, 640, 480, 4, 1, cfg=cfg or converging_cfg())
    if mode is not None:
        bt.set_pose_guess_mode(mode)
    et, er, its = [], [], []
    for k in range(n):
        if mode == GIVEN and k > 0:
            bt.set_pose_guess(np.stack([dvo.se3.log(np.linalg.inv(P[b][k]) @ P[b][k - 1]) for b in range(B)]).astype(np.float32))
        bt.push_device(g[k].data_ptr(), d[k].data_ptr(), s[k].data_ptr())
        if k < RAMP:
            continue
        xi, _ = bt.last_poses()
        for b in range(B):
            E = synth.se3_exp_np(xi[b].astype(np.float64)) @ np.linalg.inv(np.linalg.inv(P[b][k]) @ P[b][k - 1])
            et.append(float(np.linalg.norm(E[:3, 3])))
            er.append(float(np.degrees(np.arccos(np.clip((np.trace(E[:3, :3]) - 1.0) / 2.0, -1.0, 1.0)))))
            its.append(int(sum(bt.last_track_log(b)["n_iter"][:4])))
    bt.close()
    return float(np.mean(et)), float(np.mean(er)), float(np.mean(its))


def test_a_guess_keeps_track_of_fast_motion():
    none = smooth_run(None)
    given = smooth_run(GIVEN)
    cv = smooth_run(CV)
    print("smooth trajectory (mean t error m, mean r error deg, iterations / frame): none %s given %s cv %s" % (none, given, cv))
    assert given[0] * 3 < none[0], (none, given)
    assert cv[0] * 3 < none[0], (none, cv)
    assert given[2] < none[2] and cv[2] < none[2], (none, given, cv)
