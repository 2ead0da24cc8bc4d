"""Keyframe tracking of a sensor-depth batch (dvo_batch_set_keyframe_tracking, include/dvo.h) on the GPU.

keyframe_max_frames = 1 is today's frame-to-frame batch, bit for bit; otherwise every tracked frame gives the bits of a one-sequence
batch pushed its keyframe and then the frame, under every schedule and input form; is_keyframe and the world twists follow a host
model of the mono rule built on dvo.se3.concatenate; the oracle agrees at the keyframe pair; the keyframe holds the pyramid of the
promoted frame; the start pose follows the mono convention; the errors change nothing; and on a smooth trajectory the world poses
are measured against the composition of frame-to-frame poses.  One tile size throughout (gn_pixels_per_thread = 4)."""
import numpy as np
import pytest

import dvo_amd as dvo
import lockstep
import orc
from dvo_amd import synth
from util import K640, TOL_BACKWARD, assert_composed, backward_error

pytestmark = pytest.mark.gpu

SKIP, TRACK, RESTART = dvo.SEQ_SKIP, dvo.SEQ_TRACK, dvo.SEQ_RESTART
TRACKED, SKIPPED, STARTED = dvo.SEQ_TRACKED, dvo.SEQ_SKIPPED, dvo.SEQ_STARTED
NONE, GIVEN, CV = dvo.GUESS_NONE, dvo.GUESS_GIVEN, dvo.GUESS_CONSTANT_VELOCITY
cat = dvo.se3.concatenate
N_FRAMES = 12


def _cfg(**kw):
    return dvo.default_config(gn_pixels_per_thread=4, **kw)


def _conv(**kw):   # bench.py's converging constants (tests/test_gpu_pose_guess.py::converging_cfg)
    return _cfg(step_default=1.0, step_level1=0.75, step_level2=0.5, min_residual=0.0, **kw)


def _bits(lg):
    return (tuple(int(n) for n in lg["n_iter"][:4]), tuple(np.asarray(r, np.float32).tobytes() for r in lg["residual"][:4]),
            tuple(np.asarray(x, np.float32).tobytes() for x in lg["xi_after"][:4]))


_POOL = {}


def pool():
    """N_FRAMES frames of one trajectory with enough motion for the translation rule (sigma 0.5): float maps and their raw forms"""
    if not _POOL:
        g, d, s, poses = synth.sequence(N_FRAMES, seed=5, sigma_value=0.5, device="cuda", sigma_t=0.012, sigma_r_deg=0.4)
        g, d, s = g.cpu().numpy(), d.cpu().numpy(), s.cpu().numpy()
        g8 = np.clip(np.round(g * 255.0), 0, 255).astype(np.uint8)
        d16 = np.clip(np.round(d * 5000.0), 0, 65535).astype(np.uint16)
        _POOL.update(g=g, d=d, s=s, g8=g8, d16=d16, poses=poses)
    return _POOL


def _dev(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return t


def _push(bt, sel, feed, skip=None):
    """push frames `sel` (one pool index per sequence); skipped slots hold NaN / garbage"""
    P = pool()
    if feed in ("raw_device", "raw_host"):
        g8, d16 = P["g8"][sel].copy(), P["d16"][sel].copy()
        if skip is not None:
            g8[skip] = 77; d16[skip] = 12345
        if feed == "raw_host":
            bt.push_raw_host(g8, d16)
        else:
            t = [_dev(g8), _dev(d16.view(np.int16))]
            bt.push_raw_device(t[0].data_ptr(), 1, t[1].data_ptr())
            bt._keep = t
        return
    g, d, s = P["g"][sel].copy(), P["d"][sel].copy(), P["s"][sel].copy()
    if skip is not None:
        g[skip] = np.nan; d[skip] = np.nan; s[skip] = np.nan
    if feed == "host":
        bt.push_host(g, d, s)
    else:
        t = [_dev(x) for x in (g, d, s)]
        bt.push_device(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr())
        bt._keep = t


def schedule(B, n, seed, p=(0.15, 0.75, 0.10)):
    """actions [n][B] (first push all TRACK) and frames idx[n][B]: every sequence walks forward through the pool"""
    rng = np.random.RandomState(seed)
    acts = rng.choice([SKIP, TRACK, RESTART], size=(n, B), p=p).astype(np.uint8)
    acts[0] = TRACK
    idx = [[(k + 2 * b) % N_FRAMES for b in range(B)] for k in range(n)]
    return idx, acts


def run(cfg, B, idx, acts=None, kf=True, feed="device", K=None, cams=None, dists=None, D0=None, mode=None, rows=None):
    """one batch over the pushes; per push: xi, T, status, logs, start and (keyframe tracking) world twists, T_world, is_keyframe.
    cams / dists: {k: K table / D} set before push k; rows(k, outs) -> GIVEN rows of push k or None"""
    bt = dvo.Batch(B, K640 if K is None else K, 640, 480, 4, 1, cfg=cfg)
    if kf:
        bt.set_keyframe_tracking(True)
    if D0 is not None:
        bt.set_distortion(D0)
    if mode is not None:
        bt.set_pose_guess_mode(mode)
    outs = []
    for k in range(len(idx)):
        skip = None
        if acts is not None:
            bt.set_actions(acts[k])
            skip = acts[k] == SKIP
        if cams and k in cams:
            bt.set_intrinsics(cams[k])
        if dists and k in dists:
            bt.set_distortion(dists[k])
        r = rows(k, outs) if rows is not None else None
        if r is not None:
            bt.set_pose_guess(r)
        _push(bt, list(idx[k]), feed, skip)
        xi, T = bt.last_poses()
        o = dict(xi=xi.copy(), T=T.copy(), status=bt.last_status().copy(), logs=[_bits(bt.last_track_log(b)) for b in range(B)],
                 start=bt.last_start_poses().copy())
        if kf:
            o["xw"], o["Tw"], o["key"] = bt.world_poses()
        outs.append(o)
    return bt, outs


def keyframe_of(outs, idx, consumed=False):
    """host model: the pool frame each sequence's keyframe holds before each push (-1: none); with `consumed`, also the frame the
    sequence consumed last before each push (its frame-to-frame reference)"""
    B = len(idx[0])
    kf = np.full(B, -1); last = np.full(B, -1)
    before, before_last = [], []
    for k, o in enumerate(outs):
        before.append(kf.copy()); before_last.append(last.copy())
        if o is None:   # (a sentinel after the last push: its entry is the keyframe after it)
            break
        for b in range(B):
            if o["status"][b] == STARTED or (o["status"][b] == TRACKED and o["key"][b]):
                kf[b] = idx[k][b]
            if o["status"][b] in (STARTED, TRACKED):
                last[b] = idx[k][b]
    return (before, before_last) if consumed else before


def late_pairs(outs, idx):
    """the TRACKED (push, sequence) pairs whose keyframe is older than the frame the sequence consumed last: pairs a frame-to-frame
    batch would not have tracked"""
    before, last = keyframe_of(outs, idx, consumed=True)
    return [(k, b) for k in range(len(outs)) for b in range(len(idx[0]))
            if outs[k]["status"][b] == TRACKED and before[k][b] != last[k][b]]


def one_sequence(cfg, ref_frame, frame, feed="device", K=None, D=None):
    """relative pose and log of a fresh one-sequence frame-to-frame batch pushed (ref_frame, frame)"""
    bt = dvo.Batch(1, K640 if K is None else K, 640, 480, 4, 1, cfg=cfg)
    if D is not None:
        bt.set_distortion(D)
    _push(bt, [ref_frame], feed)
    _push(bt, [frame], feed)
    xi, _ = bt.last_poses()
    lg = _bits(bt.last_track_log(0))
    bt.close()
    return xi[0], lg


def check_pairs(cfg, outs, idx, n_pairs, seed, feed="device", K_of=None, D=None):
    """a sample of TRACKED (sequence, push) pairs equals a one-sequence batch pushed the keyframe's frame, then the frame"""
    before = keyframe_of(outs, idx)
    pairs = [(k, b) for k in range(len(outs)) for b in range(len(idx[0])) if outs[k]["status"][b] == TRACKED]
    late = late_pairs(outs, idx)
    rng = np.random.RandomState(seed)
    pick = [late[i] for i in rng.choice(len(late), min(len(late), n_pairs - 1), replace=False)] if late else []
    pick.append(pairs[rng.randint(len(pairs))])
    for k, b in pick:
        xi, lg = one_sequence(cfg, before[k][b], idx[k][b], feed, None if K_of is None else K_of(k, b), D)
        np.testing.assert_array_equal(outs[k]["xi"][b], xi, err_msg="push %d seq %d" % (k, b))
        assert outs[k]["logs"][b] == lg, (k, b)
    return len(late)


# ------------------------------------------------------------------------------------------------------------------------- 1
def test_max_frames_one_is_frame_to_frame():
    idx, acts = schedule(6, 12, seed=3, p=(0.25, 0.6, 0.15))
    cfg = _cfg(keyframe_max_frames=1)
    bk, kf = run(cfg, 6, idx, acts)
    bk.close()
    bp, plain = run(cfg, 6, idx, acts, kf=False)
    bp.close()
    for k, (x, y) in enumerate(zip(kf, plain)):
        np.testing.assert_array_equal(x["xi"], y["xi"], err_msg="push %d" % k)
        np.testing.assert_array_equal(x["T"], y["T"], err_msg="push %d" % k)
        np.testing.assert_array_equal(x["status"], y["status"], err_msg="push %d" % k)
        assert x["logs"] == y["logs"], k
        np.testing.assert_array_equal(x["key"], x["status"] != SKIPPED, err_msg="push %d" % k)   # every tracked frame is a keyframe


# ------------------------------------------------------------------------------------------------------------------- 2, 3, 5
_MAIN = {}


def main_run():
    if not _MAIN:
        idx, acts = schedule(8, 14, seed=7)
        bt, outs = run(_conv(), 8, idx, acts)
        import torch
        xw = torch.zeros((8, 6), dtype=torch.float32, device="cuda"); Tw = torch.zeros((8, 16), dtype=torch.float32, device="cuda")
        kw = torch.zeros(8, dtype=torch.int32, device="cuda")
        bt.copy_world_poses_device(xw.data_ptr(), Tw.data_ptr(), kw.data_ptr())
        bt.synchronize()
        dev = (xw.cpu().numpy(), Tw.cpu().numpy().reshape(8, 4, 4), kw.cpu().numpy().astype(bool))
        kfs = [bt.keyframe(b) for b in range(8)]
        bt.close()
        _MAIN.update(idx=idx, acts=acts, outs=outs, dev=dev, kfs=kfs)
    return _MAIN


def test_each_frame_is_tracked_against_its_keyframe():
    m = main_run()
    late = check_pairs(_conv(), m["outs"], m["idx"], 6, seed=1)
    assert late >= 5, "too few frames tracked against an older keyframe: %d" % late


def test_the_rule_and_the_world_poses():
    m = main_run()
    cfg = _conv()
    B = 8
    fid = np.zeros(B, int); kid = np.zeros(B, int); kxi = np.zeros((B, 6), np.float32); xw = np.zeros((B, 6), np.float32)
    started = np.zeros(B, bool)
    by_t = kept = 0
    for k, o in enumerate(m["outs"]):
        for b in range(B):
            st = o["status"][b]
            if st == STARTED:
                fid[b] = 0; kid[b] = 0; kxi[b] = 0; xw[b] = 0; started[b] = True
                assert o["key"][b], (k, b)
            elif st == TRACKED:
                rel = o["xi"][b]
                fid[b] += 1
                tn = np.sqrt(float(rel[0]) * float(rel[0]) + float(rel[1]) * float(rel[1]) + float(rel[2]) * float(rel[2]))
                by_t += int(tn > float(np.float32(cfg.keyframe_min_translation)) and fid[b] - kid[b] < cfg.keyframe_max_frames)
                need = tn > float(np.float32(cfg.keyframe_min_translation)) or fid[b] - kid[b] >= cfg.keyframe_max_frames
                xw[b] = cat(kxi[b], rel)
                assert bool(o["key"][b]) == need, (k, b)
                kept += int(not need)
                if need:
                    kxi[b] = xw[b]; kid[b] = fid[b]
            else:
                assert not o["key"][b], (k, b)
                if not started[b]:
                    np.testing.assert_array_equal(o["Tw"][b], np.eye(4, dtype=np.float32))
            np.testing.assert_array_equal(o["xw"][b], xw[b], err_msg="push %d seq %d" % (k, b))
            np.testing.assert_allclose(o["Tw"][b], synth.se3_exp_np(xw[b].astype(np.float64)), atol=1e-5)
    assert by_t > 0, "the translation rule never fired"
    assert kept > 0, "every tracked frame became a keyframe"
    last = m["outs"][-1]
    for got, want in zip(m["dev"], (last["xw"], last["Tw"], last["key"])):   # the device copy equals the host read
        np.testing.assert_array_equal(got, want)
    for b in range(B):   # keyframe(): the host model's twist and id
        if started[b]:
            np.testing.assert_array_equal(m["kfs"][b]["xi"], kxi[b])
            assert m["kfs"][b]["id"] == kid[b]


def test_keyframe_maps_are_the_promoted_pyramid():
    m = main_run()
    P = pool()
    kf = keyframe_of(m["outs"] + [None], m["idx"] + [None])[-1]   # the model's keyframe after the last push
    for b in range(8):
        if kf[b] < 0:
            continue
        gp, dp, _ = dvo.pyramid(P["g"][kf[b]], P["d"][kf[b]], P["s"][kf[b]], 4, 1)
        np.testing.assert_array_equal(m["kfs"][b]["gray"], gp[3], err_msg="seq %d" % b)
        np.testing.assert_array_equal(m["kfs"][b]["depth"], dp[3], err_msg="seq %d" % b)


def test_keyframe_of_a_skipped_sequence_does_not_change_and_levels():
    P = pool()
    bt = dvo.Batch(3, K640, 640, 480, 4, 1, cfg=_cfg(keyframe_max_frames=1))
    bt.set_keyframe_tracking(True)
    _push(bt, [0, 1, 2], "device")
    _push(bt, [3, 4, 5], "device")                     # every sequence promotes (max frames 1)
    before = [bt.keyframe(1, l) for l in range(4)]
    bt.set_actions(np.array([TRACK, SKIP, TRACK], np.uint8))
    _push(bt, [6, 7, 8], "device", skip=np.array([False, True, False]))
    for l in range(4):
        k = bt.keyframe(1, l)
        np.testing.assert_array_equal(k["gray"], before[l]["gray"])
        np.testing.assert_array_equal(k["depth"], before[l]["depth"])
        gp, dp, _ = dvo.pyramid(P["g"][4], P["d"][4], P["s"][4], 4, 1)
        np.testing.assert_array_equal(k["gray"], gp[l], err_msg="level %d" % l)
        np.testing.assert_array_equal(k["depth"], dp[l], err_msg="level %d" % l)
        k0 = bt.keyframe(0, l)
        gp, dp, _ = dvo.pyramid(P["g"][6], P["d"][6], P["s"][6], 4, 1)
        np.testing.assert_array_equal(k0["gray"], gp[l], err_msg="level %d" % l)
        np.testing.assert_array_equal(k0["depth"], dp[l], err_msg="level %d" % l)
    assert bt.keyframe(1)["n_keyframes"] == 2 and bt.keyframe(0)["n_keyframes"] == 3
    bt.close()


# ------------------------------------------------------------------------------------------------------------------------- 4
def test_oracle_at_the_keyframe_pair():
    """(the oracle's optimize uses the default step constants: a run of its own with them)"""
    P = pool()
    cfg = _cfg(keyframe_max_frames=3)
    idx, acts = schedule(4, 8, seed=13, p=(0.0, 1.0, 0.0))
    bt, outs = run(cfg, 4, idx, acts)
    bt.close()
    m = dict(idx=idx, outs=outs)
    before = keyframe_of(outs, idx)
    late = late_pairs(outs, idx)
    assert late
    for k, b in late[:2]:
        bt = dvo.Batch(1, K640, 640, 480, 4, 1, cfg=cfg)   # (the full log of that pair: its bits are the keyframe batch's, test 2)
        for f in (before[k][b], m["idx"][k][b]):
            _push(bt, [f], "device")
        log = bt.last_track_log(0)
        xi_end, _ = bt.last_poses()
        bt.close()
        assert _bits(log) == m["outs"][k]["logs"][b]
        ref = orc.OFrame(P["g"][before[k][b]], P["d"][before[k][b]], P["s"][before[k][b]], K640, 4, 1)
        obj = orc.OFrame(P["g"][m["idx"][k][b]], P["d"][m["idx"][k][b]], P["s"][m["idx"][k][b]], K640, 4, 1)
        xi = np.zeros(6, np.float32)
        n_it = 0
        for l in range(4):
            for it in range(int(log["n_iter"][l])):
                where = "push %d seq %d level %d iteration %d" % (k, b, l, it)
                o = orc.optimize(obj.gray(l), ref.gray(l), ref.depth(l), ref.sigma(l), ref.K(l), xi, l, crop=bool(cfg.crop_enable))
                upd, aft = log["xi_update"][l][it], log["xi_after"][l][it]
                assert o["n_valid"] == int(log["n_valid"][l][it]), where
                if o["n_valid"] > 0:
                    np.testing.assert_allclose(log["residual"][l][it], o["residual"], rtol=lockstep.RESIDUAL_RTOL, err_msg=where)
                    assert backward_error(o["H"], o["g"], upd) <= TOL_BACKWARD, where
                assert_composed(xi, upd, aft, tag=where)
                xi = np.asarray(aft, np.float32).copy()
                n_it += 1
        assert n_it >= 4
        np.testing.assert_array_equal(xi, xi_end[0])
        np.testing.assert_array_equal(xi, m["outs"][k]["xi"][b])


# ------------------------------------------------------------------------------------------------------------------------- 6
VARIANTS = [
    ("adaptive_off", dict(track_adaptive=-1), "device"),
    ("fused_tiles", dict(track_fused_tiles=8), "device"),
    ("two_streams", dict(track_streams=2), "device"),
    ("lds_patch", dict(gn_use_lds_patch=1), "device"),
    ("single_launch", dict(track_single_launch=1), "device"),
    ("host_feed", dict(), "host"),
    ("raw_device", dict(), "raw_device"),
]


@pytest.mark.parametrize("name,kw,feed", VARIANTS, ids=[v[0] for v in VARIANTS])
def test_schedules_and_inputs(name, kw, feed):
    idx, acts = schedule(6, 9, seed=19)
    cfg = _conv(**kw)
    bt, outs = run(cfg, 6, idx, acts, feed=feed)
    bt.close()
    late = check_pairs(cfg, outs, idx, 3, seed=2, feed=feed)
    assert late > 0, "no pair was tracked against a keyframe older than the previous frame"
    if feed == "raw_device":   # raw device input equals raw host input (constant weights: the 8-map promotion)
        bh, host = run(cfg, 6, idx, acts, feed="raw_host")
        bh.close()
        for k, (x, y) in enumerate(zip(outs, host)):
            np.testing.assert_array_equal(x["xi"], y["xi"], err_msg="push %d" % k)
            np.testing.assert_array_equal(x["xw"], y["xw"], err_msg="push %d" % k)
            assert x["logs"] == y["logs"], k


def test_per_sequence_intrinsics_and_distortion():
    B = 4
    idx, acts = schedule(B, 9, seed=23, p=(0.1, 0.85, 0.05))
    K1 = np.stack([K640] * B).astype(np.float32)
    K1[1, 0, 0] *= np.float32(1.01); K1[3, 1, 2] += np.float32(2.0)
    K2 = K1.copy(); K2[2, 0, 0] *= np.float32(0.99)
    D0 = np.array([0.02, -0.01, 0.0, 0.0, 0.0], np.float32)
    D1 = np.array([0.03, -0.01, 0.0, 0.0, 0.0], np.float32)
    cfg = _conv()
    for dists, D in ((None, None), ({6: D1}, D0)):
        bt, outs = run(cfg, B, idx, acts, cams={0: K1, 4: K2}, dists=dists, D0=D)
        bt.close()
        for b in range(B):   # a change of K (push 4, sequence 2) or of D (push 6, every sequence) starts the sequence over
            if b == 2 and acts[4][b] != SKIP:
                assert outs[4]["status"][b] == STARTED
        if dists:
            for b in range(B):
                if acts[6][b] != SKIP:
                    assert outs[6]["status"][b] == STARTED
        K_of = lambda k, b: (K1 if k < 4 else K2)[b]
        last = 6 if dists else len(idx)
        late = check_pairs(cfg, outs[:last], idx[:last], 3, seed=5, K_of=K_of, D=D)
        assert late > 0, "no pair was tracked against a keyframe older than the previous frame"


# ------------------------------------------------------------------------------------------------------------------------- 7
def test_start_pose():
    B = 6
    idx, acts = schedule(B, 10, seed=29)
    cfg = _conv()
    rng = np.random.RandomState(4)

    def given(k, outs):
        return (rng.normal(size=(B, 6)) * np.array([0.01] * 3 + [0.005] * 3)).astype(np.float32) if k > 0 else None
    rows_seen = {}

    def given_rec(k, outs):
        r = given(k, outs)
        rows_seen[k] = r
        return r
    bt, outs = run(cfg, B, idx, acts, mode=GIVEN, rows=given_rec)
    bt.close()
    kxi = np.zeros((B, 6), np.float32)
    for k, o in enumerate(outs):
        for b in range(B):
            if o["status"][b] == TRACKED and rows_seen.get(k) is not None:
                np.testing.assert_array_equal(o["start"][b], cat(-kxi[b], rows_seen[k][b]), err_msg="push %d seq %d" % (k, b))
            else:
                assert not np.any(o["start"][b])
            if o["status"][b] == STARTED:
                kxi[b] = 0
            elif o["status"][b] == TRACKED and o["key"][b]:
                kxi[b] = o["xw"][b]
    # CONSTANT_VELOCITY equals GIVEN fed the host model (world twists w1, w2 of the last two TRACKED / STARTED pushes since the start)
    bc, cv = run(cfg, B, idx, acts, mode=CV)
    bc.close()
    hist = [[] for _ in range(B)]

    def model(k, outs):
        if k > 0:
            o = outs[k - 1]
            for b in range(B):
                if o["status"][b] == STARTED:
                    hist[b] = [o["xw"][b].copy()]
                elif o["status"][b] == TRACKED:
                    hist[b] = [o["xw"][b].copy()] + hist[b][:1]
        r = np.full((B, 6), np.nan, np.float32)
        for b in range(B):
            if len(hist[b]) == 2:
                w1, w2 = hist[b]
                r[b] = cat(w1, cat(-w2, w1))
        return r
    bg, gv = run(cfg, B, idx, acts, mode=GIVEN, rows=model)
    bg.close()
    moved = 0
    for k, (x, y) in enumerate(zip(cv, gv)):
        for f in ("xi", "start", "xw", "key", "status"):
            np.testing.assert_array_equal(x[f], y[f], err_msg="push %d %s" % (k, f))
        assert x["logs"] == y["logs"], k
        moved += int(np.any(x["start"]))
    assert moved > 0
    bn, nn = run(cfg, B, idx, acts, mode=NONE)
    bn.close()
    for o in nn:
        assert not np.any(o["start"])


# ------------------------------------------------------------------------------------------------------------------------- 8
def test_errors_change_nothing():
    import ctypes as C
    L = dvo.lib()
    P = pool()
    bt = dvo.Batch(2, K640, 640, 480, 4, 1, cfg=_cfg())
    assert L.dvo_batch_world_poses(bt._p, None, None, None) == dvo.DVO_ERR_BAD_ARGUMENT   # plain sensor-depth batch: still refused
    assert L.dvo_batch_copy_world_poses_device(bt._p, None, None, None) == dvo.DVO_ERR_BAD_ARGUMENT
    assert L.dvo_batch_set_keyframe_tracking(None, 1) == dvo.DVO_ERR_BAD_ARGUMENT
    mb = dvo.MonoBatch(2, K640, 640, 480)
    assert L.dvo_batch_set_keyframe_tracking(mb._p, 1) == dvo.DVO_ERR_BAD_ARGUMENT
    mb.close()
    bt.set_keyframe_tracking(True)
    bt.set_keyframe_tracking(False)                       # back to frame to frame before the first push
    _push(bt, [0, 1], "device")
    assert L.dvo_batch_world_poses(bt._p, None, None, None) == dvo.DVO_ERR_BAD_ARGUMENT
    assert L.dvo_batch_set_keyframe_tracking(bt._p, 1) == dvo.DVO_ERR_NOT_READY
    bt.close()
    bt = dvo.Batch(2, K640, 640, 480, 4, 1, cfg=_cfg())
    bt.set_keyframe_tracking(True)
    assert L.dvo_batch_world_poses(bt._p, None, None, None) == dvo.DVO_ERR_NOT_READY
    t = [_dev(x[[0, 1]]) for x in (P["g"], P["d"], P["s"])]
    assert L.dvo_batch_prefetch_device(bt._p, C.c_void_p(t[0].data_ptr()), C.c_void_p(t[1].data_ptr()),
                                       C.c_void_p(t[2].data_ptr())) == dvo.DVO_ERR_NOT_READY
    _push(bt, [0, 1], "device")
    _push(bt, [2, 3], "device")
    ref = (bt.last_poses()[0].copy(), bt.world_poses()[0].copy(), bt.keyframe(0, 2))
    assert L.dvo_batch_set_keyframe_tracking(bt._p, 0) == dvo.DVO_ERR_NOT_READY
    assert L.dvo_batch_set_keyframe_tracking(bt._p, 1) == dvo.DVO_ERR_NOT_READY
    assert L.dvo_batch_prefetch_device(bt._p, C.c_void_p(t[0].data_ptr()), C.c_void_p(t[1].data_ptr()),
                                       C.c_void_p(t[2].data_ptr())) == dvo.DVO_ERR_NOT_READY
    buf = np.zeros((120, 160), np.float32)
    fpn = lambda a: a.ctypes.data_as(dvo.FP)
    for sg, ag in ((fpn(buf), None), (None, fpn(buf))):
        assert L.dvo_batch_keyframe_get(bt._p, 0, 2, fpn(buf), None, sg, ag, None, None, None, None) == dvo.DVO_ERR_BAD_ARGUMENT
    np.testing.assert_array_equal(bt.last_poses()[0], ref[0])
    np.testing.assert_array_equal(bt.world_poses()[0], ref[1])
    k = bt.keyframe(0, 2)
    np.testing.assert_array_equal(k["gray"], ref[2]["gray"]); np.testing.assert_array_equal(k["depth"], ref[2]["depth"])
    _push(bt, [4, 5], "device")                          # still pushes and tracks after the refused calls
    assert list(bt.last_status()) == [TRACKED, TRACKED]
    with pytest.raises(ValueError):
        bt.keyframe(0, 4)                                # a level outside the pyramid, refused before any buffer is sized
    ms, px = bt.probe_gn(3, 2)                           # the operands of the last track(): (last frame, keyframe)
    assert ms > 0 and px == 2 * 320 * 240
    bt.close()


# ------------------------------------------------------------------------------------------------------------------------- 9
# The workload was fixed before it was measured (0.01 m and 0.5 degrees per frame, converging constants).  Measured on an MI355X
# (DESIGN.md §19): mean error 0.00468 m frame to frame, 0.00498 m with keyframes, 2.44 frames per keyframe -- no gain on these noise-free
# renders.  The test pins what was measured, with margin: keyframe mode replaces the keyframe on fewer than every other frame and its
# world poses are no worse than the frame-to-frame composition by more than a quarter.
DRIFT_B, DRIFT_N, DRIFT_T, DRIFT_R_DEG = 8, 40, 0.01, 0.5
DRIFT_MARGIN = 1.25


def _smooth(seed=31):
    rng = np.random.RandomState(seed)
    out = []
    for _ in range(DRIFT_B):
        dt = rng.normal(size=3); dt *= DRIFT_T / np.linalg.norm(dt)
        dr = rng.normal(size=3); dr *= np.radians(DRIFT_R_DEG) / np.linalg.norm(dr)
        v = np.concatenate([dt, dr])
        P = [np.eye(4)]
        for k in range(1, DRIFT_N):
            P.append(P[-1] @ synth.se3_exp_np(min(1.0, k / 3.0) * v))
        out.append(P)
    return out


def drift(kf):
    """mean world-position error over every frame and sequence (m), and the mean number of frames per keyframe.  Both modes and the ground
    truth compose the same way: W_k = W_ref exp(rel_k) (the world twist of dvo_batch_world_poses, the mono rule), with ref the frame's
    keyframe (frame to frame: the previous frame) and the ground-truth relative pose inv(P_k) P_ref (bench.py's convention)"""
    import torch
    P = _smooth()
    g, d = synth.render_batch([P[b][k] for k in range(DRIFT_N) for b in range(DRIFT_B)], K640, 640, 480, device="cuda")
    g = g.reshape(DRIFT_N, DRIFT_B, 480, 640).contiguous(); d = d.reshape(DRIFT_N, DRIFT_B, 480, 640).contiguous()
    s = torch.full_like(d, 0.5)
    torch.cuda.synchronize()
    bt = dvo.Batch(DRIFT_B, K640, 640, 480, 4, 1, cfg=_conv())
    if kf:
        bt.set_keyframe_tracking(True)
    W = [np.eye(4) for _ in range(DRIFT_B)]; G = [np.eye(4) for _ in range(DRIFT_B)]
    Wk = [np.eye(4) for _ in range(DRIFT_B)]; Gk = [np.eye(4) for _ in range(DRIFT_B)]
    ref = [0] * DRIFT_B
    err, keys = [], 0
    for k in range(DRIFT_N):
        bt.push_device(g[k].data_ptr(), d[k].data_ptr(), s[k].data_ptr())
        if k == 0:
            continue
        xi, T = bt.last_poses()
        if kf:
            _, Tw, key = bt.world_poses()
        for b in range(DRIFT_B):
            Gb = Gk[b] @ (np.linalg.inv(P[b][k]) @ P[b][ref[b]])
            Wb = Tw[b].astype(np.float64) if kf else W[b] @ T[b].astype(np.float64)
            err.append(float(np.linalg.norm(Wb[:3, 3] - Gb[:3, 3])))
            if not kf:
                W[b] = Wb
                Gk[b] = Gb; ref[b] = k
            elif key[b]:
                keys += 1
                Gk[b] = Gb; ref[b] = k
    bt.close()
    return float(np.mean(err)), (DRIFT_B * (DRIFT_N - 1)) / max(1, keys)


def test_keyframe_drift_on_a_smooth_trajectory():
    f2f, _ = drift(False)
    kf, per_key = drift(True)
    print("drift over %d frames (mean world-position error m): frame to frame %.5f keyframes %.5f (%.2f frames per keyframe, ratio %.2f)"
          % (DRIFT_N, f2f, kf, per_key, f2f / kf))
    assert per_key > 2.0, per_key
    assert kf < DRIFT_MARGIN * f2f, (f2f, kf, per_key)
