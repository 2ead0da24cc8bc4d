"""Per-sequence camera intrinsics of a mono batch (dvo_batch_create_mono_cameras, include/dvo.h) on the GPU.

Every sequence of a mixed-camera mono batch must give the bits of a dvo_vo handle created with that sequence's K (and of a
one-camera mono batch) on the same frames: world poses, keyframe flags, the newest keyframe's maps and twist, and the track log.
One tile size throughout (gn_pixels_per_thread = 4), as tests/test_gpu_mono_batch.py."""
import ctypes as C
import functools

import numpy as np
import pytest

import dvo_amd as dvo
import orc
from dvo_amd import synth

pytestmark = pytest.mark.gpu


def _K(fx, fy, cx, cy, skew=0.0):
    return np.array([[fx, skew, cx], [0, fy, cy], [0, 0, 1]], np.float32)


# synth.K_640, the TUM fr1 RGB camera, one far from the others, and one with a skew term (K[0][1] != 0: depthEstimate's full K
# products instead of the sparse ones)
CAMS = [synth.K_640, _K(517.3, 516.5, 318.6, 255.3), _K(400.0, 400.0, 300.0, 260.0), _K(560.0, 555.0, 322.0, 236.0, skew=1.5)]
FAR = 2
N_RENDER = 6


def _cfg(**kw):
    return dvo.default_config(rng_seed=3, gn_pixels_per_thread=4, **kw)


@functools.lru_cache(maxsize=None)
def _render(cam):
    """N_RENDER frames of one trajectory rendered with camera `cam`: gray, depth (numpy) and the GT poses"""
    g, d, _, poses = synth.sequence(N_RENDER, K=CAMS[cam], seed=7, sigma_value=0.5)
    return g.numpy(), d.numpy(), poses


@functools.lru_cache(maxsize=None)
def _init_depth():
    """one initial depth map for every sequence (as tests/test_gpu_mono_batch.py: K_640's first depth, culled twice, plus noise)"""
    d0 = orc.cull_image(_render(0)[1][0], 2)
    return (d0 + np.random.RandomState(12).normal(0, 0.1, d0.shape)).astype(np.float32)


def _orders(B, n_frames):
    """per sequence the frame index at each step: small steps (mostly depth updates), larger ones (keyframes by translation) and a
    static stretch (keyframes by the frame-count rule), so both branches of Mapper::estimate are taken on the same step"""
    out = []
    for b in range(B):
        step, start = 1 + b % 3, (b // 4) % N_RENDER
        seq = [(start + step * k) % N_RENDER for k in range(n_frames)]
        if b % 4 == 3:
            seq = [seq[0]] * 3 + seq[3:]
        out.append(tuple(seq))
    return out


def _logbits(lg):
    return (tuple(lg["n_iter"]), tuple(np.asarray(r, np.float32).tobytes() for r in lg["residual"]),
            tuple(np.asarray(x, np.float32).tobytes() for x in lg["xi_after"]), tuple(np.asarray(v).tobytes() for v in lg["n_valid"]))


def _kfbits(kf):
    return tuple(np.asarray(kf[k], np.float32).tobytes() for k in ("gray", "depth", "sigma", "age", "xi"))


def _stack(cam, orders, k):
    return np.stack([_render(int(c))[0][o[k]] for c, o in zip(cam, orders)])


def _feed(mb, feed, g):
    import torch
    if feed.startswith("raw"):
        g8 = np.clip(np.rint(g * 255), 0, 255).astype(np.uint8)
        if feed == "raw_host":
            mb.odometrize_host(g8)
        else:
            t = torch.from_numpy(g8).cuda(); torch.cuda.synchronize()
            mb.odometrize_raw_device(t.data_ptr(), 1)
            mb.synchronize()
    elif feed == "host":
        mb.odometrize_host(np.ascontiguousarray(g))
    else:
        t = torch.from_numpy(np.ascontiguousarray(g)).cuda(); torch.cuda.synchronize()
        mb.odometrize_device(t.data_ptr())
        mb.synchronize()


def _run_mono(cfg, cam, orders, n_frames, per_camera=True, shared_K=synth.K_640, feed="device", seqs=None):
    """A mono batch over the sequences, sequence q on frames rendered with camera cam[q] (per_camera: created with K = CAMS[cam[q]];
    else with shared_K for all).  Per frame, per sequence of `seqs`: (T_world, is_keyframe, keyframe bits, track-log bits from
    frame 1 on)."""
    B = len(cam)
    K = np.stack([CAMS[int(c)] for c in cam]) if per_camera else shared_K
    mb = dvo.MonoBatch(B, K, 640, 480, cfg=cfg, per_sequence_K=per_camera)
    init = _init_depth()
    mb.setInitialDepth(init, np.full_like(init, 0.5))
    seqs = list(range(B)) if seqs is None else list(seqs)
    out = []
    for k in range(n_frames):
        _feed(mb, feed, _stack(cam, orders, k))
        _, T, key = mb.world_poses()
        out.append([(T[q].copy(), bool(key[q]), _kfbits(mb.keyframe(q)), _logbits(mb.last_track_log(q)) if k else None) for q in seqs])
    mb.close()
    return out


@functools.lru_cache(maxsize=None)
def _vo(c, order):
    """a dvo_vo handle created with camera c on one sequence's frames: per frame (T_world, is_keyframe, keyframe bits, log bits)"""
    vo = dvo.VisualOdometry(CAMS[c], 640, 480, cfg=_cfg())
    init = _init_depth()
    vo.setInitialDepth(init, np.full_like(init, 0.5))
    res = []
    for k, i in enumerate(order):
        T, key = vo.odometrize(_render(c)[0][i])
        kf = vo.keyframe(vo.keyframeCount() - 1)
        res.append((np.asarray(T, np.float32).copy(), bool(key), _kfbits(kf), _logbits(vo.lastTrackLog()) if k else None))
    vo.close()
    return res


def _one_camera(cfg, cam, orders, n_frames, feed="device", seqs=None):
    """The same sequences run as one mono batch per camera (dvo_batch_create_mono with that K), reassembled in batch order."""
    B = len(cam)
    seqs = list(range(B)) if seqs is None else list(seqs)
    res = {}
    for c in sorted(set(int(x) for x in cam)):
        members = [q for q in range(B) if int(cam[q]) == c]
        want = [j for j, q in enumerate(members) if q in seqs]
        o = _run_mono(cfg, [c] * len(members), [orders[q] for q in members], n_frames, per_camera=False, shared_K=CAMS[c], feed=feed,
                      seqs=want)
        for w, j in enumerate(want):
            res[members[j]] = [o[k][w] for k in range(n_frames)]
    return [[res[q][k] for q in seqs] for k in range(n_frames)]


def _assert_same(got, ref, seqs, what):
    n_key = n_upd = 0
    for k in range(len(got)):
        for j, q in enumerate(seqs):
            T, key, kf, lb = got[k][j]
            T1, key1, kf1, lb1 = ref[k][j]
            assert key == key1, (what, "frame", k, "seq", q)
            np.testing.assert_array_equal(T, T1, err_msg="%s: pose of sequence %d frame %d" % (what, q, k))
            assert kf == kf1, (what, "keyframe maps / twist", k, q)
            assert lb == lb1, (what, "track log", k, q)
            if k:
                n_key += int(key); n_upd += int(not key)
    return n_key, n_upd


VARIANTS = ["default", "track_adaptive=-1", "B=6", "track_fused_tiles=8", "gn_use_lds_patch=1", "track_streams=2"]


@pytest.mark.parametrize("variant", VARIANTS)
def test_mixed_cameras_equal_single_handles(variant):
    B = 6 if variant == "B=6" else 12   # B=6: one launch per iteration (k_track_gn_fused) on the levels that fit it
    cfg = _cfg() if "=" not in variant or variant == "B=6" else _cfg(**{variant.split("=")[0]: int(variant.split("=")[1])})
    n_frames = 8
    cam = [q % len(CAMS) for q in range(B)]
    orders = _orders(B, n_frames)
    got = _run_mono(cfg, cam, orders, n_frames)
    if variant == "gn_use_lds_patch=1":
        # (another tile kernel, k_track_gn_tile, which the single handle's one-launch tracker does not use: one-camera batches instead)
        ref = _one_camera(cfg, cam, orders, n_frames)
    else:
        ref = [[_vo(int(cam[q]), orders[q])[k] for q in range(B)] for k in range(n_frames)]
    n_key, n_upd = _assert_same(got, ref, range(B), variant)
    assert n_key >= B // 2 and n_upd >= B // 2, (n_key, n_upd)   # keyframes were created and depth updates ran


def test_uniform_table_is_the_plain_handle():
    B, n_frames = 12, 6
    cam = [0] * B
    orders = _orders(B, n_frames)
    plain = _run_mono(_cfg(), cam, orders, n_frames, per_camera=False)
    table = _run_mono(_cfg(), cam, orders, n_frames, per_camera=True)
    _assert_same(table, plain, range(B), "uniform table")


@pytest.mark.parametrize("feed", ["device", "raw_device", "host", "raw_host"])
def test_feeds_match_one_camera_batches(feed):
    B, n_frames = 8, 6
    cam = [(q * 3) % len(CAMS) for q in range(B)]
    orders = _orders(B, n_frames)
    got = _run_mono(_cfg(), cam, orders, n_frames, feed=feed)
    _assert_same(got, _one_camera(_cfg(), cam, orders, n_frames, feed=feed), range(B), feed)


def test_scale_1024_sequences():
    """1 024 sequences on 4 cameras against four one-camera batches of 256: every world pose and keyframe flag, and the keyframe maps
    and track logs of a sample.  Frames are gathered on the device (raw u8) to keep the host out of it."""
    import torch
    B, n_frames = 1024, 4
    cam = np.array([q % len(CAMS) for q in range(B)])
    orders = np.array(_orders(B, n_frames))
    sample = sorted(np.random.RandomState(16).choice(B, 16, replace=False).tolist())
    lib8 = torch.from_numpy(np.stack([np.clip(np.rint(_render(c)[0] * 255), 0, 255).astype(np.uint8) for c in range(len(CAMS))])).cuda()

    def run(K, members):
        mb = dvo.MonoBatch(len(members), K, 640, 480, cfg=_cfg(), per_sequence_K=K.ndim == 3)
        init = _init_depth()
        mb.setInitialDepth(init, np.full_like(init, 0.5))
        cm = torch.from_numpy(cam[members]).cuda()
        poses, keys, detail = [], [], []
        for k in range(n_frames):
            fr = lib8[cm, torch.from_numpy(orders[members, k]).cuda()].contiguous()
            torch.cuda.synchronize()
            mb.odometrize_raw_device(fr.data_ptr(), 1)
            _, T, key = mb.world_poses()
            poses.append(T.copy()); keys.append(key.copy())
            detail.append({int(members[j]): (_kfbits(mb.keyframe(j)), _logbits(mb.last_track_log(j)) if k else None)
                           for j in range(len(members)) if int(members[j]) in sample})
            del fr
        mb.close()
        return poses, keys, detail

    all_q = np.arange(B)
    P, Kf, D = run(np.stack([CAMS[c] for c in cam]), all_q)
    for c in range(len(CAMS)):
        members = all_q[cam == c]
        P1, K1, D1 = run(CAMS[c], members)
        for k in range(n_frames):
            np.testing.assert_array_equal(P[k][members], P1[k], err_msg="camera %d frame %d" % (c, k))
            np.testing.assert_array_equal(Kf[k][members], K1[k])
            for q, v in D1[k].items():
                assert D[k][q] == v, (c, k, q)
    assert 0 < sum(int(Kf[k].sum()) for k in range(1, n_frames)) < B * (n_frames - 1)   # both branches of the mapper ran


# Bound on the far camera's world-pose translation error (m) over the frames, with ground-truth initial depth.  Measured on an
# MI355X: 8.4e-4 m with the per-sequence K, 5.7e-3 m with the shared K_640 on the same frames; the test asks
# for < RIGHT_K_BOUND and > 2.5 x RIGHT_K_BOUND respectively.
RIGHT_K_BOUND = 1.5e-3


# The bench's converging constants (as tests/test_gpu_batch_cameras.py::test_the_right_K_matters): the update is the Gauss-Newton
# step, so the pose error measures the model -- here the intrinsics -- not the over-relaxed iteration.
def _converging_cfg():
    return _cfg(step_default=1.0, step_level1=0.75, step_level2=0.5, min_residual=0.0)


def _far_errors(per_camera):
    import torch
    B, n_frames = 8, N_RENDER
    cam = np.array([0, FAR] * (B // 2))
    poses = _render(FAR)[2]
    init = np.stack([orc.cull_image(_render(int(c))[1][0], 2) for c in cam]).astype(np.float32)
    sig = np.full_like(init, 0.5)
    K = np.stack([CAMS[int(c)] for c in cam]) if per_camera else CAMS[0]
    mb = dvo.MonoBatch(B, K, 640, 480, cfg=_converging_cfg(), per_sequence_K=per_camera)
    ti, ts = torch.from_numpy(init).cuda(), torch.from_numpy(sig).cuda()
    torch.cuda.synchronize()
    mb.setInitialDepthDevice(ti.data_ptr(), ts.data_ptr())
    errs = []
    for k in range(n_frames):
        t = torch.from_numpy(np.stack([_render(int(c))[0][k] for c in cam])).cuda(); torch.cuda.synchronize()
        mb.odometrize_device(t.data_ptr())
        _, T, _ = mb.world_poses()
        if k:
            gt = np.linalg.inv(poses[k]) @ poses[0]          # camera k <- camera 0
            for q in np.flatnonzero(cam == FAR):
                E = T[q].astype(np.float64) @ np.linalg.inv(gt)
                errs.append(float(np.linalg.norm(E[:3, 3])) if np.isfinite(E).all() else np.inf)
    mb.close()
    return max(errs)


def test_the_right_K_matters():
    right, shared = _far_errors(True), _far_errors(False)
    print("far camera: max world translation error per-camera K %.3g m, shared K_640 %.3g m" % (right, shared))
    assert right < RIGHT_K_BOUND, (right, shared)
    assert shared > 2.5 * RIGHT_K_BOUND, (right, shared)


def test_errors():
    L = dvo.lib()
    Ks = np.stack([CAMS[c] for c in (0, 1, 2, 3)])
    for bad, q in (("nan", 2), ("fx0", 1), ("fy-", 3)):
        K = Ks.copy()
        if bad == "nan":
            K[q, 1, 2] = np.nan
        elif bad == "fx0":
            K[q, 0, 0] = 0.0
        else:
            K[q, 1, 1] = -400.0
        p = C.c_void_p()
        assert L.dvo_batch_create_mono_cameras(4, K.ctypes.data_as(C.c_void_p), 640, 480, 8, None, C.byref(p)) == 1, bad
        assert not p.value
        assert ("sequence %d" % q) in L.dvo_last_error().decode(), bad
    mb = dvo.MonoBatch(4, Ks, 640, 480, per_sequence_K=True)
    K9 = np.zeros((4, 9), np.float32)
    assert L.dvo_batch_set_intrinsics(mb._p, Ks.ctypes.data_as(C.c_void_p)) == 1
    assert L.dvo_batch_get_intrinsics(mb._p, K9.ctypes.data_as(C.c_void_p)) == 1
    acts = np.full(4, dvo.SEQ_TRACK, np.uint8)
    assert L.dvo_batch_set_actions(mb._p, acts.ctypes.data_as(C.c_void_p), 0) == 1
    mb.close()
