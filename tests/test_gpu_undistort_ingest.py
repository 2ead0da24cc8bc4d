"""Lens undistortion fused into the mono ingest (dvo_batch_set_distortion, dvo_vo_set_distortion, include/dvo.h) on the GPU.

A handle with D must give, bit for bit, what a plain handle with the same K, config and initial depth gives when it is fed
dvo_op_undistort(ingest(frame), K, D): world poses, keyframe flags, the newest keyframe's maps at every level and the mono stats
(dvo_vo: also the track log).  Frames at 640x480 with the reference's webcam camera (K_LOGICOOL, D_LOGICOOL) and a strong D (TUM
fr1) whose border and folds really occur.  One tile size throughout (gn_pixels_per_thread = 4), as tests/test_gpu_mono_batch.py."""
import ctypes as C
import functools

import numpy as np
import pytest

import dvo_amd as dvo
import orc
from dvo_amd import synth
from real_data import D_LOGICOOL, K_LOGICOOL

pytestmark = pytest.mark.gpu

D_TUM = np.array([0.2624, -0.9531, -0.0054, 0.0026, 1.1633], np.float32)   # TUM fr1 RGB camera
D_ZERO = np.zeros(5, np.float32)
N_RENDER = 6
N_FRAMES = 12
LEVELS = 3


def _K(fx, fy, cx, cy):
    return np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], np.float32)


CAMS = [K_LOGICOOL, _K(517.3, 516.5, 318.6, 255.3), _K(525.0, 525.0, 319.5, 239.5), _K(560.0, 555.0, 322.0, 236.0)]


def _cfg(**kw):
    return dvo.default_config(rng_seed=3, gn_pixels_per_thread=4, **kw)


@functools.lru_cache(maxsize=None)
def _render():
    """N_RENDER frames of one trajectory (the input the handles are fed: for the equality tests any image is a 'distorted' frame)"""
    g, d, _, poses = synth.sequence(N_RENDER, K=K_LOGICOOL, seed=7, sigma_value=0.5)
    return g.numpy(), d.numpy(), poses


@functools.lru_cache(maxsize=None)
def _init_depth():
    d0 = orc.cull_image(_render()[1][0], 2)
    return (d0 + np.random.RandomState(12).normal(0, 0.1, d0.shape)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _u8(i):
    return np.clip(np.rint(_render()[0][i] * 255), 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def _rgb(i, ch):
    """a raw frame with `ch` channels whose colour channels differ (so the fixed-point luma is exercised)"""
    g = _u8(i).astype(np.int32)
    if ch == 1:
        return g.astype(np.uint8)
    chans = [g, (g * 7 + 31) % 256, 255 - g] + ([(g * 3) % 256] if ch == 4 else [])
    return np.stack(chans, -1).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def _undist(i, cam, D_bytes, ch=0):
    """dvo_op_undistort of frame i (ch > 0: of dvo_op_ingest of its raw form) with camera `cam`"""
    src = _render()[0][i] if ch == 0 else dvo.ingest(_rgb(i, ch))
    return dvo.undistort(src, CAMS[cam], np.frombuffer(D_bytes, np.float32))


def _orders(B):
    out = []
    for b in range(B):
        step, start = 1 + b % 3, (b // 4) % N_RENDER
        seq = [(start + step * k) % N_RENDER for k in range(N_FRAMES)]
        if b % 4 == 3:
            seq = [seq[0]] * 3 + seq[3:]
        out.append(tuple(seq))
    return out


def _state(mb, B):
    """per sequence: (T_world, is_keyframe, keyframe bits at every level, mono stats)"""
    _, T, key = mb.world_poses()
    out = []
    for q in range(B):
        kb = []
        for lv in range(LEVELS):
            kf = mb.keyframe(q, lv)
            kb.append(tuple(np.asarray(kf[k], np.float32).tobytes() for k in ("gray", "depth", "sigma", "xi")
                            ) + ((kf["age"].tobytes(),) if kf["age"] is not None else ()) + ((kf["id"], kf["n_keyframes"], kf["valid_updates"]),))
        out.append((T[q].tobytes(), bool(key[q]), tuple(kb), tuple(sorted(mb.stats(q).items()))))
    return out


def _device_feed(mb, arr, raw_ch=0):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(arr)).cuda()
    torch.cuda.synchronize()
    if raw_ch:
        mb.odometrize_raw_device(t.data_ptr(), raw_ch)
    else:
        mb.odometrize_device(t.data_ptr())
    mb.synchronize()


def _host_feed(mb, arr, ch, pinned):
    import torch
    a = np.ascontiguousarray(arr)
    if not pinned:
        mb.odometrize_host(a)
        return
    t = torch.from_numpy(a).pin_memory()
    dvo._check(dvo.lib().dvo_batch_odometrize_raw_host(mb._p, C.c_void_p(t.data_ptr()), ch))
    mb.synchronize()


def _new_batch(B, K, per_camera=False, D=None):
    mb = dvo.MonoBatch(B, K, 640, 480, cfg=_cfg(), per_sequence_K=per_camera)
    init = _init_depth()
    mb.setInitialDepth(init, np.full_like(init, 0.5))
    if D is not None:
        mb.set_distortion(D)
    return mb


def _run(mb, frames_of_step):
    B = mb.n_seq
    res = []
    for k in range(N_FRAMES):
        frames_of_step(mb, k)
        res.append(_state(mb, B))
    mb.close()
    return res


def _branches(res):
    """(keyframes created after frame 0, depth updates) over all sequences and frames"""
    keys = sum(1 for k in range(1, len(res)) for s in res[k] if s[1])
    upd = sum(1 for k in range(1, len(res)) for s in res[k] if not s[1])
    return keys, upd


@functools.lru_cache(maxsize=None)
def _plain_float(B, D_bytes):
    """the definition: a plain batch fed dvo_op_undistort'ed float frames"""
    orders = _orders(B)
    mb = _new_batch(B, K_LOGICOOL)
    return _run(mb, lambda m, k: _device_feed(m, np.stack([_undist(o[k], 0, D_bytes) for o in orders])))


@pytest.mark.parametrize("D", [D_LOGICOOL, D_TUM], ids=["logicool", "tum"])
def test_float_device_equals_undistorted_plain_batch(D):
    B = 8
    orders = _orders(B)
    ref = _plain_float(B, D.tobytes())
    mb = _new_batch(B, K_LOGICOOL, D=D)
    got = _run(mb, lambda m, k: _device_feed(m, np.stack([_render()[0][o[k]] for o in orders])))
    for k in range(N_FRAMES):
        for q in range(B):
            assert got[k][q] == ref[k][q], ("frame", k, "sequence", q)
    keys, upd = _branches(got)
    assert keys > 0 and upd > 0, (keys, upd)
    # and the undistortion does something: the plain handle fed the distorted frames differs
    plain = _run(_new_batch(B, K_LOGICOOL), lambda m, k: _device_feed(m, np.stack([_render()[0][o[k]] for o in orders])))
    assert any(plain[k][q][0] != got[k][q][0] for k in range(1, N_FRAMES) for q in range(B))


@functools.lru_cache(maxsize=None)
def _plain_ingested(B, D_bytes, ch):
    orders = _orders(B)
    mb = _new_batch(B, K_LOGICOOL)
    return _run(mb, lambda m, k: _device_feed(m, np.stack([_undist(o[k], 0, D_bytes, ch) for o in orders])))


@pytest.mark.parametrize("ch", [1, 3, 4])
@pytest.mark.parametrize("feed", ["raw_device", "raw_host_pinned", "raw_host_pageable"])
def test_raw_frames_equal_the_float_path(ch, feed):
    B = 4
    orders = _orders(B)
    ref = _plain_ingested(B, D_TUM.tobytes(), ch)
    mb = _new_batch(B, K_LOGICOOL, D=D_TUM)

    def step(m, k):
        arr = np.stack([_rgb(o[k], ch) for o in orders])
        if feed == "raw_device":
            _device_feed(m, arr, raw_ch=ch)
        else:
            _host_feed(m, arr, ch, pinned=feed.endswith("pinned"))
    got = _run(mb, step)
    for k in range(N_FRAMES):
        for q in range(B):
            assert got[k][q] == ref[k][q], (feed, ch, "frame", k, "sequence", q)


def test_per_sequence_cameras_and_distortion():
    # sequences 1 and 4 share (K, D): one table for both; sequence 2 has an all-zero D (still applied)
    cam = [0, 1, 2, 3, 1, 1]
    D = np.stack([D_LOGICOOL, D_TUM, D_ZERO, np.array([-0.1, 0.05, 0.001, -0.002, 0.0], np.float32), D_TUM, D_LOGICOOL])
    B = len(cam)
    orders = _orders(B)
    mb = dvo.MonoBatch(B, np.stack([CAMS[c] for c in cam]), 640, 480, cfg=_cfg(), per_sequence_K=True)
    init = _init_depth()
    mb.setInitialDepth(init, np.full_like(init, 0.5))
    mb.set_distortion(D)
    got_D, en = mb.distortion()
    assert en and got_D.tobytes() == D.tobytes()
    got = _run(mb, lambda m, k: _device_feed(m, np.stack([_render()[0][o[k]] for o in orders])))
    for q in range(B):
        one = _new_batch(1, CAMS[cam[q]])
        ref = _run(one, lambda m, k: _device_feed(m, _undist(orders[q][k], cam[q], D[q].tobytes())[None]))
        for k in range(N_FRAMES):
            assert got[k][q] == ref[k][0], ("frame", k, "sequence", q)
    keys, upd = _branches(got)
    assert keys > 0 and upd > 0, (keys, upd)


def _vo_run(D, frames, raw):
    vo = dvo.VisualOdometry(K_LOGICOOL, 640, 480, cfg=_cfg())
    init = _init_depth()
    vo.setInitialDepth(init, np.full_like(init, 0.5))
    if D is not None:
        vo.setDistortion(D)
    res = []
    for k, f in enumerate(frames):
        T, key = vo.odometrizeRaw(f) if raw else vo.odometrize(f)
        kf = vo.keyframe(vo.keyframeCount() - 1)
        lg = vo.lastTrackLog() if k else None
        res.append((np.asarray(T, np.float32).tobytes(), bool(key),
                    tuple(np.asarray(kf[n], np.float32).tobytes() for n in ("gray", "depth", "sigma", "age", "xi")),
                    None if lg is None else (tuple(lg["n_iter"]), tuple(np.asarray(r, np.float32).tobytes() for r in lg["residual"]))))
    vo.close()
    return res


@pytest.mark.parametrize("stage", ["1", "0"], ids=["staged", "dma"])
def test_dvo_vo_equals_plain_and_batch(stage, monkeypatch):
    monkeypatch.setenv("DVO_MONO_STAGE", stage)   # (read per handle)
    order = _orders(1)[0]
    D = D_TUM
    ref = _vo_run(None, [_undist(i, 0, D.tobytes()) for i in order], raw=False)
    got_f = _vo_run(D, [_render()[0][i] for i in order], raw=False)
    got_r = _vo_run(D, [_u8(i) for i in order], raw=True)
    ref_r = _vo_run(None, [_undist(i, 0, D.tobytes(), 1) for i in order], raw=False)
    for k in range(N_FRAMES):
        assert got_f[k] == ref[k], ("float", k)
        assert got_r[k] == ref_r[k], ("raw", k)
    # ... and the one-sequence batch with the same D: the same poses, flags and newest keyframe's top-level maps
    mb = _new_batch(1, K_LOGICOOL, D=D)
    for k, i in enumerate(order):
        _device_feed(mb, _render()[0][i][None])
        _, T, key = mb.world_poses()
        kf = mb.keyframe(0, 2)
        assert T[0].tobytes() == got_f[k][0] and bool(key[0]) == got_f[k][1], k
        assert tuple(np.asarray(kf[n], np.float32).tobytes() for n in ("gray", "depth", "sigma", "age", "xi")) == got_f[k][2], k
    monkeypatch.delenv("DVO_MONO_STAGE", raising=False)
    mb.close()


def test_lifecycle_and_errors():
    L = dvo.lib()
    B = 3
    frames = [np.stack([_render()[0][(i + q) % N_RENDER] for q in range(B)]) for i in range(4)]
    # NULL before the first frame: the plain handle, bit for bit
    a = _new_batch(B, K_LOGICOOL, D=D_TUM)
    a.set_distortion(None)
    got_D, en = a.distortion()
    assert not en and not got_D.any()
    b = _new_batch(B, K_LOGICOOL)
    for f in frames:
        _device_feed(a, f); _device_feed(b, f)
        assert _state(a, B) == _state(b, B)
    a.close(); b.close()
    # after the first frame: NOT_READY, nothing changes
    a = _new_batch(B, K_LOGICOOL, D=D_LOGICOOL)
    c = _new_batch(B, K_LOGICOOL, D=D_LOGICOOL)
    _device_feed(a, frames[0]); _device_feed(c, frames[0])
    d = D_TUM.copy()
    assert L.dvo_batch_set_distortion(a._p, d.ctypes.data_as(C.c_void_p), 0) == 5      # DVO_ERR_NOT_READY
    assert L.dvo_batch_set_distortion(a._p, None, 0) == 5
    got_D, en = a.distortion()
    assert en and (got_D == D_LOGICOOL[None]).all()
    for f in frames[1:]:
        _device_feed(a, f); _device_feed(c, f)
        assert _state(a, B) == _state(c, B)
    a.close(); c.close()
    # a non-finite coefficient: BAD_ARGUMENT naming the sequence, nothing changes
    a = _new_batch(B, K_LOGICOOL)
    bad = np.stack([D_LOGICOOL] * B)
    bad[2, 3] = np.nan
    assert L.dvo_batch_set_distortion(a._p, bad.ctypes.data_as(C.c_void_p), 1) == 1
    assert "sequence 2" in L.dvo_last_error().decode()
    one = D_LOGICOOL.copy(); one[0] = np.inf
    assert L.dvo_batch_set_distortion(a._p, one.ctypes.data_as(C.c_void_p), 0) == 1
    assert "sequence 0" in L.dvo_last_error().decode()
    assert not a.distortion()[1]
    a.close()
    # a sensor-depth batch refuses
    sb = dvo.Batch(2, synth.K_640, 640, 480)
    assert L.dvo_batch_set_distortion(sb._p, D_TUM.ctypes.data_as(C.c_void_p), 0) == 1
    assert L.dvo_batch_get_distortion(sb._p, None, None) == 1
    sb.close()
    # dvo_vo with D refuses the sensor-depth entry points and init_keyframe; without frames D can be changed
    vo = dvo.VisualOdometry(K_LOGICOOL, 640, 480)
    vo.setDistortion(D_LOGICOOL)
    vo.setDistortion(D_TUM)
    g = _render()[0][0]; dep = _render()[1][0]; sg = np.full_like(dep, 0.1)
    T = np.zeros(16, np.float32)
    gp, dp, sp = (x.ctypes.data_as(C.c_void_p) for x in (g, dep, sg))
    assert L.dvo_vo_odometrize_depth(vo._p, gp, dp, sp, T.ctypes.data_as(C.c_void_p)) == 1
    d16 = np.zeros((480, 640), np.uint16)
    assert L.dvo_vo_odometrize_depth_raw(vo._p, _u8(0).ctypes.data_as(C.c_void_p), 1, d16.ctypes.data_as(C.c_void_p), C.c_float(0.0002),
                                         T.ctypes.data_as(C.c_void_p)) == 1
    assert L.dvo_vo_init_keyframe(vo._p, gp, dp, sp) == 1
    vo.odometrize(g)
    with pytest.raises(dvo.DvoError, match="NOT_READY|not ready|consumed"):
        vo.setDistortion(D_LOGICOOL)
    vo.close()
    # a plain dvo_vo that took a depth frame can no longer be given D
    vo = dvo.VisualOdometry(K_LOGICOOL, 640, 480)
    vo.odometrizeUsingDepth(g, dep, sg)
    assert L.dvo_vo_set_distortion(vo._p, D_TUM.ctypes.data_as(C.c_void_p)) == 5
    vo.close()


# ---------------------------------------------------------------- what a missing D costs
def _distort_frames(gray, K, D, iters=20):
    """Distorted images of pinhole renders: output pixel p_d shows the scene point of the undistorted pixel p_u with
    distort(p_u) = p_d, found by fixed-point iteration (as cv::undistortPoints) and sampled bilinearly from the pinhole render."""
    import torch
    n, h, w = gray.shape
    fx, fy, cx, cy = (float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2]))
    k1, k2, p1, p2, k3 = (float(x) for x in D)
    v, u = torch.meshgrid(torch.arange(h, dtype=torch.float64), torch.arange(w, dtype=torch.float64), indexing="ij")
    xd, yd = (u - cx) / fx, (v - cy) / fy
    x, y = xd.clone(), yd.clone()
    for _ in range(iters):
        r2 = x * x + y * y
        rad = 1 + r2 * (k1 + r2 * (k2 + r2 * k3))
        dx = 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
        dy = p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
        x, y = (xd - dx) / rad, (yd - dy) / rad
    gx = (x * fx + cx) / (w - 1) * 2 - 1
    gy = (y * fy + cy) / (h - 1) * 2 - 1
    grid = torch.stack([gx, gy], -1).float()[None].expand(n, h, w, 2)
    img = torch.from_numpy(gray)[:, None]
    out = torch.nn.functional.grid_sample(img, grid, mode="bilinear", padding_mode="border", align_corners=True)[:, 0]
    return np.clip(np.rint(out.numpy() * 255), 0, 255).astype(np.uint8)


def _converging_cfg():
    return _cfg(step_default=1.0, step_level1=0.75, step_level2=0.5, min_residual=0.0)


def _trajectory_error(with_D, n=N_RENDER):
    import torch
    g, d, poses = _render()
    raw = _distort_frames(g, K_LOGICOOL, D_TUM)
    mb = dvo.MonoBatch(1, K_LOGICOOL, 640, 480, cfg=_converging_cfg())
    init = orc.cull_image(d[0], 2).astype(np.float32)                  # ground-truth initial depth: mono scale anchored
    mb.setInitialDepth(init, np.full_like(init, 0.5))                  # (sigma 0.5: the update is the Gauss-Newton step)
    if with_D:
        mb.set_distortion(D_TUM)
    errs = []
    for k in range(n):
        t = torch.from_numpy(raw[k][None].copy()).cuda(); torch.cuda.synchronize()
        mb.odometrize_raw_device(t.data_ptr(), 1)
        _, T, _ = mb.world_poses()
        if k:
            gt = np.linalg.inv(poses[k]) @ poses[0]                      # camera k <- camera 0
            E = T[0].astype(np.float64) @ np.linalg.inv(gt)
            errs.append(float(np.linalg.norm(E[:3, 3])) if np.isfinite(E).all() else np.inf)
    mb.close()
    return max(errs)


# measured on an MI355X: 1.28e-3 m with set_distortion, 2.22e-3 m without (ratio 0.58; the run is deterministic, and
# the margin leaves room for the remaining error of the 8-bit, bilinear-resampled distorted frames and the nearest remap)
def test_a_missing_D_costs_accuracy():
    right, missing = _trajectory_error(True), _trajectory_error(False)
    print("strong D (TUM fr1): max world translation error with set_distortion %.3g m, without %.3g m" % (right, missing))
    assert right < 0.75 * missing, (right, missing)
