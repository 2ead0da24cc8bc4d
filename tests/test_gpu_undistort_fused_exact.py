"""The undistortion fused into frame ingest, bit for bit against the float64 camera model (tests/real_data.py:undistort_index_np)
rather than against dvo_op_undistort, which runs the same undistort_source on the same device.

Mono (k_undistort_map + k_pyramid_remap / k_pyramid_remap_plan): the newest keyframe's gray at every level, after the first frame
and after every frame that makes a new keyframe, equals the oracle's pyramid (orc.OFrame(., 3, 2)) of the numpy-undistorted frame
with an INVALID (-2) border.  Sensor depth (k_pyramid_remap_depth), which has no map readout: a batch with per-sequence K and D
gives the poses, status and track logs of a plain batch with the same K fed the numpy-undistorted gray, depth and sigma."""
import functools

import numpy as np
import pytest

import dvo_amd as dvo
import orc
from dvo_amd import synth
from lockstep import raw_gray
from real_data import D_LOGICOOL, K_LOGICOOL, ingest_np, undistort_index_np
from undistort_sweep import D_TUM, D_of, K_of

pytestmark = pytest.mark.gpu

SKIP, TRACK = dvo.SEQ_SKIP, dvo.SEQ_TRACK
SKIPPED = dvo.SEQ_SKIPPED
LEVELS = 3
N_RENDER = 6
N_FRAMES = 10

# six sequences, each with its own camera and its own D
MONO_K = [K_LOGICOOL, K_of(517.3, 516.5, 318.6, 255.3), K_of(525.0, 525.0, 319.5, 239.5), K_of(560.0, 555.0, 322.0, 236.0),
          K_of(600.0, 590.0, 300.0, 250.0), K_of(500.0, 520.0, 330.5, 230.5)]
MONO_D = [D_LOGICOOL, D_TUM, D_of(k1=-0.1, k2=0.05, p1=0.001, p2=-0.002), D_of(k1=-0.3, k2=0.1),
          D_of(p1=0.01, p2=-0.008), D_of(k1=0.2, p2=0.003, k3=-0.1)]


def _undistort_np(img, K, D):
    """nearest remap by the reference's source index, border INVALID (-2)"""
    h, w = img.shape
    idx = undistort_index_np(K, D, w, h)
    out = np.full((h, w), -2.0, np.float32)
    out[idx >= 0] = img.reshape(-1)[idx[idx >= 0]]
    return out


def _assert_bits(got, exp, where):
    got = np.asarray(got, np.float32); exp = np.asarray(exp, np.float32)
    assert got.shape == exp.shape, (where, got.shape, exp.shape)
    bad = got.view(np.uint32) != exp.view(np.uint32)
    if bad.any():
        ys, xs = np.nonzero(bad)
        y, x = int(ys[0]), int(xs[0])
        raise AssertionError("%s: %d pixel(s) differ, first at (x=%d, y=%d): GPU %r, reference %r"
                             % (where, int(bad.sum()), x, y, float(got[y, x]), float(exp[y, x])))


# ---------------------------------------------------------------- mono
@functools.lru_cache(maxsize=None)
def _mono_render():
    g, d, _, _ = synth.sequence(N_RENDER, K=K_LOGICOOL, seed=7, sigma_value=0.5)
    return g.numpy(), d.numpy()


@functools.lru_cache(maxsize=None)
def _init_depth():
    d0 = orc.cull_image(_mono_render()[1][0], 2)
    return (d0 + np.random.RandomState(12).normal(0, 0.1, d0.shape)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _rgb(i, ch):
    g = np.clip(np.rint(_mono_render()[0][i] * 255), 0, 255).astype(np.int32)
    if ch == 1:
        return g.astype(np.uint8)
    return np.stack([g, (g * 7 + 31) % 256, 255 - g] + ([(g * 3) % 256] if ch == 4 else []), -1).astype(np.uint8)


def _gray_of(i, ch):
    """the float gray the library ingests: the render (ch = 0) or k_ingest of the raw frame"""
    return _mono_render()[0][i] if ch == 0 else raw_gray(_rgb(i, ch))


@functools.lru_cache(maxsize=None)
def _ref_pyramid(i, ch, K_bytes, D_bytes):
    K = np.frombuffer(K_bytes, np.float32).reshape(3, 3)
    D = np.frombuffer(D_bytes, np.float32)
    fr = orc.OFrame(_undistort_np(_gray_of(i, ch), K, D), None, None, K, LEVELS, 2)
    return tuple(fr.gray(l) for l in range(LEVELS))


def _orders(B):
    out = []
    for b in range(B):
        step, start = 1 + b % 3, (b // 3) % N_RENDER
        out.append([(start + step * k) % N_RENDER for k in range(N_FRAMES)])
    return out


def _mono_feed(mb, arr, feed, ch):
    import torch
    if feed == "device":
        t = torch.from_numpy(np.ascontiguousarray(arr)).cuda()
        torch.cuda.synchronize()
        if ch:
            mb.odometrize_raw_device(t.data_ptr(), ch)
        else:
            mb.odometrize_device(t.data_ptr())
        mb.synchronize()
    else:
        mb.odometrize_host(arr)


@pytest.mark.parametrize("feed,ch,planned", [("device", 0, False), ("device", 0, True),
                                             ("device", 1, False), ("device", 3, False), ("device", 4, True),
                                             ("host", 1, False), ("host", 3, True), ("host", 4, False)],
                         ids=["float_device", "float_device_planned", "raw1_device", "raw3_device", "raw4_device_planned",
                              "raw1_host", "raw3_host_planned", "raw4_host"])
def test_mono_keyframe_pyramids_equal_reference(feed, ch, planned):
    B = len(MONO_K)
    orders = _orders(B)
    mb = dvo.MonoBatch(B, np.stack(MONO_K), 640, 480, cfg=dvo.default_config(rng_seed=3, gn_pixels_per_thread=4), per_sequence_K=True)
    init = _init_depth()
    mb.setInitialDepth(init, np.full_like(init, 0.5))
    mb.set_distortion(np.stack(MONO_D))
    checked, skipped = 0, 0
    for k in range(N_FRAMES):
        if planned:
            a = np.full(B, TRACK, np.uint8)
            if k == 3:
                a[2] = SKIP
            mb.set_actions(a)
        arr = np.stack([_mono_render()[0][o[k]] if ch == 0 else _rgb(o[k], ch) for o in orders])
        _mono_feed(mb, arr, feed, ch)
        _, _, key = mb.world_poses()
        status = mb.last_status()
        for q in range(B):
            if status[q] == SKIPPED:
                skipped += 1
                continue
            if k and not key[q]:
                continue
            exp = _ref_pyramid(orders[q][k], ch, MONO_K[q].tobytes(), MONO_D[q].tobytes())
            for lv in range(LEVELS):
                _assert_bits(mb.keyframe(q, lv)["gray"], exp[lv], "frame %d sequence %d level %d" % (k, q, lv))
            checked += k > 0
    mb.close()
    assert checked >= 2, checked            # keyframes after the first frame were checked too
    assert skipped == (1 if planned else 0), skipped


@pytest.mark.parametrize("planned", [False, True], ids=["k_pyramid_remap", "k_pyramid_remap_plan"])
def test_mono_build_reports_the_remap_kernel(planned):
    """which kernel the cases above reach: a mono handle with D reports kind REMAP, and the PLAN instance exactly when actions are set;
    the first keyframe's pyramid of every sequence is the reference's"""
    B = len(MONO_K)
    mb = dvo.MonoBatch(B, np.stack(MONO_K), 640, 480, cfg=dvo.default_config(rng_seed=3, gn_pixels_per_thread=4), per_sequence_K=True)
    init = _init_depth()
    mb.setInitialDepth(init, np.full_like(init, 0.5))
    mb.set_distortion(np.stack(MONO_D))
    if planned:
        mb.set_actions(np.full(B, TRACK, np.uint8))
    _mono_feed(mb, np.stack([_rgb(q % N_RENDER, 1) for q in range(B)]), "host", 1)
    ran = mb.last_pyramid_kernel()
    assert (ran.kind, ran.plan) == (dvo.PYRAMID_KERNEL_REMAP, 1 if planned else 0), ran.name()
    for q in range(B):
        exp = _ref_pyramid(q % N_RENDER, 1, MONO_K[q].tobytes(), MONO_D[q].tobytes())
        for lv in range(LEVELS):
            _assert_bits(mb.keyframe(q, lv)["gray"], exp[lv], "sequence %d level %d" % (q, lv))
    mb.close()


@pytest.mark.parametrize("raw", [False, True], ids=["float", "raw1"])
def test_dvo_vo_keyframe_pyramids_equal_reference(raw):
    order = _orders(1)[0]
    vo = dvo.VisualOdometry(K_LOGICOOL, 640, 480, cfg=dvo.default_config(rng_seed=3, gn_pixels_per_thread=4))
    init = _init_depth()
    vo.setInitialDepth(init, np.full_like(init, 0.5))
    vo.setDistortion(D_TUM)
    checked = 0
    for k, i in enumerate(order):
        _, key = vo.odometrizeRaw(_rgb(i, 1)) if raw else vo.odometrize(_mono_render()[0][i])
        if k and not key:
            continue
        exp = _ref_pyramid(i, 1 if raw else 0, K_LOGICOOL.tobytes(), D_TUM.tobytes())
        n = vo.keyframeCount() - 1
        for lv in range(LEVELS):
            _assert_bits(vo.keyframe(n, lv)["gray"], exp[lv], "frame %d level %d" % (k, lv))
        checked += k > 0
    vo.close()
    assert checked >= 1, checked


# ---------------------------------------------------------------- sensor depth
N_PUSH = 5
SENSOR_K = [synth.K_640, K_of(517.3, 516.5, 318.6, 255.3), K_of(535.4, 539.2, 320.1, 247.6), K_of(540.0, 530.0, 330.0, 230.0)]
SENSOR_D = [D_TUM, D_LOGICOOL, D_of(k1=-0.1, k2=0.05, p1=0.001, p2=-0.002), D_of(k1=0.05, p1=-0.004, p2=0.006, k3=-0.02)]


def _sensor_K(w, h):
    return np.stack([K * np.array([[w / 640.0], [h / 480.0], [1.0]], np.float32) for K in SENSOR_K]).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _sensor_render(w, h):
    K = _sensor_K(w, h)[0]
    g, d, s, _ = synth.sequence(4, width=w, height_px=h, K=K, seed=42, sigma_value=0.1)
    return g.numpy(), d.numpy(), s.numpy()


@functools.lru_cache(maxsize=None)
def _sensor_raw(i, ch, w, h):
    g, d, _ = _sensor_render(w, h)
    g8 = np.clip(np.rint(g[i] * 255), 0, 255).astype(np.int32)
    d16 = np.clip(np.rint(d[i] * 5000), 0, 65535).astype(np.uint16)
    d16[100 + 20 * i:150 + 20 * i, 200:280] = 0
    if ch == 1:
        rgb = g8.astype(np.uint8)
    else:
        rgb = np.stack([g8, (g8 * 7 + 31) % 256, 255 - g8] + ([(g8 * 3) % 256] if ch == 4 else []), -1).astype(np.uint8)
    return rgb, d16


def _sensor_maps(i, ch, w, h):
    """(gray, depth, sigma) the library ingests: the render's float maps or ingest_np of the raw frame"""
    if ch == 0:
        return tuple(m[i] for m in _sensor_render(w, h))
    return ingest_np(*_sensor_raw(i, ch, w, h))


def _sensor_run(levels, culls, w, h, feed, ch, frames, D, actions=None):
    import torch
    B = len(SENSOR_K)
    bt = dvo.Batch(B, SENSOR_K[0], w, h, levels, culls, cfg=dvo.default_config(gn_pixels_per_thread=4))
    bt.set_intrinsics(_sensor_K(w, h))
    if D is not None:
        bt.set_distortion(D)
    out = []
    for k in range(N_PUSH):
        maps = [np.ascontiguousarray(np.stack(m)) for m in zip(*frames(k))]
        if actions is not None and actions[k] is not None:
            bt.set_actions(np.array(actions[k], np.uint8))
        if feed == "host":
            bt.push_host(*maps)
        elif feed == "device":
            t = [torch.from_numpy(x).cuda() for x in maps]
            torch.cuda.synchronize()
            bt.push_device(*(x.data_ptr() for x in t))
        elif feed == "raw_device":
            t = [torch.from_numpy(maps[0]).cuda(), torch.from_numpy(maps[1].view(np.int16)).cuda()]
            torch.cuda.synchronize()
            bt.push_raw_device(t[0].data_ptr(), ch, t[1].data_ptr())
        else:
            assert feed == "raw_host", feed
            bt.push_raw_host(*maps)
        bt.synchronize()
        xi, T = bt.last_poses()
        logs = [bt.last_track_log(q) for q in range(B)]
        out.append((xi.copy(), T.copy(), bt.last_status().copy(),
                    [(tuple(lg["n_iter"]), tuple(np.asarray(r, np.float32).tobytes() for r in lg["residual"])) for lg in logs]))
    bt.close()
    return out


SENSOR_CASES = [(4, 1, 640, 480, "host", 0), (4, 1, 640, 480, "device", 0), (3, 2, 640, 480, "host", 0), (3, 2, 640, 480, "device", 0),
                (4, 1, 640, 480, "raw_device", 1), (4, 1, 640, 480, "raw_device", 3), (4, 1, 640, 480, "raw_host", 4),
                (3, 2, 640, 480, "raw_host", 1), (3, 2, 640, 480, "raw_device", 4),
                (4, 1, 646, 486, "device", 0), (4, 1, 646, 486, "raw_device", 1)]


@pytest.mark.parametrize("levels,culls,w,h,feed,ch", SENSOR_CASES,
                         ids=["%dx%d_L%dC%d_%s%s" % (c[2], c[3], c[0], c[1], c[4], c[5] or "") for c in SENSOR_CASES])
def test_sensor_batch_equals_plain_batch_fed_reference(levels, culls, w, h, feed, ch):
    B = len(SENSOR_K)
    Ks = _sensor_K(w, h)
    orders = [[(q + k) % 4 for k in range(N_PUSH)] for q in range(B)]

    def dist(k):
        return [_sensor_raw(orders[q][k], ch, w, h) if ch else _sensor_maps(orders[q][k], 0, w, h) for q in range(B)]

    def und(k):
        return [tuple(_undistort_np(m, Ks[q], SENSOR_D[q]) for m in _sensor_maps(orders[q][k], ch, w, h)) for q in range(B)]

    got = _sensor_run(levels, culls, w, h, feed, ch, dist, np.stack(SENSOR_D))
    ref = _sensor_run(levels, culls, w, h, "device", 0, und, None)
    for k in range(N_PUSH):
        for q in range(B):
            where = "push %d sequence %d" % (k, q)
            assert got[k][0][q].tobytes() == ref[k][0][q].tobytes(), (where, got[k][0][q], ref[k][0][q])
            assert got[k][1][q].tobytes() == ref[k][1][q].tobytes(), where
            assert got[k][2][q] == ref[k][2][q], where
            assert got[k][3][q] == ref[k][3][q], where
    # the pushes after the first tracked
    assert all((got[k][2] == dvo.SEQ_TRACKED).all() for k in range(1, N_PUSH)), [g[2] for g in got]


@pytest.mark.parametrize("feed,ch", [("device", 0), ("raw_device", 1), ("raw_host", 3)], ids=["float", "raw1", "raw3"])
def test_sensor_scalar_kernel_copies_skipped_sequences_forward(feed, ch):
    """k_pyramid_remap_depth<1, true> with SKIP in the plan.  The batch reports no kernel: the 323-pixel top level of a 646-pixel
    frame admits only the scalar kernel, and the intrinsics table makes every build a planned one.  A skipped sequence's slot holds
    garbage and its reference is copied forward, so every later twist of that sequence depends on the copy: the twists, poses,
    status and track logs equal, byte for byte, those of a plain batch with the same actions fed the numpy-undistorted maps."""
    levels, culls, w, h = 4, 1, 646, 486
    assert (w >> culls) % 4 != 0 and ((w >> culls) - 1) >> 2 >= (w >> culls) >> 2    # scalar kernel; a lower level drops a column
    B = len(SENSOR_K)
    Ks = _sensor_K(w, h)
    orders = [[(q + k) % 4 for k in range(N_PUSH)] for q in range(B)]
    S, T = SKIP, TRACK
    actions = [None, (T, S, T, T), (S, T, T, S), (T, T, S, T), (T, T, T, T)]

    def dist(k):
        fr = [_sensor_raw(orders[q][k], ch, w, h) if ch else _sensor_maps(orders[q][k], 0, w, h) for q in range(B)]
        for q in range(B):
            if actions[k] is not None and actions[k][q] == S:    # a skipped slot is never read
                fr[q] = tuple(np.full_like(m, 0xA5 if ch else 12345.0) for m in fr[q])
        return fr

    def und(k):
        return [tuple(_undistort_np(m, Ks[q], SENSOR_D[q]) for m in _sensor_maps(orders[q][k], ch, w, h)) for q in range(B)]

    got = _sensor_run(levels, culls, w, h, feed, ch, dist, np.stack(SENSOR_D), actions)
    ref = _sensor_run(levels, culls, w, h, "device", 0, und, None, actions)
    for k in range(N_PUSH):
        for q in range(B):
            where = "push %d sequence %d" % (k, q)
            assert got[k][0][q].tobytes() == ref[k][0][q].tobytes(), (where, got[k][0][q], ref[k][0][q])
            assert got[k][1][q].tobytes() == ref[k][1][q].tobytes(), where
            assert got[k][2][q] == ref[k][2][q], where
            assert got[k][3][q] == ref[k][3][q], where
        if actions[k] is not None:
            assert [int(x) for x in got[k][2]] == [SKIPPED if a == S else dvo.SEQ_TRACKED for a in actions[k]], (k, got[k][2])

