"""Photometric calibration (inverse response + vignette) fused into the mono ingest (dvo_batch_set_photometric,
dvo_vo_set_photometric), bit for bit against the numpy replica tests/photometric_ref.py.

    gray = inv_response[c][g8] * (1.0f / vignette[c][p]),   DVO_INVALID where vignette[c][p] is not finite or <= 0

Shapes: 320x240 (top level 80x60: k_pyramid_raw4_photo with a partial last workgroup), 328x246 (top level 82x61: k_pyramid_photo;
the height is no multiple of 4, so host uploads are whole frames), 64x64 for the lifecycle, 640x480 for the dvo_vo upload paths."""
import ctypes as C
import functools

import numpy as np
import pytest

import dvo_amd as dvo
import orc
import photometric_ref as pr
from dvo_amd import synth
from real_data import undistort_index_np

pytestmark = pytest.mark.gpu

SKIP, TRACK, RESTART = dvo.SEQ_SKIP, dvo.SEQ_TRACK, dvo.SEQ_RESTART
BAD_ARGUMENT, NOT_READY = 1, 5
LEVELS = 3
N_RENDER = 6
N_FRAMES = 8
D_TUM = np.array([0.2624, -0.9531, -0.0054, 0.0026, 1.1633], np.float32)
D_MILD = np.array([-0.1, 0.05, 0.001, -0.002, 0.0], np.float32)
RAW4, SCALAR = (320, 240), (328, 246)


def _K(w, h, fx=525.0, fy=525.0, cx=319.5, cy=239.5):
    return np.array([[fx * w / 640.0, 0, cx * w / 640.0], [0, fy * h / 480.0, cy * h / 480.0], [0, 0, 1]], np.float32)


def _cfg(**kw):
    return dvo.default_config(rng_seed=3, gn_pixels_per_thread=4, **kw)


@functools.lru_cache(maxsize=None)
def _render(w, h):
    g, d, _, poses = synth.sequence(N_RENDER, w, h, _K(w, h), seed=7, sigma_value=0.5)
    return g.numpy(), d.numpy(), poses


@functools.lru_cache(maxsize=None)
def _init_depth(w, h):
    d0 = orc.cull_image(_render(w, h)[1][0], 2)
    return (d0 + np.random.RandomState(12).normal(0, 0.1, d0.shape)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _rgb(w, h, i, ch):
    """a raw frame with `ch` channels whose colour channels differ (so the fixed-point luma is exercised)"""
    g = np.clip(np.rint(_render(w, h)[0][i] * 255), 0, 255).astype(np.int32)
    if ch == 1:
        return g.astype(np.uint8)
    return np.stack([g, (g * 7 + 31) % 256, 255 - g] + ([(g * 3) % 256] if ch == 4 else []), -1).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def _cals(w, h):
    """two calibrations: (gamma 2.2, cos^4 to 0.4 in the corners) and (an S-curve, off centre with a masked bottom band)"""
    luts = np.stack([pr.gamma_response(2.2), pr.s_curve_response()]).astype(np.float32)
    Vs = np.stack([pr.cos4_vignette(w, h, 0.4), pr.masked_vignette(w, h)]).astype(np.float32)
    return luts, Vs


SEQ_CAL = np.array([0, 1, 1, 0], np.int32)


def _undistort_np(img, K, D):
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


def _new_batch(B, w, h, K=None, per_camera=False, cfg=None):
    mb = dvo.MonoBatch(B, _K(w, h) if K is None else K, w, h, cfg=cfg if cfg is not None else _cfg(), per_sequence_K=per_camera)
    init = _init_depth(w, h)
    mb.setInitialDepth(init, np.full_like(init, 0.5))
    return mb


def _feed(mb, arr, feed="device"):
    import torch
    arr = np.ascontiguousarray(arr)
    if feed == "host":
        mb.odometrize_host(arr)
        return
    t = torch.from_numpy(arr).cuda()
    torch.cuda.synchronize()
    if arr.dtype == np.uint8:
        mb.odometrize_raw_device(t.data_ptr(), 1 if arr.ndim == 3 else arr.shape[3])
    else:
        mb.odometrize_device(t.data_ptr())
    mb.synchronize()


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


def _orders(B):
    return [[((b // 3) + (1 + b % 3) * k) % N_RENDER for k in range(N_FRAMES)] for b in range(B)]


# ---------------------------------------------------------------- 1. the gain table
def _special_vignette(w, h):
    """a vignette holding 0, a negative, NaN, +inf and a denormal at kept pixels.  The first four mask the pixel (gain -1, gray
    INVALID); the denormal is positive and finite, so its gain is 1 / V = +inf and the product is IEEE's (inf, or NaN for a zero
    response, which the pyramid's pass_valid turns into INVALID as it does for a float frame)."""
    V = pr.cos4_vignette(w, h, 0.4).copy()
    V[0, 0] = 0.0; V[4, 8] = -0.5; V[8, 4] = np.nan; V[12, 12] = np.inf; V[16, 20] = np.float32(1e-40); V[20, 16] = np.float32(1e-40)
    return V


def test_gain_table_without_lens_and_special_values():
    w, h = RAW4
    V = _special_vignette(w, h)
    lut = pr.gamma_response(2.2).astype(np.float32)
    mb = _new_batch(2, w, h)
    mb.set_photometric(lut, V)
    exp = pr.gain_table_np(V, w, h)
    assert exp[0, 0] == -1 and exp[1, 2] == -1 and exp[2, 1] == -1 and exp[3, 3] == -1 and np.isposinf(exp[4, 5]) and np.isposinf(exp[5, 4])
    for q in range(2):
        _assert_bits(mb.photometric_gain(q), exp, "gain of sequence %d" % q)
    # ... and the product: a frame whose byte at one denormal pixel is 0 (0 * inf = NaN -> INVALID) and 200 at the other (inf)
    f = _rgb(w, h, 0, 1).copy()
    f[16, 20] = 0; f[20, 16] = 200
    _feed(mb, np.stack([f, f]))
    fr = orc.OFrame(pr.correct_np(f, lut, V), None, None, _K(w, h), LEVELS, 2)
    top = fr.gray(2)
    assert top[0, 0] == -2 and top[1, 2] == -2 and top[2, 1] == -2 and top[3, 3] == -2 and top[4, 5] == -2 and np.isposinf(top[5, 4])
    for lv in range(LEVELS):
        _assert_bits(mb.keyframe(1, lv)["gray"], fr.gray(lv), "level %d" % lv)
    mb.close()


@pytest.mark.parametrize("lens_first", [False, True], ids=["calibration_then_D", "D_then_calibration"])
def test_gain_table_with_two_lenses_and_two_calibrations(lens_first):
    w, h = RAW4
    Ks = np.stack([_K(w, h), _K(w, h, 517.3, 516.5, 318.6, 255.3)])
    cam = [0, 1, 0, 1]
    cal = np.array([0, 0, 1, 1], np.int32)
    D = np.stack([D_TUM, D_MILD])
    luts, Vs = _cals(w, h)
    Vs = Vs.copy(); Vs[0] = _special_vignette(w, h)
    mb = _new_batch(4, w, h, K=np.stack([Ks[c] for c in cam]), per_camera=True)
    if lens_first:
        mb.set_distortion(np.stack([D[c] for c in cam]))
    mb.set_photometric(luts, Vs, cal)
    if not lens_first:
        mb.set_distortion(np.stack([D[c] for c in cam]))
    n, sc = mb.get_photometric()
    assert n == 2 and (sc == cal).all()
    masked = 0
    for q in range(4):
        exp = pr.gain_table_np(Vs[cal[q]], w, h, Ks[cam[q]], D[cam[q]])
        masked += int((exp < 0).sum())
        _assert_bits(mb.photometric_gain(q), exp, "gain of sequence %d" % q)
    assert masked > 0   # the remap's border and the masked band really occur
    mb.close()


# ---------------------------------------------------------------- 2. pyramids
@functools.lru_cache(maxsize=None)
def _ref_pyramid(w, h, i, ch, c, with_D):
    luts, Vs = _cals(w, h)
    img = pr.correct_np(_rgb(w, h, i, ch), luts[c], Vs[c])
    if with_D:
        img = _undistort_np(img, _K(w, h), D_TUM)
    fr = orc.OFrame(img, None, None, _K(w, h), LEVELS, 2)
    return tuple(fr.gray(l) for l in range(LEVELS))


PYRAMID_CASES = [
    # shape, channels, feed, planned, with D, the kernel kind that must have run
    (RAW4, 1, "device", False, False, dvo.PYRAMID_KERNEL_PHOTO_RAW4),
    (RAW4, 1, "host", True, False, dvo.PYRAMID_KERNEL_PHOTO_RAW4),
    (RAW4, 3, "device", True, False, dvo.PYRAMID_KERNEL_PHOTO_SCALAR),
    (RAW4, 4, "host", False, False, dvo.PYRAMID_KERNEL_PHOTO_SCALAR),
    (SCALAR, 1, "device", False, False, dvo.PYRAMID_KERNEL_PHOTO_SCALAR),
    (SCALAR, 1, "host", True, False, dvo.PYRAMID_KERNEL_PHOTO_SCALAR),
    (SCALAR, 3, "host", False, False, dvo.PYRAMID_KERNEL_PHOTO_SCALAR),
    (SCALAR, 4, "device", True, False, dvo.PYRAMID_KERNEL_PHOTO_SCALAR),
    (RAW4, 1, "device", False, True, dvo.PYRAMID_KERNEL_PHOTO_REMAP),
    (RAW4, 3, "host", True, True, dvo.PYRAMID_KERNEL_PHOTO_REMAP),
    (SCALAR, 4, "device", True, True, dvo.PYRAMID_KERNEL_PHOTO_REMAP),
    (SCALAR, 1, "host", False, True, dvo.PYRAMID_KERNEL_PHOTO_REMAP),
]


@pytest.mark.parametrize("shape,ch,feed,planned,with_D,kind", PYRAMID_CASES,
                         ids=["%dx%d_raw%d_%s%s%s" % (c[0][0], c[0][1], c[1], c[2], "_planned" if c[3] else "", "_D" if c[4] else "")
                              for c in PYRAMID_CASES])
def test_keyframe_pyramids_equal_replica(shape, ch, feed, planned, with_D, kind):
    w, h = shape
    B = 4
    luts, Vs = _cals(w, h)
    orders = _orders(B)
    mb = _new_batch(B, w, h)
    mb.set_photometric(luts, Vs, SEQ_CAL)
    if with_D:
        mb.set_distortion(D_TUM)
    checked, skipped = 0, 0
    for k in range(N_FRAMES):
        if planned:
            a = np.full(B, TRACK, np.uint8)
            if k == 3:
                a[2] = SKIP
            mb.set_actions(a)
        _feed(mb, np.stack([_rgb(w, h, o[k], ch) for o in orders]), feed)
        ran = mb.last_pyramid_kernel()
        assert (ran.kind, ran.plan) == (kind, 1 if planned else 0), (k, ran.name())
        assert ran.culls == (2 if kind == dvo.PYRAMID_KERNEL_PHOTO_RAW4 else 0)
        _, _, key = mb.world_poses()
        status = mb.last_status()
        for q in range(B):
            if status[q] == dvo.SEQ_SKIPPED:
                skipped += 1
                continue
            if k and not key[q]:
                continue
            exp = _ref_pyramid(w, h, orders[q][k], ch, int(SEQ_CAL[q]), with_D)
            for lv in range(LEVELS):
                _assert_bits(mb.keyframe(q, lv)["gray"], exp[lv], "frame %d sequence %d level %d" % (k, q, lv))
            checked += k > 0
    mb.close()
    assert checked >= 1, checked            # a keyframe after the first frame was checked too
    assert skipped == (1 if planned else 0), skipped


@pytest.mark.parametrize("planned", [False, True], ids=["plain", "planned"])
def test_keyframe_pyramids_with_the_response_read_by_plain_loads(planned, monkeypatch):
    """k_pyramid_raw4_photo<2, planned, false>: DVO_PHOTO_RESPONSE=global (read at every launch) takes the instance without the LDS
    stage, held to the same replica by the same case; the reported kind does not tell the two instances apart, the variable does"""
    monkeypatch.setenv("DVO_PHOTO_RESPONSE", "global")
    test_keyframe_pyramids_equal_replica(RAW4, 1, "device", planned, False, dvo.PYRAMID_KERNEL_PHOTO_RAW4)


# ---------------------------------------------------------------- 3. equal to two passes
def _run(mb, B, frames_of, feed="device"):
    out = []
    for k in range(N_FRAMES):
        _feed(mb, frames_of(k), feed)
        out.append(_state(mb, B))
    mb.close()
    return out


@pytest.mark.parametrize("ch,with_D", [(1, False), (3, False), (1, True)], ids=["raw1", "raw3", "raw1_D"])
def test_calibrated_batch_equals_plain_batch_fed_corrected_frames(ch, with_D):
    w, h = RAW4
    B = 4
    luts, Vs = _cals(w, h)
    orders = _orders(B)
    a = _new_batch(B, w, h)
    a.set_photometric(luts, Vs, SEQ_CAL)
    if with_D:
        a.set_distortion(D_TUM)
    got = _run(a, B, lambda k: np.stack([_rgb(w, h, o[k], ch) for o in orders]))

    def corrected(k):
        fr = [pr.correct_np(_rgb(w, h, orders[q][k], ch), luts[SEQ_CAL[q]], Vs[SEQ_CAL[q]]) for q in range(B)]
        if with_D:
            fr = [dvo.undistort(f, _K(w, h), D_TUM) for f in fr]
        return np.stack(fr)

    ref = _run(_new_batch(B, w, h), B, corrected)
    keys = 0
    for k in range(N_FRAMES):
        for q in range(B):
            assert got[k][q] == ref[k][q], ("frame", k, "sequence", q)
            keys += k > 0 and got[k][q][1]
    assert keys > 0, "no keyframe after the first frame: the mapping branch was not compared"


# ---------------------------------------------------------------- 4. identity
def test_identity_calibration_is_the_plain_handle():
    w, h = RAW4
    B = 2
    ones = np.ones((h, w), np.float32)
    ident = pr.identity_response()
    assert ident.tobytes() == (np.arange(256, dtype=np.float32) * np.float32(1.0 / 255.0)).tobytes()
    runs = {}
    for name, (lut, V) in {"both": (ident, ones), "response_null": (None, ones), "vignette_null": (ident, None), "never": (None, None)}.items():
        mb = _new_batch(B, w, h)
        if name != "never":
            mb.set_photometric(lut, V)
        kinds = []
        out = []
        for k in range(5):
            _feed(mb, np.stack([_rgb(w, h, (k + q) % N_RENDER, 1) for q in range(B)]))
            kinds.append(mb.last_pyramid_kernel().kind)
            out.append(_state(mb, B))
        mb.close()
        runs[name] = out
        assert set(kinds) == {dvo.PYRAMID_KERNEL_RAW4 if name == "never" else dvo.PYRAMID_KERNEL_PHOTO_RAW4}, (name, kinds)
    for name in ("both", "response_null", "vignette_null"):
        assert runs[name] == runs["never"], name
    # ... and the never-set handle on the other shape runs the plain scalar kernel
    w, h = SCALAR
    mb = _new_batch(1, w, h)
    _feed(mb, _rgb(w, h, 0, 1)[None])
    assert mb.last_pyramid_kernel().kind == dvo.PYRAMID_KERNEL_SCALAR
    mb.close()


# ---------------------------------------------------------------- 5. dvo_vo
@pytest.mark.parametrize("stage", ["1", "0"], ids=["staged", "dma"])
def test_dvo_vo_equals_one_sequence_batch(stage, monkeypatch):
    monkeypatch.setenv("DVO_MONO_STAGE", stage)   # (read per handle)
    w, h = 640, 480
    luts, Vs = _cals(w, h)
    lut, V = luts[1], Vs[1]
    order = _orders(1)[0]
    vo = dvo.VisualOdometry(_K(w, h), w, h, cfg=_cfg())
    init = _init_depth(w, h)
    vo.setInitialDepth(init, np.full_like(init, 0.5))
    vo.set_photometric(lut, V)
    mb = _new_batch(1, w, h)
    mb.set_photometric(lut, V)
    for k, i in enumerate(order):
        f = _rgb(w, h, i, 1)
        T, key = vo.odometrizeRaw(f)
        kf = vo.keyframe(vo.keyframeCount() - 1)
        _feed(mb, f[None])
        _, Tb, keyb = mb.world_poses()
        kb = mb.keyframe(0, 2)
        assert np.asarray(T, np.float32).tobytes() == Tb[0].tobytes() and bool(key) == bool(keyb[0]), k
        for n in ("gray", "depth", "sigma", "age", "xi"):
            assert np.asarray(kf[n], np.float32).tobytes() == np.asarray(kb[n], np.float32).tobytes(), (k, n)
        if k == 0:
            _assert_bits(kf["gray"], orc.OFrame(pr.correct_np(f, lut, V), None, None, _K(w, h), LEVELS, 2).gray(2), "dvo_vo first keyframe")
    # the float and sensor-depth entry points are refused on a calibrated handle
    L = dvo.lib()
    g = _render(w, h)[0][0]
    T = np.zeros(16, np.float32); kk = C.c_int(0)
    assert L.dvo_vo_odometrize(vo._p, dvo.fp(g), dvo.fp(T), C.byref(kk)) == BAD_ARGUMENT
    assert b"dvo_vo_set_photometric" in L.dvo_last_error()
    assert L.dvo_vo_odometrize_depth(vo._p, dvo.fp(g), dvo.fp(g), dvo.fp(g), dvo.fp(T)) == BAD_ARGUMENT
    assert L.dvo_vo_set_photometric(vo._p, None, None) == NOT_READY
    monkeypatch.delenv("DVO_MONO_STAGE", raising=False)
    vo.close(); mb.close()


# ---------------------------------------------------------------- 6. lifecycle and errors
def test_lifecycle_and_errors():
    L = dvo.lib()
    w = h = 64
    B = 3
    luts, Vs = _cals(w, h)
    cal = np.array([0, 1, 0], np.int32)
    frames = [np.stack([_rgb(w, h, (i + q) % N_RENDER, 1) for q in range(B)]) for i in range(5)]
    ip = lambda a: a.ctypes.data_as(C.c_void_p)

    # every error of the contract, before anything changes
    a = _new_batch(B, w, h)
    assert L.dvo_batch_set_photometric(None, 1, dvo.fp(luts), None, None) == BAD_ARGUMENT
    assert L.dvo_batch_set_photometric(a._p, -1, dvo.fp(luts), None, None) == BAD_ARGUMENT and b"n_cal" in L.dvo_last_error()
    assert L.dvo_batch_set_photometric(a._p, 2, None, None, None) == BAD_ARGUMENT and b"n_cal > 0" in L.dvo_last_error()
    bad_cal = np.array([0, 2, 0], np.int32)
    assert L.dvo_batch_set_photometric(a._p, 2, dvo.fp(luts), dvo.fp(Vs), ip(bad_cal)) == BAD_ARGUMENT
    assert b"sequence 1" in L.dvo_last_error()
    bad_cal[1] = -1
    assert L.dvo_batch_set_photometric(a._p, 2, dvo.fp(luts), dvo.fp(Vs), ip(bad_cal)) == BAD_ARGUMENT and b"sequence 1" in L.dvo_last_error()
    for bad in (np.nan, np.inf, -0.25):
        bl = luts.copy(); bl[1, 17] = bad
        assert L.dvo_batch_set_photometric(a._p, 2, dvo.fp(bl), dvo.fp(Vs), ip(cal)) == BAD_ARGUMENT
        assert b"calibration 1" in L.dvo_last_error() and b"entry 17" in L.dvo_last_error()
    sensor = dvo.Batch(2, _K(w, h), w, h, 3, 2, cfg=_cfg())
    assert L.dvo_batch_set_photometric(sensor._p, 2, dvo.fp(luts), dvo.fp(Vs), None) == BAD_ARGUMENT and b"mono batch" in L.dvo_last_error()
    sensor.close()
    n, sc = a.get_photometric()
    assert n == 0 and not sc.any()                       # nothing was set by any of them
    gain = np.zeros((h // 4, w // 4), np.float32)
    assert L.dvo_debug_batch_photometric_gain(a._p, 0, dvo.fp(gain)) == NOT_READY
    # set, then cleared: the never-set handle, and get round-trips
    a.set_photometric(luts, Vs, cal)
    n, sc = a.get_photometric()
    assert n == 2 and (sc == cal).all()
    a.set_photometric(None, None)
    assert a.get_photometric()[0] == 0
    b = _new_batch(B, w, h)
    for f in frames:
        _feed(a, f); _feed(b, f)
        assert a.last_pyramid_kernel().kind == dvo.PYRAMID_KERNEL_RAW4
        assert _state(a, B) == _state(b, B)
    a.close(); b.close()

    # set after a frame: NOT_READY, and the run continues unchanged; float feeds are refused; RESTART keeps the calibration
    a = _new_batch(B, w, h); a.set_photometric(luts, Vs, cal)
    c = _new_batch(B, w, h); c.set_photometric(luts, Vs, cal)
    _feed(a, frames[0]); _feed(c, frames[0])
    assert L.dvo_batch_set_photometric(a._p, 0, None, None, None) == NOT_READY
    assert L.dvo_batch_set_photometric(a._p, 1, dvo.fp(luts), None, None) == NOT_READY
    assert a.get_photometric()[0] == 2
    import torch
    fl = torch.zeros((B, h, w), dtype=torch.float32, device="cuda")
    assert L.dvo_batch_odometrize_device(a._p, C.c_void_p(fl.data_ptr())) == BAD_ARGUMENT and b"dvo_batch_set_photometric" in L.dvo_last_error()
    host_fl = np.zeros((B, h, w), np.float32)
    assert L.dvo_batch_odometrize_host(a._p, dvo.fp(host_fl)) == BAD_ARGUMENT
    for f in frames[1:3]:
        _feed(a, f); _feed(c, f)
        assert _state(a, B) == _state(c, B)
    a.close(); c.close()
    a = _new_batch(B, w, h); a.set_photometric(luts, Vs, cal)
    for k, f in enumerate(frames):
        act = np.full(B, TRACK, np.uint8)
        if k == 2:
            act[1] = RESTART
        a.set_actions(act)
        _feed(a, f)
        if k == 2:
            assert a.last_status()[1] == dvo.SEQ_STARTED
            exp = orc.OFrame(pr.correct_np(f[1], luts[1], Vs[1]), None, None, _K(w, h), LEVELS, 2)
            for lv in range(LEVELS):
                _assert_bits(a.keyframe(1, lv)["gray"], exp.gray(lv), "restarted keyframe level %d" % lv)
    assert a.get_photometric()[0] == 2
    a.close()


# ---------------------------------------------------------------- 7. composition
@pytest.mark.parametrize("terms", ["huber_median", "huber_affine_estimate"])
def test_composition_with_opt_in_terms_equals_plain_batch(terms):
    """Huber weights with the median scale, or Huber weights with affine ESTIMATE (the library refuses the median scale together with
    affine brightness: two runs cover both), each with track quality and a constant-velocity pose guess, on five sequences with
    per-sequence cameras, one SKIP and one RESTART on the way: none of them knows about the calibration."""
    w, h = RAW4
    B = 5
    luts, Vs = _cals(w, h)
    cal = np.array([0, 1, 1, 0, 1], np.int32)
    Ks = np.stack([_K(w, h, 525.0 + 4 * q, 525.0 - 3 * q, 319.5 + q, 239.5 - q) for q in range(B)])
    orders = _orders(B)

    def run(calibrated):
        mb = _new_batch(B, w, h, K=Ks, per_camera=True)
        if calibrated:
            mb.set_photometric(luts, Vs, cal)
        if terms == "huber_median":
            mb.set_robust_median(dvo.ROBUST_HUBER, 1.345)
        else:
            mb.set_robust_weights(dvo.ROBUST_HUBER, 1.345)
            mb.set_affine_brightness(dvo.AFFINE_ESTIMATE)
        mb.set_track_quality(True)
        mb.set_pose_guess_mode(dvo.GUESS_CONSTANT_VELOCITY)
        out = []
        for k in range(N_FRAMES):
            act = np.full(B, TRACK, np.uint8)
            if k == 3:
                act[1] = SKIP
            if k == 4:
                act[3] = RESTART
            mb.set_actions(act)
            raw = [_rgb(w, h, o[k], 1) for o in orders]
            if calibrated:
                _feed(mb, np.stack(raw))
            else:
                _feed(mb, np.stack([pr.correct_np(raw[q], luts[cal[q]], Vs[cal[q]]) for q in range(B)]))
            st = mb.last_status()
            live = [q for q in range(B) if st[q] != dvo.SEQ_SKIPPED]
            _, T, key = mb.world_poses()
            rec = ()
            if k:
                rec = (mb.last_robust_scales().tobytes(), mb.last_track_quality().tobytes())
                rec += (mb.last_affine().tobytes(),) if terms == "huber_affine_estimate" else ()
            out.append((st.tobytes(), T.tobytes(), key.tobytes(), rec,
                        [tuple(mb.keyframe(q, lv)["gray"].tobytes() for lv in range(LEVELS)) + (tuple(sorted(mb.stats(q).items())),) for q in live]))
        mb.close()
        return out

    got, ref = run(True), run(False)
    for k in range(N_FRAMES):
        assert got[k] == ref[k], ("frame", k)
