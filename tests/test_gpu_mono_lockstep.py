"""The mono pipeline against the CPU oracle in lockstep (tests/lockstep.py): the oracle follows the GPU's tracked pose at every
frame, every Gauss-Newton iteration is checked at the GPU's own input pose, and everything downstream of the pose -- keyframe
decision, propagate / Mapper::update / regularize in the pipeline's own kernels, the re-decimated pyramid -- must equal the oracle
bit for bit on every frame.  No pixel-fraction allowances: the only float tolerances are those of the per-iteration tracking check.

Frame orders follow tests/test_gpu_batch_mono_cameras.py: small steps (stereo updates), larger ones and wrap-arounds (keyframes by
translation) and static stretches (keyframes by the frame-count rule).  ring_keyframes covers every keyframe of a run: the oracle's
history is unbounded (ring overflow is pinned against dvo_vo_set_history_limit in tests/test_gpu_mono_batch.py)."""
import functools
import os
import time

import numpy as np
import pytest

import dvo_amd as dvo
import orc
from dvo_amd import synth
import lockstep
from lockstep import Replay, assert_maps_equal, batch_frames, total, vo_frame

N_RENDER = 6
N_FRAMES = 16
SEED = 3
CONTRAST = 3.0     # gray = clip(0.5 + CONTRAST (texture - 0.5), 0, 1): steep enough gradients along the epipolar lines ...
INIT_SIGMA = 0.15  # ... and a narrow enough prior that depthEstimate's sigma passes the 0.5 gate (mapper.cpp:122) on 5 mm baselines
INIT_NOISE = 0.03


def _K(fx, fy, cx, cy, skew=0.0):
    return np.array([[fx, skew, cx], [0, fy, cy], [0, 0, 1]], np.float32)


K640 = synth.K_640
K_ANISO = _K(600.0, 450.0, 320.0, 240.0)              # fx / fy = 4 / 3
K_OFFCENTRE = _K(525.0, 525.0, 250.0, 300.0)          # principal point 70 px left of and 60 px below the centre
K_SKEW = _K(560.0, 555.0, 322.0, 236.0, skew=1.5)     # tests/test_gpu_batch_mono_cameras.py: depthEstimate's full-K branch


def _scaled(K, w, h):
    K = np.array(K, np.float32).copy()
    K[0] *= w / 640.0; K[1] *= h / 480.0
    return K


@functools.lru_cache(maxsize=None)
def _render(K_bytes, w=640, h=480):
    K = np.frombuffer(K_bytes, np.float32).reshape(3, 3)
    g, d, _, _ = synth.sequence(N_RENDER, width=w, height_px=h, K=K, seed=7, sigma_value=0.5)
    return np.clip(0.5 + CONTRAST * (g.numpy() - 0.5), 0.0, 1.0).astype(np.float32), d.numpy()


def render(K, w=640, h=480):
    return _render(np.asarray(K, np.float32).tobytes(), w, h)


def init_depth(K, w=640, h=480):
    d0 = orc.cull_image(render(K, w, h)[1][0], 2)
    return (d0 + np.random.RandomState(12).normal(0, INIT_NOISE, d0.shape)).astype(np.float32)


def orders(B, n_frames=N_FRAMES):
    """per sequence the frame index at each step (tests/test_gpu_batch_mono_cameras.py::_orders, with a static stretch of seven
    frames so that the frame-count rule fires)"""
    out = []
    for b in range(B):
        step, start = 1 + b % 3, (b // 4) % N_RENDER
        seq = [(start + step * k) % N_RENDER for k in range(n_frames)]
        if b % 4 == 3:
            seq = seq[:4] + [seq[4]] * 7 + seq[11:]
        out.append(seq)
    return out


def _cfg():
    return dvo.default_config(rng_seed=SEED)


def _report(name, t0, replays):
    cov = total(replays)
    print("%s: %.1f s, coverage %s" % (name, time.perf_counter() - t0, cov))
    return cov


def _assert_coverage(cov, n_seq):
    assert cov["key_translation"] >= n_seq and cov["key_count"] >= 1, cov     # both keyframe rules
    assert cov["updates_written"] >= n_seq, cov                                 # stereo updates that really wrote depth


def _to_device(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return t


def _run_batch(Ks, w, h, frame_of, n_frames, feed="device", init=None, ring=None, seed=SEED, names=None, sigma=INIT_SIGMA):
    """A MonoBatch over len(Ks) sequences (one camera if all Ks are the same object, else a per-sequence table) in lockstep with one
    Replay per sequence.  frame_of(q, k) -> the frame sequence q sees at step k: float gray, or u8 [H, W(, C)] for feed='raw'."""
    B = len(Ks)
    shared = all(k is Ks[0] for k in Ks)
    ring = ring or n_frames
    mb = dvo.MonoBatch(B, Ks[0] if shared else np.stack(Ks), w, h, ring_keyframes=ring, cfg=dvo.default_config(rng_seed=seed),
                       per_sequence_K=not shared)
    inits = [init_depth(K, w, h) for K in Ks] if init is None else [init] * B
    sig = np.full_like(inits[0], sigma)
    if shared and init is not None:
        mb.setInitialDepth(init, sig)
    else:
        ti, ts = _to_device(np.stack(inits)), _to_device(np.stack([sig] * B))
        mb.setInitialDepthDevice(ti.data_ptr(), ts.data_ptr())
    reps = [Replay(Ks[q], w, h, seed, inits[q], sig, name=(names[q] if names else "sequence %d" % q)) for q in range(B)]
    for k in range(n_frames):
        fr = np.stack([frame_of(q, k) for q in range(B)])
        t = _to_device(fr)
        if feed == "raw":
            mb.odometrize_raw_device(t.data_ptr(), 1 if fr.ndim == 3 else fr.shape[3])
        else:
            mb.odometrize_device(t.data_ptr())
        mb.synchronize()
        for q, gf in enumerate(batch_frames(mb, k == 0)):
            reps[q].step(lockstep.raw_gray(fr[q]) if feed == "raw" else fr[q], gf)
    mb.close()
    return reps


# ---------------------------------------------------------------------------------------------------------- CPU: the helper itself
def test_replay_restates_the_oracles_visual_odometry():
    """The replay, fed the ORACLE's own per-iteration track log and poses, reproduces orc.OVO (orc_vo_odometrize) bit for bit: the
    helper restates the pipeline, so a lockstep failure on the GPU is the GPU's."""
    g, _ = render(K640)
    init = init_depth(K640)
    sig = np.full_like(init, INIT_SIGMA)
    ovo = orc.OVO(K640, 640, 480, seed=SEED)
    ovo.set_initial_depth(init, sig)
    rep = Replay(K640, 640, 480, SEED, init, sig, name="oracle")
    order = orders(4, 12)[3]           # step 1 with a static stretch: updates and keyframes by both rules
    order = order[:4] + [5, 2] + order[6:]
    for k, i in enumerate(order):
        n = ovo.keyframe_count()
        log = None
        if n:
            ref = ovo.keyframe(n - 1)
            obj = orc.OFrame(g[i], None, None, K640, 3, 2)
            _, log = orc.track(obj, ref)
            log["xi_update"] = []
            for l in range(3):
                xi, ups = np.zeros(6, np.float32), []
                if l:
                    xi = log["xi_after"][l - 1][-1]
                for it in range(log["n_iter"][l]):
                    ups.append(orc.optimize(obj.gray(l), ref.gray(l), ref.depth(l), ref.sigma(l), ref.K(l), xi, l)["xi_update"])
                    xi = log["xi_after"][l][it]
                log["xi_update"].append(np.array(ups, np.float32))
        _, key = ovo.odometrize(g[i])
        okf = ovo.keyframe(ovo.keyframe_count() - 1)
        xi_world = okf.xi if key else ovo.last_frame().xi

        def kf(level, okf=okf):
            return dict(gray=okf.gray(level), depth=okf.depth(level), sigma=okf.sigma(level), age=okf.age(), xi=okf.xi, id=okf.c.id)
        rep.step(g[i], lockstep.GpuFrame(key, xi_world, log, kf, ovo.keyframe_count(), ovo.last_valid_updates()))
    cov = rep.coverage()
    assert cov["key_translation"] >= 1 and cov["key_count"] >= 1 and cov["updates_written"] >= 2, cov


def test_replay_names_the_first_differing_pixel():
    a = np.zeros((4, 5), np.float32); b = a.copy(); b[2, 3] = 1.5; b[3, 4] = 2.0
    with pytest.raises(AssertionError, match=r"2 pixel\(s\) differ, first at \(x=3, y=2\): GPU 0.0, oracle 1.5"):
        assert_maps_equal(a, b, "x")
    n = np.full((2, 2), np.nan, np.float32)
    assert_maps_equal(n, n.copy(), "nan")


# ---------------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
def test_vo_handle_in_lockstep_with_the_oracle():
    """dvo_vo, mono, the default one-launch schedule (k_track_persist with the mono tail; the age table computed in the tail)."""
    t0 = time.perf_counter()
    g, _ = render(K640)
    init = init_depth(K640)
    sig = np.full_like(init, INIT_SIGMA)
    reps = []
    for q, order in enumerate(orders(4, 20)):
        vo = dvo.VisualOdometry(K640, 640, 480, cfg=_cfg())
        vo.setInitialDepth(init, sig)
        rep = Replay(K640, 640, 480, SEED, init, sig, name="dvo_vo order %d" % q)
        for k, i in enumerate(order):
            _, key = vo.odometrize(g[i])
            rep.step(g[i], vo_frame(vo, key, k == 0))
        vo.close()
        reps.append(rep)
    _assert_coverage(_report("dvo_vo", t0, reps), 4)


def _u8(g, channels):
    g8 = np.clip(np.rint(g * 255), 0, 255).astype(np.uint8)
    if channels == 1:
        return g8
    return np.stack([g8, np.clip(g8.astype(np.int32) * 3 // 4 + 40, 0, 255).astype(np.uint8), 255 - g8], axis=-1)


@pytest.mark.gpu
@pytest.mark.parametrize("feed", ["float", "raw1", "raw3"])
def test_mono_batch_one_camera_in_lockstep_with_the_oracle(feed):
    t0 = time.perf_counter()
    B = 10
    g, _ = render(K640)
    od = orders(B)
    if feed == "float":
        frame_of = lambda q, k: g[od[q][k]]                                   # noqa: E731
    else:
        frames8 = [_u8(x, int(feed[-1])) for x in g]
        frame_of = lambda q, k: frames8[od[q][k]]                             # noqa: E731
    reps = _run_batch([K640] * B, 640, 480, frame_of, N_FRAMES, feed="float" if feed == "float" else "raw", init=init_depth(K640))
    _assert_coverage(_report("MonoBatch %s" % feed, t0, reps), B)


@pytest.mark.gpu
def test_mono_batch_per_sequence_cameras_in_lockstep_with_the_oracle():
    """K640, a strongly anisotropic camera, a far off-centre principal point and the skew camera, each on frames rendered with it."""
    t0 = time.perf_counter()
    cams = [("K640", K640), ("anisotropic", K_ANISO), ("off-centre", K_OFFCENTRE), ("skew", K_SKEW)]
    B = 8
    cam = [q % len(cams) for q in range(B)]
    od = orders(B)
    Ks = [cams[c][1] for c in cam]
    reps = _run_batch(Ks, 640, 480, lambda q, k: render(Ks[q])[0][od[q][k]], N_FRAMES,
                      names=["sequence %d (%s)" % (q, cams[cam[q]][0]) for q in range(B)])
    _assert_coverage(_report("MonoBatch cameras", t0, reps), B)
    for c, (name, _) in enumerate(cams):
        cov = total([r for q, r in enumerate(reps) if cam[q] == c])
        assert cov["updates_written"] >= 2, (name, cov)   # every camera's depthEstimate ran against the oracle; for the skew
        #                                                   camera that is the full-K branch (k_sparse == 0)


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", [(648, 488), (320, 240)])
def test_mono_batch_frame_geometry_in_lockstep_with_the_oracle(w, h):
    """648 x 488: a 162 x 122 top map, no multiple of the workgroup.  320 x 240: an 80 x 60 top map, so the mapping window of
    mapper.cpp:90 (x in [16, 144], y in [12, 108]) is clipped by the map's own right and bottom edges."""
    t0 = time.perf_counter()
    B = 8
    K = _scaled(K640, w, h)
    g, _ = render(K, w, h)
    od = orders(B)
    reps = _run_batch([K] * B, w, h, lambda q, k: g[od[q][k]], N_FRAMES, init=init_depth(K, w, h))
    _assert_coverage(_report("MonoBatch %dx%d" % (w, h), t0, reps), B)
    if w == 320:
        upd = np.logical_or.reduce([r.updated for r in reps])
        tw, th = w >> 2, h >> 2
        assert upd[:, tw - 4:].any() and upd[th - 4:, :].any(), "no update near the clipped edges of the mapping window"


def _logicool():
    from real_data import K_LOGICOOL, frames_from_fixture
    fx = dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "logicool0_excerpt.npz")))
    return fx, frames_from_fixture(fx), K_LOGICOOL


@pytest.mark.gpu
def test_vo_handle_on_logicool0_in_lockstep_with_the_oracle():
    t0 = time.perf_counter()
    fx, frames, K = _logicool()
    seed = int(fx["seed_vo"])
    init = fx["init_depth"]
    sig = np.full_like(init, 0.5)
    vo = dvo.VisualOdometry(K, 640, 480, cfg=dvo.default_config(rng_seed=seed))
    vo.setInitialDepth(init, sig)
    rep = Replay(K, 640, 480, seed, init, sig, name="logicool0 dvo_vo")
    for k, g in enumerate(frames):
        _, key = vo.odometrize(g)
        rep.step(g, vo_frame(vo, key, k == 0))
    vo.close()
    cov = _report("logicool0 dvo_vo", t0, [rep])
    assert cov["key_translation"] + cov["key_count"] >= 5 and cov["updates_written"] >= 5, cov


@pytest.mark.gpu
def test_mono_batch_on_logicool0_in_lockstep_with_the_oracle():
    t0 = time.perf_counter()
    fx, frames, K = _logicool()
    B = 4
    od = [[(3 * b + k) % len(frames) for k in range(N_FRAMES)] for b in range(B)]
    reps = _run_batch([K] * B, 640, 480, lambda q, k: frames[od[q][k]], N_FRAMES, init=fx["init_depth"], seed=int(fx["seed_vo"]),
                      sigma=0.5)
    cov = _report("logicool0 MonoBatch", t0, reps)
    assert cov["key_translation"] + cov["key_count"] >= 2 * B and cov["updates_written"] >= 2 * B, cov
