"""Per-sequence camera intrinsics of a sensor-depth batch (dvo_batch_set_intrinsics, include/dvo.h) on the GPU.

Every sequence of a mixed-camera batch must give the bits of a one-sequence batch created with that sequence's K on the same
frames; a sequence whose intrinsics change loses its reference at that push.  One tile size throughout (gn_pixels_per_thread = 4):
at one tile size every schedule gives the same bits (test_gpu_parity.py::test_batch_many_iterations_every_sequence_matches_single)."""
import ctypes as C
import functools

import numpy as np
import pytest

import dvo_amd as dvo
import orc
from dvo_amd import synth

pytestmark = pytest.mark.gpu

SKIP, TRACK, RESTART = dvo.SEQ_SKIP, dvo.SEQ_TRACK, dvo.SEQ_RESTART
TRACKED, SKIPPED, STARTED = dvo.SEQ_TRACKED, dvo.SEQ_SKIPPED, dvo.SEQ_STARTED
EYE = np.eye(4, dtype=np.float32)


def _K(fx, fy, cx, cy):
    return np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], np.float32)


# synth.K_640, the TUM fr1 and fr3 RGB cameras, and one far from the others
CAMS = [synth.K_640, _K(517.3, 516.5, 318.6, 255.3), _K(535.4, 539.2, 320.1, 247.6), _K(400.0, 400.0, 300.0, 260.0)]
FAR = 3
N_FRAMES = 4


def _cfg(**kw):
    return dvo.default_config(gn_pixels_per_thread=4, **kw)


def _logbits(lg):
    """(iterations per level, residual bits per level) of a track log: what must agree bit for bit"""
    return tuple(lg["n_iter"][:4]), tuple(np.asarray(r, np.float32).tobytes() for r in lg["residual"][:4])


@functools.lru_cache(maxsize=None)
def _render(cam, sigma=0.1):
    """N_FRAMES frames of a trajectory rendered with camera `cam` (numpy gray, depth, sigma, GT poses)"""
    g, d, s, poses = synth.sequence(N_FRAMES, K=CAMS[cam], seed=42 + cam, sigma_value=sigma)
    return g.numpy(), d.numpy(), s.numpy(), poses


def _feed(bt, feed, g, d, s):
    """one push of float maps (host / device) or of raw u8 + u16 frames (host / device) derived from them"""
    import torch
    if feed.startswith("raw"):
        g8 = np.clip(np.rint(g * 255), 0, 255).astype(np.uint8)
        d16 = np.clip(np.rint(d * 5000), 0, 65535).astype(np.uint16)
        if feed == "raw_host":
            bt.push_raw_host(g8, d16)
        else:
            tg = torch.from_numpy(g8).cuda(); td = torch.from_numpy(d16.view(np.int16)).cuda(); torch.cuda.synchronize()
            bt.push_raw_device(tg.data_ptr(), 1, td.data_ptr())
            bt.synchronize()
    elif feed == "host":
        bt.push_host(np.ascontiguousarray(g), np.ascontiguousarray(d), np.ascontiguousarray(s))
    else:
        t = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (g, d, s)]
        torch.cuda.synchronize()
        bt.push_device(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr())
        bt.synchronize()


def _plan(B, seed, cams=None):
    rng = np.random.RandomState(seed)
    cam = np.array(cams if cams is not None else [q % len(CAMS) for q in range(B)])
    order = np.stack([rng.permutation(N_FRAMES) for _ in range(B)])
    return cam, order


def _frames_of(cam, order, k, sigma=0.1):
    rs = [_render(int(c), sigma) for c in cam]
    idx = [int(order[q][k]) for q in range(len(cam))]
    return (np.stack([r[0][i] for r, i in zip(rs, idx)]), np.stack([r[1][i] for r, i in zip(rs, idx)]),
            np.stack([r[2][i] for r, i in zip(rs, idx)]))


def _run(cfg, cam, order, n_push, feed="device", table=True, seqs=None):
    """A batch over the sequences' cameras (table=False: every sequence on the creation K_640); per push k >= 1 (xi, T, logbits)."""
    B = len(cam)
    bt = dvo.Batch(B, CAMS[0], 640, 480, 4, 1, cfg=cfg)
    if table:
        bt.set_intrinsics(np.stack([CAMS[int(c)] for c in cam]))
    out = []
    for k in range(n_push):
        _feed(bt, feed, *_frames_of(cam, order, k))
        if k:
            xi, T = bt.last_poses()
            assert (bt.last_status() == TRACKED).all(), k
            out.append((xi.copy(), T.copy(), [_logbits(bt.last_track_log(int(q))) for q in (seqs if seqs is not None else range(B))]))
    bt.close()
    return out


_one_cache = {}


def _one(cfg_key, cfg, c, frames_seq, feed="host", src=None):
    """A one-sequence batch created with camera c, fed frames_seq (list of (frame index, (g, d, s))) rendered with camera src
    (default c); per push k >= 1 (xi, T, logbits)."""
    key = (cfg_key, c, c if src is None else src, tuple(i for i, _ in frames_seq), feed)
    if key not in _one_cache:
        bt = dvo.Batch(1, CAMS[c], 640, 480, 4, 1, cfg=cfg)
        out = []
        for k, (_, (g, d, s)) in enumerate(frames_seq):
            _feed(bt, "raw_host" if feed.startswith("raw") else "host", g[None], d[None], s[None])
            if k:
                xi, T = bt.last_poses()
                out.append((xi[0].copy(), T[0].copy(), _logbits(bt.last_track_log(0))))
        bt.close()
        _one_cache[key] = out
    return _one_cache[key]


def _check_against_one(out, cfg_key, cfg, cam, order, n_push, feed="host", seqs=None):
    seqs = list(seqs if seqs is not None else range(len(cam)))
    for j, q in enumerate(seqs):
        r = _render(int(cam[q]))
        fr = [(int(order[q][k]), (r[0][order[q][k]], r[1][order[q][k]], r[2][order[q][k]])) for k in range(n_push)]
        ref = _one(cfg_key, cfg, int(cam[q]), fr, feed)
        for k in range(n_push - 1):
            xi, T, lb = out[k]
            np.testing.assert_array_equal(xi[q], ref[k][0], err_msg="push %d seq %d" % (k + 1, q))
            np.testing.assert_array_equal(T[q], ref[k][1], err_msg="push %d seq %d" % (k + 1, q))
            assert lb[j] == ref[k][2], (k + 1, q)


@pytest.mark.parametrize("variant", ["default", "track_adaptive=-1", "B=6", "track_fused_tiles=8", "gn_use_lds_patch=1", "track_streams=2"])
def test_mixed_cameras_equal_one_camera_batches(variant):
    B = 6 if variant == "B=6" else 12   # B=6: one launch per iteration (k_track_gn_fused) on the levels that fit it
    cfg = _cfg() if "=" not in variant or variant == "B=6" else _cfg(**{variant.split("=")[0]: int(variant.split("=")[1])})
    cam, order = _plan(B, seed=11)
    out = _run(cfg, cam, order, 3)
    # (gn_use_lds_patch: another tile shape, so the one-sequence batches run the same kernel, k_track_gn_tile)
    _check_against_one(out, variant if variant == "gn_use_lds_patch=1" else "pinned", cfg, cam, order, 3)


def test_uniform_table_is_the_plain_path():
    cam, order = _plan(12, seed=12, cams=[0] * 12)
    plain = _run(_cfg(), cam, order, 3, table=False)
    table = _run(_cfg(), cam, order, 3, table=True)
    for (x0, T0, r0), (x1, T1, r1) in zip(plain, table):
        np.testing.assert_array_equal(x0, x1); np.testing.assert_array_equal(T0, T1)
        assert r0 == r1


# The bench's converging constants (bench.py's converging side leg: reference steps x 0.5, sigma 0.5): the update is the Gauss-Newton
# step, so the pose error measures the model -- here the intrinsics -- not the over-relaxed iteration.
# Bound on the far camera's consecutive-frame translation error (m).  Measured on an MI355X: 4.5e-4 m with the per-sequence K,
# 4.1e-3 m with the shared K_640 on the same frames; the test asks for < FAR_BOUND and > 3 x FAR_BOUND respectively.
FAR_BOUND = 1.0e-3


def test_the_right_K_matters():
    cfg = _cfg(step_default=1.0, step_level1=0.75, step_level2=0.5, min_residual=0.0)
    B = 8
    cam = np.array([0, FAR] * (B // 2))
    g, d, s, poses = _render(FAR, 0.5)
    errs = {}
    for table in (True, False):
        bt = dvo.Batch(B, CAMS[0], 640, 480, 4, 1, cfg=cfg)
        if table:
            bt.set_intrinsics(np.stack([CAMS[int(c)] for c in cam]))
        e = []
        for k in range(N_FRAMES):
            gs = np.stack([_render(int(c), 0.5)[0][k] for c in cam])
            ds = np.stack([_render(int(c), 0.5)[1][k] for c in cam])
            ss = np.stack([_render(int(c), 0.5)[2][k] for c in cam])
            bt.push_host(gs, ds, ss)
            if k:
                xi = bt.last_poses()[0]
                for q in np.flatnonzero(cam == FAR):
                    E = synth.se3_exp_np(np.asarray(xi[q], np.float64)) @ np.linalg.inv(np.linalg.inv(poses[k]) @ poses[k - 1])
                    e.append(float(np.linalg.norm(E[:3, 3])))
        bt.close()
        errs[table] = max(x if np.isfinite(x) else np.inf for x in e)
    print("far camera: max translation error per-camera %.3g m, shared K %.3g m" % (errs[True], errs[False]))
    assert errs[True] < FAR_BOUND, errs
    assert errs[False] > 3 * FAR_BOUND, errs


def _change_run(mode):
    """6 sequences on K_640; before push 2 sequences 0, 1, 2 move to the fr1 camera (2 with a SKIP under actions); 4 pushes."""
    import torch
    B = 6
    cam, order = _plan(B, seed=13, cams=[0] * B)
    bt = dvo.Batch(B, CAMS[0], 640, 480, 4, 1, cfg=_cfg())
    Ks = np.stack([CAMS[0]] * B)
    got = []
    for k in range(4):
        if k == 2:
            Ks[:3] = CAMS[1]
            bt.set_intrinsics(Ks)
        acts = np.full(B, TRACK, np.uint8)
        if k == 2 and mode != "none":
            acts[2] = SKIP
        if mode == "host":
            bt.set_actions(acts)
        elif mode == "device":
            ta = torch.from_numpy(acts).cuda(); torch.cuda.synchronize()
            bt.set_actions(ta.data_ptr(), on_device=True)
        g, d, s = _frames_of(cam, order, k)
        if k == 2 and mode != "none":
            g[2] = np.nan; d[2] = np.nan; s[2] = np.nan   # a skipped slot is never read
        _feed(bt, "host", g, d, s)
        if k == 0 and mode == "none":   # (a plain first push tracks nothing and has no poses)
            got.append(None)
            continue
        xi, T = bt.last_poses()
        got.append((xi.copy(), T.copy(), bt.last_status(), [_logbits(bt.last_track_log(q)) for q in range(B)]))
        if mode == "device":
            del ta
    bt.close()
    return cam, order, got


@pytest.mark.parametrize("mode", ["none", "host", "device"])
def test_camera_change_mid_stream(mode):
    cam, order, got = _change_run(mode)
    skip2 = mode != "none"
    st2, st3 = got[2][2], got[3][2]
    assert list(st2[:2]) == [STARTED, STARTED]
    assert st2[2] == (SKIPPED if skip2 else STARTED)
    assert (st2[3:] == TRACKED).all()
    assert st3[2] == (STARTED if skip2 else TRACKED)      # the SKIP left it without a reference
    assert (np.delete(st3, 2) == TRACKED).all()
    for q in (0, 1, 2):
        assert not np.any(got[2][0][q]); np.testing.assert_array_equal(got[2][1][q], EYE)
    r0 = _render(0)
    for q in range(6):
        f = [int(order[q][k]) for k in range(4)]
        if q < 2 or (q == 2 and not skip2):   # a fresh one-sequence batch with the new K from push 2 on
            ref = _one("pinned", _cfg(), 1, [(i, (r0[0][i], r0[1][i], r0[2][i])) for i in f[2:]], src=0)
            xi, T, _, lb = got[3]
            np.testing.assert_array_equal(xi[q], ref[0][0]); np.testing.assert_array_equal(T[q], ref[0][1])
            assert lb[q] == ref[0][2], q
        elif q == 2:
            assert not np.any(got[3][0][q])
        else:                                 # unchanged sequences keep tracking on K_640
            ref = _one("pinned", _cfg(), 0, [(i, (r0[0][i], r0[1][i], r0[2][i])) for i in f])
            for k in (1, 2, 3):
                xi, T, _, lb = got[k]
                np.testing.assert_array_equal(xi[q], ref[k - 1][0], err_msg="push %d seq %d" % (k, q))
                assert lb[q] == ref[k - 1][2], (k, q)


@pytest.mark.parametrize("feed", ["raw_device", "raw_host", "host"])
def test_feeds_match_one_camera_batches(feed):
    cam, order = _plan(8, seed=14)
    out = _run(_cfg(), cam, order, 3, feed=feed)
    _check_against_one(out, "pinned", _cfg(), cam, order, 3, feed=feed)


def test_scale_1024_sequences():
    B = 1024
    cam, order = _plan(B, seed=15)
    sample = np.random.RandomState(16).choice(B, 16, replace=False)
    out = _run(_cfg(), cam, order, 3, seqs=sample)
    _check_against_one(out, "pinned", _cfg(), cam, order, 3, seqs=sample)


def test_contributing_pixels_match_the_oracle():
    """Per Gauss-Newton iteration, the contributing-pixel count equals orc.optimize with the sequence's K at the GPU's input pose."""
    cam, order = _plan(4, seed=17, cams=[1, 0, FAR, 0])
    bt = dvo.Batch(4, CAMS[0], 640, 480, 4, 1, cfg=_cfg())
    bt.set_intrinsics(np.stack([CAMS[int(c)] for c in cam]))
    for k in range(2):
        _feed(bt, "host", *_frames_of(cam, order, k))
    checked = 0
    for q in (0, 2):
        g, d, s, _ = _render(int(cam[q]))
        ref = orc.OFrame(g[order[q][0]], d[order[q][0]], s[order[q][0]], CAMS[int(cam[q])], 4, 1)
        obj = orc.OFrame(g[order[q][1]], d[order[q][1]], s[order[q][1]], CAMS[int(cam[q])], 4, 1)
        lg = bt.last_track_log(q)
        xi = np.zeros(6, np.float32)
        for l in range(4):
            for it in range(lg["n_iter"][l]):
                o = orc.optimize(obj.gray(l), ref.gray(l), ref.depth(l), ref.sigma(l), ref.K(l), xi, l)
                assert o["n_valid"] == lg["n_valid"][l][it], (q, l, it)
                xi = np.asarray(lg["xi_after"][l][it], np.float32)
                checked += 1
    bt.close()
    assert checked >= 8


def test_errors():
    import torch
    L = dvo.lib()
    B = 4
    bt = dvo.Batch(B, CAMS[0], 640, 480, 4, 1, cfg=_cfg())
    np.testing.assert_array_equal(bt.intrinsics(), np.stack([CAMS[0]] * B))
    Ks = np.stack([CAMS[c] for c in (0, 1, 2, 3)])
    for bad in ("nan", "fx0", "fy-"):
        K = Ks.copy()
        if bad == "nan":
            K[2, 1, 2] = np.nan
        elif bad == "fx0":
            K[1, 0, 0] = 0.0
        else:
            K[3, 1, 1] = -400.0
        assert L.dvo_batch_set_intrinsics(bt._p, K.ctypes.data_as(C.c_void_p)) == 1, bad
    np.testing.assert_array_equal(bt.intrinsics(), np.stack([CAMS[0]] * B))   # a refused table changes nothing
    assert L.dvo_batch_set_intrinsics(None, Ks.ctypes.data_as(C.c_void_p)) == 1
    bt.set_intrinsics(Ks.reshape(B, 9))
    np.testing.assert_array_equal(bt.intrinsics(), Ks)
    bt.set_intrinsics(None)
    np.testing.assert_array_equal(bt.intrinsics(), np.stack([CAMS[0]] * B))
    # a prefetched frame waiting -> NOT_READY
    g, d, s = _frames_of(np.zeros(B, int), np.zeros((B, N_FRAMES), int), 0)
    t = [torch.from_numpy(x).cuda() for x in (g, d, s)]
    torch.cuda.synchronize()
    bt.prefetch_device(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr())
    assert L.dvo_batch_set_intrinsics(bt._p, Ks.ctypes.data_as(C.c_void_p)) == 5
    bt.push_device(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr())
    bt.set_intrinsics(Ks)
    bt.synchronize()
    bt.close()
    mb = dvo.MonoBatch(2, CAMS[0], 640, 480)
    assert L.dvo_batch_set_intrinsics(mb._p, Ks[:2].ctypes.data_as(C.c_void_p)) == 1
    mb.close()
