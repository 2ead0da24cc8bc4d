"""Per-sequence skip / restart of a sensor-depth batch (dvo_batch_set_actions, include/dvo.h) on the GPU.

Every tracked sequence must give the bits of a single-sequence track against that sequence's own reference frame; skipped and
(re)started sequences report a zero twist, identity T and no iterations.  One tile size throughout (gn_pixels_per_thread = 4):
at one tile size every schedule gives the same bits (test_gpu_parity.py::test_batch_many_iterations_every_sequence_matches_single)."""
import ctypes as C

import numpy as np
import pytest

import dvo_amd as dvo
from util import K640, frames

pytestmark = pytest.mark.gpu

SKIP, TRACK, RESTART = dvo.SEQ_SKIP, dvo.SEQ_TRACK, dvo.SEQ_RESTART
TRACKED, SKIPPED, STARTED, BAD = dvo.SEQ_TRACKED, dvo.SEQ_SKIPPED, dvo.SEQ_STARTED, dvo.SEQ_BAD_ACTION
EYE = np.eye(4, dtype=np.float32)


def _logbits(lg):
    """(iterations per level, residual bits per level) of a track log: what must agree bit for bit"""
    return tuple(lg["n_iter"][:4]), tuple(np.asarray(r, np.float32).tobytes() for r in lg["residual"][:4])


def _cfg(**kw):
    return dvo.default_config(gn_pixels_per_thread=4, **kw)


def _schedule(B, n_push, seed, p=(0.3, 0.55, 0.15)):
    rng = np.random.RandomState(seed)
    order = np.stack([rng.permutation(6) for _ in range(B)])            # per-sequence frame order
    acts = rng.choice([SKIP, TRACK, RESTART], size=(n_push, B), p=p).astype(np.uint8)
    return order, acts


def _expected(order, acts):
    """Python model of the references: expected status and (object frame, reference frame) of every tracked sequence."""
    n_push, B = acts.shape
    ref = [None] * B
    status = np.zeros((n_push, B), np.int32)
    pairs = {}
    for k in range(n_push):
        for b in range(B):
            a, f = int(acts[k, b]), int(order[b][k])
            if a == TRACK and ref[b] is not None:
                status[k, b] = TRACKED
                pairs[(k, b)] = (f, ref[b])
                ref[b] = f
            elif a in (TRACK, RESTART):
                status[k, b] = STARTED
                ref[b] = f
            else:
                status[k, b] = SKIPPED if a == SKIP else BAD
    return status, pairs


def _inputs(order, acts, k, B):
    g, d, s, _ = frames(6, sigma=0.1)
    idx = [int(order[b][k]) for b in range(B)]
    gi, di, si = g[idx].copy(), d[idx].copy(), s[idx].copy()
    skip = np.array([acts[k, b] not in (TRACK, RESTART) for b in range(B)])
    gi[skip] = np.nan; di[skip] = np.nan; si[skip] = np.nan             # a skipped slot is never read
    return gi, di, si


def _run(cfg, order, acts, B, feed="host", device_actions=False):
    """Pushes of float maps with actions; returns per push (xi, T, status, n_iter [B][4], residual [B][4][32])."""
    import torch
    bt = dvo.Batch(B, K640, 640, 480, 4, 1, cfg=cfg)
    out = []
    for k in range(acts.shape[0]):
        gi, di, si = _inputs(order, acts, k, B)
        if device_actions:
            ta = torch.from_numpy(acts[k][:B].copy()).cuda()
            torch.cuda.synchronize()
            bt.set_actions(ta.data_ptr(), on_device=True)
        else:
            bt.set_actions(acts[k][:B])
        if feed == "host":
            bt.push_host(gi, di, si)
        else:
            t = [torch.from_numpy(x).cuda() for x in (gi, di, si)]
            torch.cuda.synchronize()
            bt.push_device(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr())
        xi, T = bt.last_poses()
        st = bt.last_status()
        logs = [bt.last_track_log(b) for b in range(B)]
        out.append((xi.copy(), T.copy(), st, np.array([lg["n_iter"][:4] for lg in logs]), [_logbits(lg) for lg in logs]))
    bt.close()
    return out


_single_cache = {}


def _single(obj, ref, cfg, tag=""):
    key = (obj, ref, tag)
    if key not in _single_cache:
        g, d, s, _ = frames(6, sigma=0.1)
        _single_cache[key] = dvo.track(g[obj], g[ref], d[ref], s[ref], K640, 4, 1, cfg=cfg)
    return _single_cache[key]


def _check_against_single(out, order, acts, cfg, seqs=None, tag=""):
    status, pairs = _expected(order, acts)
    n_tracked = 0
    for k, (xi, T, st, n_iter, res) in enumerate(out):
        np.testing.assert_array_equal(st, status[k][: len(st)], err_msg="push %d" % k)
        for b in (seqs if seqs is not None else range(len(st))):
            if st[b] == TRACKED:
                x1, lg = _single(*pairs[(k, b)], cfg, tag)
                np.testing.assert_array_equal(xi[b], x1, err_msg="push %d seq %d" % (k, b))
                assert res[b] == _logbits(lg), (k, b)
                n_tracked += 1
            else:
                assert not np.any(xi[b]), (k, b, xi[b])
                np.testing.assert_array_equal(T[b], EYE)
                assert not np.any(n_iter[b]), (k, b)
    return n_tracked


def _same(a, b, B=None):
    for (x0, T0, s0, n0, r0), (x1, T1, s1, n1, r1) in zip(a, b):
        sl = slice(0, B)
        np.testing.assert_array_equal(x0[sl], x1[sl]); np.testing.assert_array_equal(T0[sl], T1[sl])
        np.testing.assert_array_equal(s0[sl], s1[sl]); np.testing.assert_array_equal(n0[sl], n1[sl])
        assert r0[sl] == r1[sl]


@pytest.fixture(scope="module")
def base():
    order, acts = _schedule(16, 6, seed=5)
    out = _run(_cfg(), order, acts, 16)
    return order, acts, out


def test_random_schedule_matches_single_sequence_tracking(base):
    order, acts, out = base
    status, _ = _expected(order, acts)
    assert (status == TRACKED).sum() >= 20 and (status == SKIPPED).sum() >= 10 and (status == STARTED).sum() >= 16
    assert _check_against_single(out, order, acts, _cfg()) == (status == TRACKED).sum()


_STREAMS_XFAIL = ("plain pushes with track_streams=2 already differ from the single-sequence tracker on this workload (one sequence of 16 "
                  "stops a level early); the per-sequence path inherits that, see DESIGN.md section 12")


@pytest.mark.parametrize("variant", [pytest.param("track_streams=2", marks=pytest.mark.xfail(reason=_STREAMS_XFAIL, strict=False)),
                                     "track_fused_tiles=8", "gn_use_lds_patch=1", "B=6"])
def test_schedule_variants_give_identical_bits(base, variant):
    order, acts, ref = base
    if variant == "B=6":   # few sequences: one launch per iteration (k_track_gn_fused) on the levels that fit it
        _same(_run(_cfg(), order[:6], acts[:, :6].copy(), 6), ref, B=6)
        return
    name, value = variant.split("=")
    cfg = _cfg(**{name: int(value)})
    out = _run(cfg, order, acts, 16)
    if name == "gn_use_lds_patch":   # another tile shape (64 x 16 LDS tiles): the bits of the single-sequence tracker with that kernel
        status, _ = _expected(order, acts)
        assert _check_against_single(out, order, acts, cfg, tag=variant) == (status == TRACKED).sum()
        return
    _same(out, ref)


def test_all_track_actions_are_the_plain_path():
    g, d, s, _ = frames(6, sigma=0.1)
    B = 12
    order, _ = _schedule(B, 4, seed=9)
    def run(with_actions):
        bt = dvo.Batch(B, K640, 640, 480, 4, 1, cfg=_cfg())
        out = []
        for k in range(4):
            idx = [int(order[b][k]) for b in range(B)]
            if with_actions:
                bt.set_actions(np.full(B, TRACK, np.uint8))
            bt.push_host(g[idx], d[idx], s[idx])
            st = bt.last_status()
            assert (st == (STARTED if k == 0 else TRACKED)).all(), (k, st)
            if k > 0:
                out.append((bt.last_poses()[0].copy(), [_logbits(bt.last_track_log(b)) for b in range(B)]))
        bt.close()
        return out
    plain, acted = run(False), run(True)
    assert len(plain) == 3
    for (x0, r0), (x1, r1) in zip(plain, acted):
        np.testing.assert_array_equal(x0, x1)
        assert r0 == r1


def test_device_actions_and_device_pushes_match_host(base):
    order, acts, ref = base
    _same(_run(_cfg(), order, acts, 16, feed="device", device_actions=True), ref)


def _raw(order, acts, k, B):
    g, d, _, _ = frames(6, sigma=0.1)
    g8 = np.stack([np.clip(np.rint(g[int(order[b][k])] * 255), 0, 255).astype(np.uint8) for b in range(B)])
    d16 = np.stack([np.clip(np.rint(d[int(order[b][k])] * 5000), 0, 65535).astype(np.uint16) for b in range(B)])
    for b in range(B):
        if acts[k, b] not in (TRACK, RESTART):   # never read: garbage
            g8[b] = 0xA5; d16[b] = 0x5A5A
    return g8, d16


@pytest.mark.parametrize("feed", ["raw_device", "raw_host"])
def test_raw_pushes_match_one_sequence_batches(feed):
    import torch
    B, n_push = 8, 5
    order, acts = _schedule(B, n_push, seed=21)
    status, _ = _expected(order, acts)
    assert (status == TRACKED).sum() >= 6 and (status == SKIPPED).sum() >= 4
    bt = dvo.Batch(B, K640, 640, 480, 4, 1, cfg=_cfg())
    got = []
    for k in range(n_push):
        g8, d16 = _raw(order, acts, k, B)
        bt.set_actions(acts[k])
        if feed == "raw_host":
            bt.push_raw_host(g8, d16)
        else:
            tg = torch.from_numpy(g8).cuda(); td = torch.from_numpy(d16.view(np.int16)).cuda(); torch.cuda.synchronize()
            bt.push_raw_device(tg.data_ptr(), 1, td.data_ptr())
        got.append((bt.last_poses()[0].copy(), bt.last_status(), [bt.last_track_log(b) for b in range(B)]))
    bt.close()
    for b in range(B):   # a 1-sequence batch fed only this sequence's frames, recreated at every (re)start
        one = None
        for k in range(n_push):
            xi, st, res = got[k]
            assert st[b] == status[k, b], (k, b)
            if status[k, b] in (SKIPPED, BAD):
                assert not np.any(xi[b])
                continue
            g8, d16 = _raw(order, acts, k, B)
            if status[k, b] == STARTED:
                if one is not None:
                    one.close()
                one = dvo.Batch(1, K640, 640, 480, 4, 1, cfg=_cfg())
            one.push_raw_host(g8[b:b + 1], d16[b:b + 1])
            if status[k, b] == TRACKED:
                np.testing.assert_array_equal(xi[b], one.last_poses()[0][0], err_msg="push %d seq %d" % (k, b))
                assert _logbits(res[b]) == _logbits(one.last_track_log(0)), (k, b)
            else:
                assert not np.any(xi[b])
        if one is not None:
            one.close()


def test_scale_1024_sequences():
    import torch
    g, d, s, _ = frames(6, sigma=0.1)
    B, n_push = 1024, 3
    rng = np.random.RandomState(3)
    order = np.stack([rng.permutation(6) for _ in range(B)])
    acts = rng.choice([SKIP, TRACK, RESTART], size=(n_push, B), p=(0.3, 0.68, 0.02)).astype(np.uint8)
    status, pairs = _expected(order, acts)
    G = [torch.from_numpy(x).cuda() for x in (g, d, s)]
    bt = dvo.Batch(B, K640, 640, 480, 4, 1, cfg=_cfg())
    sample = rng.choice(B, 32, replace=False)
    checked = 0
    for k in range(n_push):
        idx = torch.from_numpy(order[:, k].astype(np.int64)).cuda()
        t = [x.index_select(0, idx) for x in G]
        skip = torch.from_numpy(np.isin(acts[k], (TRACK, RESTART), invert=True)).cuda()
        for x in t:
            x[skip] = float("nan")
        torch.cuda.synchronize()
        bt.set_actions(acts[k])
        bt.push_device(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr())
        xi, T = bt.last_poses()
        np.testing.assert_array_equal(bt.last_status(), status[k])
        off = status[k] != TRACKED
        assert not np.any(xi[off])
        np.testing.assert_array_equal(T[off], np.broadcast_to(EYE, T[off].shape))
        for b in sample:
            if status[k, b] == TRACKED:
                x1, lg = _single(*pairs[(k, b)], _cfg())
                np.testing.assert_array_equal(xi[b], x1)
                assert _logbits(bt.last_track_log(int(b))) == _logbits(lg)
                checked += 1
        del t
    bt.close()
    assert checked >= 20


def test_errors_and_status():
    import torch
    g, d, s, _ = frames(6, sigma=0.1)
    L = dvo.lib()
    B = 4
    bt = dvo.Batch(B, K640, 640, 480, 4, 1, cfg=_cfg())
    with pytest.raises(dvo.DvoError, match="not ready"):
        bt.last_status()
    idx = [0, 1, 2, 3]
    bt.push_host(g[idx], d[idx], s[idx])
    assert (bt.last_status() == STARTED).all()
    bt.push_host(g[[1, 2, 3, 4]], d[[1, 2, 3, 4]], s[[1, 2, 3, 4]])
    assert (bt.last_status() == TRACKED).all()
    # an action outside {0, 1, 2}: BAD_ACTION, handled as SKIP (slot not read, reference kept)
    gi, di, si = g[[2, 3, 4, 5]].copy(), d[[2, 3, 4, 5]].copy(), s[[2, 3, 4, 5]].copy()
    gi[1] = np.nan; di[1] = np.nan; si[1] = np.nan
    bt.set_actions(np.array([TRACK, 7, TRACK, SKIP], np.uint8))
    bt.push_host(gi, di, si)
    st = bt.last_status()
    assert list(st) == [TRACKED, BAD, TRACKED, SKIPPED]
    xi = bt.last_poses()[0]
    assert not np.any(xi[1]) and not np.any(xi[3])
    np.testing.assert_array_equal(xi[0], dvo.track(g[2], g[1], d[1], s[1], K640, 4, 1, cfg=_cfg())[0])
    # copy_status_device equals last_status
    dst = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    bt.copy_status_device(dst.data_ptr())
    bt.synchronize()
    np.testing.assert_array_equal(dst.cpu().numpy(), st)
    # the kept references: sequence 1 still holds frame 2 (BAD_ACTION = SKIP), sequence 3 frame 4
    bt.push_host(g[[0, 0, 0, 0]], d[[0, 0, 0, 0]], s[[0, 0, 0, 0]])   # (all-TRACK through the per-sequence path)
    assert (bt.last_status() == TRACKED).all()
    xi = bt.last_poses()[0]
    np.testing.assert_array_equal(xi[1], dvo.track(g[0], g[2], d[2], s[2], K640, 4, 1, cfg=_cfg())[0])
    np.testing.assert_array_equal(xi[3], dvo.track(g[0], g[4], d[4], s[4], K640, 4, 1, cfg=_cfg())[0])
    # raw frames after float maps with actions: the weight storage would differ -> BAD_ARGUMENT, nothing enqueued
    bt.set_actions(np.full(B, TRACK, np.uint8))
    g8 = np.zeros((B, 480, 640), np.uint8); d16 = np.zeros((B, 480, 640), np.uint16)
    with pytest.raises(dvo.DvoError, match="bad argument"):
        bt.push_raw_host(g8, d16)
    # set_actions with a prefetched frame pending -> NOT_READY; prefetch with actions pending -> NOT_READY
    bt.set_actions(None)
    t = [torch.from_numpy(x[[1, 1, 1, 1]]).cuda() for x in (g, d, s)]
    torch.cuda.synchronize()
    bt.prefetch_device(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr())
    assert L.dvo_batch_set_actions(bt._p, np.ones(B, np.uint8).ctypes.data_as(C.c_void_p), 0) == 5
    bt.push_device(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr())
    bt.set_actions(np.ones(B, np.uint8))
    assert L.dvo_batch_prefetch_device(bt._p, C.c_void_p(t[0].data_ptr()), C.c_void_p(t[1].data_ptr()), C.c_void_p(t[2].data_ptr())) == 5
    bt.synchronize()
    bt.close()
    # a mono batch refuses actions
    mb = dvo.MonoBatch(2, K640, 640, 480)
    assert L.dvo_batch_set_actions(mb._p, np.ones(2, np.uint8).ctypes.data_as(C.c_void_p), 0) == 1
    mb.close()
