"""The binomial-filtered gray pyramid of a sensor-depth batch (dvo_batch_set_pyramid_filter, dvo_op_pyramid_frames_filtered;
include/dvo.h) on the GPU.

The operator gives the numpy replica of the contract (tests/pyramid_filter_ref.py) bit for bit at every level, for raw and float
feeds with holes, NaN, -inf, DVO_INVALID blocks and +inf at a corner, on an edge and in the interior; depth, sigma and wgt are
dvo_op_pyramid_frames' bits; the valid sets are the plain build's; nothing is NaN below an unchanged top.  filter = NONE is the plain
operator and the plain batch.  A batch's frame and keyframe maps equal the replica for every feed.  Planned builds copy every level
of a SKIP sequence forward.  Every logged Gauss-Newton iteration of a filtered batch is the oracle's on the replica's maps, alone and
under the robust and the geometric term.  Every refusal is returned.  On noisy pairs the filtered batch beats the plain one by the
replica's margin.

The operator's shapes are those of tests/test_gpu_pyramid_build.py (the lx >= w[l] / ly >= h[l] guards fire at each).  Which instance
runs: k_pyramid_filter_top<CULLS, RAW, PLAN, WIDE>; WIDE (16-byte staging loads) needs culls > 0 and one-channel bytes with a width
that is a multiple of 16, or float maps with a width that is a multiple of 4 -- 144 and 176 for bytes, 88 and 176 for floats; 88 (bytes),
90 and 178 are the ragged widths of the scalar fallback.  The level maps are stored one float at a time, so a batch of 3 (level
pointers off 16 bytes) runs the same instance as a batch of 4; both run.  The batch tests use tests/term_batch.py's 320x240
frames, 3 levels, culls 1."""
import ctypes as C
import functools

import numpy as np
import pytest

import dvo_amd as dvo
import geometric_ref as gr
import gn_sums
import orc
import pyramid_filter_ref as fref
import pyramid_ref as pref
import robust_ref as rr
import test_gpu_pyramid_build as tb
import term_batch as tm
from term_batch import CULLS, KH, LEVELS, SIZE, TOP
from util import K640, TOL_BACKWARD, backward_error

pytestmark = pytest.mark.gpu

F32 = np.float32
S, T, R = pref.SEQ_SKIP, pref.SEQ_TRACK, pref.SEQ_RESTART
TRACKED = dvo.SEQ_TRACKED
BINOMIAL3, NONE = dvo.PYRAMID_FILTER_BINOMIAL3, dvo.PYRAMID_FILTER_NONE
BAD = dvo.DVO_ERR_BAD_ARGUMENT


@pytest.fixture(scope="module", autouse=True)
def _oracle_steps():
    with tm.oracle_steps():
        yield


def _name(culls, raw, plan, wide):
    b = lambda v: "true" if v else "false"
    return "k_pyramid_filter_top<%d, %s, %s, %s>" % (culls, b(raw), b(plan), b(wide))


_bits = tb._bits


# ------------------------------------------------------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=None)
def _raw(n, h, w, channels, seed):
    """test_gpu_pyramid_build's raw frames (isolated d == 0 pixels and zero blocks) plus a zero checkerboard, a zero block in a corner
    and one on an edge"""
    rgb, d16 = tb._raw(n, h, w, channels, seed)
    d16 = d16.copy()
    yy, xx = np.mgrid[0:h, 0:w]
    board = ((yy + xx) % 2 == 0) & (yy >= 10) & (yy < 22) & (xx >= 12) & (xx < 30)
    d16[:, board] = 0
    d16[:, h - 3:, w - 4:] = 0
    d16[:, 14:19, :3] = 0
    d16.setflags(write=False)
    return rgb, d16


@functools.lru_cache(maxsize=None)
def _float(n, h, w, seed):
    """test_gpu_pyramid_build's float maps (3 % each of NaN, -7, INVALID, -inf, +inf, 0) with, in the gray, a NaN, a -inf and a +inf
    pixel and an INVALID block each at a corner, on an edge and in the interior"""
    g, d, s = tb._float(n, h, w, seed)
    g = g.copy()
    for q in range(n):
        g[q, 0, 0], g[q, 0, w - 1], g[q, h - 1, 0] = (np.nan, -np.inf, np.inf) if q % 2 == 0 else (np.inf, np.nan, -np.inf)
        g[q, h - 2:, w - 2:] = pref.INVALID                                                  # corner block
        g[q, 0, 10], g[q, 12, 0], g[q, h - 1, 7] = -np.inf, np.inf, np.nan                   # edges
        g[q, 16:19, w - 2:] = pref.INVALID
        g[q, 9, 13], g[q, 10, 20], g[q, 15, 9] = np.nan, -np.inf, np.inf                     # interior
        g[q, 6:10, 16:21] = pref.INVALID
    g.setflags(write=False)
    return g, d, s


def _dyadic(n, h, w, seed):
    """gray as multiples of 2^-8 in [0, 1] with holes: every partial sum of one halving is exact in float32"""
    rng = np.random.RandomState(seed)
    g = (rng.randint(0, 257, (n, h, w)) / 256.0).astype(F32)
    g[rng.rand(n, h, w) < 0.05] = pref.INVALID
    g[:, 5:9, 7:12] = pref.INVALID
    return g


def _op(kind, w, h, levels, culls, n, channels=1, depth=True, custom_cfg=False, seed=1, actions=None, filt=BINOMIAL3, flags=0):
    """one filtered op call, its replica and the plain op call on the same input; with actions: the planned build, a SKIP sequence's
    second frame being garbage"""
    cfg, cd = tb._cfg(custom_cfg)
    if kind == "raw":
        rgb, d16 = _raw(n, h, w, channels, seed)
        d16 = d16 if depth else None
        first = dict(rgb=rgb, depth16=d16)
        build = lambda f: fref.build_raw(w, h, levels, culls, f["rgb"], f["depth16"], cfg=cd)
        garbage = {"rgb": 0xA5, "depth16": 0x5A5A}
        src = _raw(n, h, w, channels, seed + 50)
        second = dict(rgb=src[0].copy(), depth16=src[1].copy() if depth else None)
    else:
        g, d, s = _float(n, h, w, seed)
        first = dict(gray=g, depth=d if depth else None, sigma=s if depth else None)
        build = lambda f: fref.build(w, h, levels, culls, f["gray"], f["depth"], f["sigma"], cfg=cd)
        garbage = dict(gray=12345.0, depth=12345.0, sigma=12345.0)
        src = _float(n, h, w, seed + 50)
        second = dict(gray=src[0].copy(), depth=src[1].copy() if depth else None, sigma=src[2].copy() if depth else None)
    kw = dict(first, flags=flags, cfg=cfg)
    want = build(first)
    if actions is not None:
        for q, a in enumerate(actions):
            if a == S:
                for m, v in garbage.items():
                    if second[m] is not None:
                        second[m][q] = v
        kw.update(seq_action=np.array(actions, np.uint8), second=second)
        want = fref.planned(want, build(second), actions, levels)
    got = dvo.op_pyramid_frames_filtered(w, h, levels, culls, filt, **kw)
    plain = dvo.op_pyramid_frames(w, h, levels, culls, **kw)
    return got, want, plain


MIX = tb.MIX
G0 = dict(w=37, h=29, levels=3, culls=0)
G1, G2, S1 = tb.G1, tb.G2, tb.S1
CASES = {}
for n in (3, 4, 8):
    CASES["raw-culls1-wide-n%d" % n] = ("raw", dict(S1, n=n), _name(1, 1, 0, 1))            # 144 x 144, levels 5: the split's geometry
    CASES["raw-culls2-wide-n%d" % n] = ("raw", dict(G2, n=n, custom_cfg=n == 4), _name(2, 1, 0, 1))
    CASES["float-culls1-wide-n%d" % n] = ("float", dict(G1, n=n), _name(1, 0, 0, 1))
CASES["float-culls2-wide"] = ("float", dict(G2, n=3, custom_cfg=True), _name(2, 0, 0, 1))
CASES["raw-culls1-width88"] = ("raw", dict(G1, n=4), _name(1, 1, 0, 0))                    # 88 is no multiple of 16
CASES["raw-culls1-width90-height73"] = ("raw", dict(G1, w=90, h=73, n=3), _name(1, 1, 0, 0))
CASES["raw-culls2-width178-height147"] = ("raw", dict(G2, w=178, h=147, n=4), _name(2, 1, 0, 0))
CASES["float-culls1-width90-height73"] = ("float", dict(G1, w=90, h=73, n=3), _name(1, 0, 0, 0))
CASES["float-culls2-width178-height147"] = ("float", dict(G2, w=178, h=147, n=4), _name(2, 0, 0, 0))
CASES["rgb-culls1"] = ("raw", dict(G1, n=4, channels=3), _name(1, 1, 0, 0))
CASES["rgba-culls2"] = ("raw", dict(G2, n=3, channels=4), _name(2, 1, 0, 0))
CASES["raw-gray-only-culls2"] = ("raw", dict(G2, n=4, depth=False), _name(2, 1, 0, 1))
CASES["float-gray-only-culls1"] = ("float", dict(G1, n=3, depth=False), _name(1, 0, 0, 1))
CASES["float-culls0"] = ("float", dict(G0, n=3, custom_cfg=True), _name(0, 0, 0, 0))
CASES["raw-culls0"] = ("raw", dict(G0, n=4), _name(0, 1, 0, 0))
CASES["plan-raw-culls1-wide"] = ("raw", dict(S1, n=8, actions=MIX), _name(1, 1, 1, 1))
CASES["plan-raw-culls2-wide"] = ("raw", dict(G2, n=8, actions=MIX, custom_cfg=True), _name(2, 1, 1, 1))
CASES["plan-raw-culls1-five-sequences"] = ("raw", dict(G1, w=90, h=73, n=5, actions=MIX[:5]), _name(1, 1, 1, 0))
CASES["plan-rgb-culls2"] = ("raw", dict(G2, w=178, h=147, n=8, channels=3, actions=MIX), _name(2, 1, 1, 0))
CASES["plan-float-culls1-wide"] = ("float", dict(G1, n=8, actions=MIX), _name(1, 0, 1, 1))
CASES["plan-float-culls2-wide-all-skip"] = ("float", dict(G2, n=8, actions=tb.ALL_SKIP), _name(2, 0, 1, 1))
CASES["plan-float-culls1-width90"] = ("float", dict(G1, w=90, h=73, n=8, actions=MIX), _name(1, 0, 1, 0))
CASES["plan-float-culls2-width178-gray"] = ("float", dict(G2, w=178, h=147, n=8, depth=False, actions=MIX), _name(2, 0, 1, 0))
CASES["plan-float-culls0"] = ("float", dict(G0, n=8, actions=MIX), _name(0, 0, 1, 0))
CASES["plan-raw-culls0-no-skip"] = ("raw", dict(G0, n=8, actions=tb.NO_SKIP), _name(0, 1, 1, 0))
INSTANCES = {_name(0, r, p, 0) for r in (0, 1) for p in (0, 1)} | {_name(c, r, p, v) for c in (1, 2) for r in (0, 1) for p in (0, 1) for v in (0, 1)}


def test_the_cases_name_every_instance():
    assert {kernel for _, _, kernel in CASES.values()} == INSTANCES and len(INSTANCES) == 20


@pytest.mark.parametrize("case", sorted(CASES))
def test_operator_matches_the_replica(case):
    kind, kw, kernel = CASES[case]
    w, h, levels, culls, n = (kw[k] for k in ("w", "h", "levels", "culls", "n"))
    assert pref.guards_fire(w, h, levels, culls) == (True, True), "the geometry fires no guard"
    got, want, plain = _op(kind, **kw)
    assert got["kernel"].kind == dvo.PYRAMID_KERNEL_FILTER and got["kernel"].name() == kernel, "%s ran %s" % (case, got["kernel"].name())
    assert plain["kernel"].kind != dvo.PYRAMID_KERNEL_FILTER
    tb._assert_maps(got, want, n, "%s [%s]" % (case, kernel))
    top = levels - 1
    for l in range(levels):
        for m in ("depth", "sigma", "wgt"):
            assert np.array_equal(_bits(got[m][l]), _bits(plain[m][l])), "%s: %s level %d is not the plain build's" % (case, m, l)
        assert np.array_equal(fref.valid(got["gray"][l]), fref.valid(plain["gray"][l])), "%s: valid set of level %d" % (case, l)
        if culls > 0 or l < top:
            assert not np.isnan(got["gray"][l]).any(), "%s: NaN at level %d" % (case, l)
    # the frames do what the case needs: holes and valid pixels at the top, the filter changed something, a hole next to a valid centre
    gt = got["gray"][top]
    assert fref.valid(gt).any() and ((gt == pref.INVALID).any() or (kind == "raw" and not kw.get("depth", True)))   # (bytes without depth have no holes)
    if culls > 0:
        assert not np.array_equal(_bits(gt), _bits(plain["gray"][top]))
    assert not np.array_equal(_bits(got["gray"][0]), _bits(plain["gray"][0]))
    if kind == "float" and kw.get("actions") is None:
        assert np.isinf(got["gray"][top]).any()                                  # +inf is a valid tap: it passes through
        if culls == 0:
            assert np.isnan(gt[0, 0, 0])                                         # the unchanged top keeps its NaN
    if kw.get("actions") is not None and S in kw["actions"]:
        q = kw["actions"].index(S)
        assert not (gt[q] == 12345.0).any() and not (gt[q] == F32(0xA5) * F32(1.0 / 255.0)).all()   # the garbage frame was not read


@pytest.mark.parametrize("culls,w,h", [(1, 88, 72), (1, 90, 73), (2, 176, 144)])
def test_dyadic_input_equals_the_exact_convolution(culls, w, h):
    """gray as multiples of 2^-8: the top level of culls 1, and at culls 2 the level the first halving would store, equal a float64
    convolution with renormalisation rounded once, bit for bit (one halving: what it divides by 9 or 12 is no longer dyadic)"""
    g = _dyadic(3, h, w, 11)
    got = dvo.op_pyramid_frames_filtered(w, h, 2, culls, gray=g)
    exact = fref.halve_exact(g)
    if culls == 1:
        assert got["kernel"].name() == _name(1, 0, 0, w % 4 == 0)
        assert np.array_equal(_bits(got["gray"][1]), _bits(exact))
    else:   # the intermediate map is never stored: hold the top to H of the exact intermediate
        assert np.array_equal(_bits(got["gray"][1]), _bits(fref.halve(exact)))
    assert np.array_equal(_bits(got["gray"][0]), _bits(fref.halve(got["gray"][1])))


def test_forced_scalar_fallback_gives_the_same_bits(monkeypatch):
    """DVO_PYRAMID_FILTER_SCALAR: the one-pixel staging loads at a shape the wide instance accepts"""
    wide, want, _ = _op("raw", n=4, **G2)
    monkeypatch.setenv("DVO_PYRAMID_FILTER_SCALAR", "1")
    one, _, _ = _op("raw", n=4, **G2)
    assert (wide["kernel"].name(), one["kernel"].name()) == (_name(2, 1, 0, 1), _name(2, 1, 0, 0))
    tb._assert_maps(one, want, 4, "forced scalar")


# ------------------------------------------------------------------------------------------------------------------ equivalences
@pytest.mark.parametrize("case", ["raw-rows", "raw-split", "float-plan"])
def test_filter_none_is_the_plain_operator(case):
    kind, kw = {"raw-rows": ("raw", dict(G1, n=4, flags=dvo.PYRAMID_ROWS_DECIMATED)), "raw-split": ("raw", dict(S1, n=4, flags=dvo.PYRAMID_SPLIT)),
                "float-plan": ("float", dict(G0, n=8, actions=MIX))}[case]
    flags = kw.pop("flags", 0)
    dec = lambda a: a if a is None or not (flags & dvo.PYRAMID_ROWS_DECIMATED) else a[:, ::1 << kw["culls"]]
    if kind == "raw":
        rgb, d16 = _raw(kw["n"], kw["h"], kw["w"], 1, 1)
        args = dict(rgb=dec(rgb), depth16=dec(d16), flags=flags)
    else:
        g, d, s = _float(kw["n"], kw["h"], kw["w"], 2)
        args = dict(gray=g, depth=d, sigma=s, seq_action=np.array(kw["actions"], np.uint8), second=dict(gray=g[::-1], depth=d[::-1], sigma=s[::-1]))
    a = dvo.op_pyramid_frames(kw["w"], kw["h"], kw["levels"], kw["culls"], **args)
    b = dvo.op_pyramid_frames_filtered(kw["w"], kw["h"], kw["levels"], kw["culls"], NONE, **args)
    assert a["kernel"].name() == b["kernel"].name() and (a["kernel"].kind, a["kernel"].culls, a["kernel"].plan) == (b["kernel"].kind, b["kernel"].culls, b["kernel"].plan)
    for m in pref.MAPS:
        for l in range(kw["levels"]):
            assert a[m][l].tobytes() == b[m][l].tobytes(), (m, l)


def _raw_of(m):
    return np.clip(np.rint(m[0] * 255), 0, 255).astype(np.uint8), np.clip(np.rint(m[1] * 5000), 0, 65535).astype(np.uint16)


def _holes(k, b, g, d):
    """holes of push k, sequence b: a zero-depth block, a zero checkerboard and single pixels (raw: they invalidate the gray)"""
    d = d.copy()
    d[30 + 7 * b:44 + 7 * b, 50 + 11 * k:75 + 11 * k] = 0
    yy, xx = np.mgrid[0:d.shape[0], 0:d.shape[1]]
    d[((yy + xx) % 2 == 0) & (yy >= 100) & (yy < 120) & (xx >= 200 + 5 * b) & (xx < 230 + 5 * b)] = 0
    d[::37, ::41] = 0
    d[:3, :5] = 0
    return g, d


def _run(B, idx, filt=BINOMIAL3, set_it=True, feed="device", cfg=None, kf=False, acts=None, cams=None, rob=None, geo=None, holes=False, garbage=False):
    """idx[k][b]: frame of sequence b at push k.  feed: device / host (float maps), raw / raw_host (bytes; with holes the gray of a
    pixel without depth is invalid), ingested (the float maps dvo.ingest makes of the raw frames, on the device), prefetch (device
    float maps, prefetched before their push).  garbage: a SKIP sequence's slot of the input holds garbage.
    Per push: dict(status, xi, T, logs, frames[b][l] = (gray, depth), kf[b][l], maps[b] = the float (gray, depth, sigma) the push is
    equivalent to, ...)"""
    g, d, s = tm.frames()
    cfg = cfg if cfg is not None else tm.cfg()
    bt = dvo.Batch(B, KH, SIZE[0], SIZE[1], LEVELS, CULLS, cfg=cfg)
    if kf:
        bt.set_keyframe_tracking(True)
    bt.set_track_quality(True)
    if cams is not None:
        bt.set_intrinsics(cams)
    if set_it:
        bt.set_pyramid_filter(filt)
        assert bt.pyramid_filter() == filt
    if rob:
        bt.set_robust_weights(**rob)
    if geo:
        bt.set_geometric(**geo)
    keep, outs = [], []

    def tensors(k):
        maps = []
        for b in range(B):
            i = idx[k][b]
            gi, di, si = g[i], d[i], s[i]
            if feed in ("raw", "raw_host", "ingested"):
                g8, d16 = _raw_of((gi, di))
                if holes:
                    g8, d16 = _holes(k, b, g8, d16)
                gi, di, si = pref.convert(g8[None], d16[None])
                maps.append((gi[0], di[0], si[0], g8, d16))
            else:
                if holes:
                    gi = gi.copy()
                    gi[_holes(k, b, gi, di)[1] == 0] = pref.INVALID
                maps.append((gi, di, si))
        return maps

    def push(k, maps, prefetch_only=False):
        if feed in ("raw", "raw_host"):
            g8 = np.stack([m[3] for m in maps]); d16 = np.stack([m[4] for m in maps])
            if garbage and acts is not None:
                for b in range(B):
                    if acts[k][b] == S:
                        g8[b] = 0xA5; d16[b] = 0x5A5A
            if feed == "raw_host":
                bt.push_raw_host(g8, d16)
            else:
                import torch
                tg = tm.dev(g8); td = torch.from_numpy(d16.view(np.int16)).cuda()
                torch.cuda.synchronize()
                keep.append((tg, td))
                bt.push_raw_device(tg.data_ptr(), 1, td.data_ptr())
            return
        arr = [np.ascontiguousarray(np.stack([m[j] for m in maps])) for j in range(3)]
        if garbage and acts is not None:
            for b in range(B):
                if acts[k][b] == S:
                    for a in arr:
                        a[b] = 12345.0
        if feed == "host":
            bt.push_host(*arr)
            return
        t = [tm.dev(x) for x in arr]
        keep.append(t)
        if prefetch_only:
            bt.prefetch_device(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr())
        else:
            bt.push_device(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr())
        return t

    for k in range(len(idx)):
        maps = tensors(k)
        if acts is not None:
            bt.set_actions(np.asarray(acts[k], np.uint8))
        if feed == "prefetch" and k > 0:
            t = push(k, maps, prefetch_only=True)
            bt.push_device(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr())
        else:
            push(k, maps)
        o = dict(status=bt.last_status(), maps=[m[:3] for m in maps], frames=[[bt.frame(b, l) for l in range(LEVELS)] for b in range(B)])
        if kf:
            o["kf"] = [[bt.keyframe(b, l) for l in range(LEVELS)] for b in range(B)]
            o["world"] = bt.world_poses()
        if k > 0 or acts is not None or kf:
            xi, Tm = bt.last_poses()
            o.update(xi=xi.copy(), T=Tm.copy(), logs=[bt.last_track_log(b) for b in range(B)], q=bt.last_track_quality())
        if rob:
            o["s2"] = bt.last_robust_scales()
        if geo:
            o["grec"] = bt.last_geometric()
            o["glogs"] = [bt.last_geometric_log(b) for b in range(B)]
        outs.append(o)
    bt.close()
    return outs


def _same(a, b):
    assert len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        np.testing.assert_array_equal(x["status"], y["status"], err_msg="push %d" % k)
        for bq, (fx, fy) in enumerate(zip(x["frames"], y["frames"])):
            for l in range(LEVELS):
                assert fx[l][0].tobytes() == fy[l][0].tobytes() and fx[l][1].tobytes() == fy[l][1].tobytes(), (k, bq, l)
        if "xi" in x:
            assert x["xi"].tobytes() == y["xi"].tobytes() and x["T"].tobytes() == y["T"].tobytes(), "push %d poses" % k
            assert [tm.logbits(l) for l in x["logs"]] == [tm.logbits(l) for l in y["logs"]], "push %d logs" % k
            assert x["q"].tobytes() == y["q"].tobytes(), "push %d records" % k


@pytest.mark.parametrize("mode", ["plain", "keyframes", "raw"])
def test_a_batch_with_none_set_is_a_batch_that_never_called_the_setter(mode):
    kw = dict(kf=mode == "keyframes", feed="raw" if mode == "raw" else "device")
    _same(_run(5, tm.wide_idx(5), NONE, **kw), _run(5, tm.wide_idx(5), set_it=False, **kw))


# ------------------------------------------------------------------------------------------------------------------ batch maps
def _replica_of(m):
    """the filtered build of one sequence's float (gray, depth, sigma): per-level gray and depth"""
    b = fref.build(SIZE[0], SIZE[1], LEVELS, CULLS, m[0][None], m[1][None], m[2][None])
    return [(b["gray"][l][0], b["depth"][l][0]) for l in range(LEVELS)]


def _assert_frames(outs, what):
    for k, o in enumerate(outs):
        for b, m in enumerate(o["maps"]):
            if o["status"][b] == dvo.SEQ_SKIPPED:
                continue
            want = _replica_of(m)
            for l in range(LEVELS):
                for j, name in ((0, "gray"), (1, "depth")):
                    assert np.array_equal(_bits(o["frames"][b][l][j]), _bits(want[l][j])), "%s: push %d sequence %d level %d %s" % (what, k, b, l, name)


@pytest.mark.parametrize("feed", ["device", "host", "raw", "raw_host", "prefetch"])
@pytest.mark.parametrize("B", [3, 4])
def test_batch_frames_equal_the_replica(feed, B):
    outs = _run(B, tm.wide_idx(B), feed=feed, holes=True)
    _assert_frames(outs, feed)
    top = outs[1]["frames"][0][TOP][0]
    assert (top == pref.INVALID).any() and fref.valid(top).sum() > top.size // 2
    assert all(o["status"][0] == TRACKED for o in outs[1:]) and np.abs(outs[2]["xi"]).max() > 0


def test_the_raw_path_equals_the_ingested_float_path():
    a = _run(4, tm.wide_idx(4), feed="raw", holes=True)
    b = _run(4, tm.wide_idx(4), feed="ingested", holes=True, cfg=tm.cfg())
    # (raw frames keep no weight maps where min_depth allows: the estimator's inputs are the same values, the poses the same bits)
    for k, (x, y) in enumerate(zip(a, b)):
        for bq in range(4):
            for l in range(LEVELS):
                assert x["frames"][bq][l][0].tobytes() == y["frames"][bq][l][0].tobytes(), (k, bq, l)
                assert x["frames"][bq][l][1].tobytes() == y["frames"][bq][l][1].tobytes(), (k, bq, l)
        if k > 0:
            assert x["xi"].tobytes() == y["xi"].tobytes(), k


def test_keyframe_maps_equal_the_replica():
    outs = _run(4, tm.wide_idx(4), kf=True, holes=True)
    _assert_frames(outs, "keyframes")
    made = [0] * 4      # the push that made each sequence's current keyframe
    for k, o in enumerate(outs):
        for b in range(4):
            if k > 0 and o["world"][2][b]:
                made[b] = k
            want = _replica_of(outs[made[b]]["maps"][b])
            for l in range(LEVELS):
                kfm = o["kf"][b][l]
                assert np.array_equal(_bits(kfm["gray"]), _bits(want[l][0])) and np.array_equal(_bits(kfm["depth"]), _bits(want[l][1])), (k, b, l)


# ------------------------------------------------------------------------------------------------------------------ plan
ACTS = [[T, T, T, T, T], [S, T, R, T, S], [T, S, T, R, S], [T, T, S, T, T]]


@pytest.mark.parametrize("feed", ["device", "raw"])
def test_skip_copies_every_level_forward_and_restart_builds(feed):
    """garbage in the skipped input slots; a skipped sequence keeps the frame set of its last built push at every level"""
    idx = [r[:5] for r in (tm.wide_idx(5) + [[4, 1, 4, 3, 2]])]
    outs = _run(5, idx, feed=feed, acts=ACTS, holes=True, garbage=True)
    last = [0] * 5
    n_skip = 0
    for k, o in enumerate(outs):
        for b in range(5):
            if o["status"][b] == dvo.SEQ_SKIPPED:
                n_skip += 1
            else:
                last[b] = k
            want = _replica_of(outs[last[b]]["maps"][b])
            for l in range(LEVELS):
                assert np.array_equal(_bits(o["frames"][b][l][0]), _bits(want[l][0])), (k, b, l, "gray")
                assert np.array_equal(_bits(o["frames"][b][l][1]), _bits(want[l][1])), (k, b, l, "depth")
    assert n_skip == 5 and outs[1]["status"][2] == dvo.SEQ_STARTED and outs[3]["status"][0] == TRACKED


def test_per_sequence_intrinsics_table():
    cams = np.stack([KH.reshape(3, 3) * np.array([[1 + 0.01 * b], [1 - 0.01 * b], [1]], F32) for b in range(4)]).astype(F32)
    outs = _run(4, tm.wide_idx(4), cams=cams, holes=True)
    _assert_frames(outs, "intrinsics table")
    assert all((o["status"] == TRACKED).all() for o in outs[1:])


def test_the_split_geometry_is_not_split_under_the_filter(monkeypatch):
    """144x144, levels 5, raw frames, DVO_PYRAMID_SPLIT=1: without the filter the batch splits its build; with it every level is the
    replica's (the split stages would store decimated gray)"""
    import test_gpu_pyramid_split as ts
    import torch
    monkeypatch.setenv("DVO_PYRAMID_SPLIT", "1")
    w = h = 144
    gray, depth = ts._frames(w, h, 2, 5)
    bt = dvo.Batch(ts.N_SEQ, ts._K(w), w, h, 5, 1)
    bt.set_pyramid_filter(BINOMIAL3)
    for k in range(2):
        tg, td = torch.from_numpy(gray[k]).cuda(), torch.from_numpy(depth[k].view(np.int16)).cuda()
        torch.cuda.synchronize()
        bt.push_raw_device(tg.data_ptr(), 1, td.data_ptr())
        want = fref.build_raw(w, h, 5, 1, gray[k], depth[k])
        for q in range(ts.N_SEQ):
            for l in range(5):
                gq, dq = bt.frame(q, l)
                assert np.array_equal(_bits(gq), _bits(want["gray"][l][q])) and np.array_equal(_bits(dq), _bits(want["depth"][l][q])), (k, q, l)
        torch.cuda.synchronize()
    assert np.abs(bt.last_poses()[0]).max() > 0
    bt.close()


# ------------------------------------------------------------------------------------------------------------------ lockstep
def _oframe(m):
    return fref.Frame(m[0], m[1], m[2], KH, LEVELS, CULLS)


def _lockstep_call(lg, obj, ref, where):
    """every logged iteration at the GPU's own input pose: n_valid equal, the logged update solves the oracle's normal equations on the
    replica's maps"""
    xi = np.zeros(6, F32)
    n_it = 0
    for l in range(LEVELS):
        n = int(lg["n_iter"][l])
        assert n >= 1, (where, l)
        for it in range(n):
            o = orc.optimize(obj.gray(l), ref.gray(l), ref.depth(l), ref.sigma(l), ref.K(l), xi, l, crop=False)
            assert o["n_valid"] == int(lg["n_valid"][l][it]) and o["n_valid"] > 0, (where, l, it, o["n_valid"], int(lg["n_valid"][l][it]))
            back = backward_error(o["H"], o["g"], lg["xi_update"][l][it])
            assert back <= TOL_BACKWARD, (where, l, it, "backward error %.3g" % back)
            xi = np.asarray(lg["xi_after"][l][it], F32).copy()
            n_it += 1
    return n_it


@pytest.mark.parametrize("B", [5, 17])
def test_tracking_in_lockstep_with_the_oracle_on_the_replica_maps(B):
    idx = tm.wide_idx(B)
    outs = _run(B, idx)
    seqs = range(B) if B == 5 else (0, 7, 8, 15, 16)
    n_it = 0
    plain_differs = 0
    for k in range(1, len(outs)):
        for b in seqs:
            assert outs[k]["status"][b] == TRACKED
            obj, ref = _oframe(outs[k]["maps"][b]), _oframe(outs[k - 1]["maps"][b])
            n_it += _lockstep_call(outs[k]["logs"][b], obj, ref, "push %d seq %d of %d" % (k, b, B))
            # (the same log does not fit the decimated maps: the lockstep tells the two pyramids apart)
            po = orc.OFrame(*outs[k]["maps"][b], KH, LEVELS, CULLS); pr = orc.OFrame(*outs[k - 1]["maps"][b], KH, LEVELS, CULLS)
            o = orc.optimize(po.gray(0), pr.gray(0), pr.depth(0), pr.sigma(0), pr.K(0), np.zeros(6, F32), 0, crop=False)
            plain_differs += backward_error(o["H"], o["g"], outs[k]["logs"][b]["xi_update"][0][0]) > TOL_BACKWARD
    assert n_it > 3 * 2 * len(seqs) and plain_differs > len(seqs)


# ------------------------------------------------------------------------------------------------------------------ composition
def test_robust_weights_on_the_filtered_maps():
    rob = dict(kind=dvo.ROBUST_HUBER, param=1.345, scale_mode=dvo.ROBUST_SCALE_ADAPTIVE, scale_floor=1e-3)
    cfg = tm.cfg()
    outs = _run(5, tm.wide_idx(5), rob=rob, cfg=cfg)
    depth = gn_sums.depth_for_cfg(cfg)
    n = 0
    for k in range(1, len(outs)):
        for b in range(5):
            obj, ref = _oframe(outs[k]["maps"][b]), _oframe(outs[k - 1]["maps"][b])
            last, m = rr.replay_call(outs[k]["logs"][b], rr.oracle_terms(obj, ref, False), LEVELS, rob["kind"], rob["param"], rob["scale_mode"],
                                     floor2=F32(1e-3) * F32(1e-3), tag="robust push %d seq %d" % (k, b), depth=depth)
            assert F32(outs[k]["s2"][b]).tobytes() == F32(last[1]).tobytes()
            n += m
    assert n > 3 * 10


def test_geometric_term_on_the_filtered_maps():
    geo = dict(weight=10.0, max_diff=0.1)
    cfg = tm.cfg()
    outs = _run(5, tm.wide_idx(5), geo=geo, cfg=cfg)
    n = 0
    for k in range(1, len(outs)):
        for b in range(5):
            obj, ref = _oframe(outs[k]["maps"][b]), _oframe(outs[k - 1]["maps"][b])
            ex, m = gr.replay_call(outs[k]["logs"][b], outs[k]["glogs"][b], gr.frame_pixels(obj, ref, False, gr.weight_params(cfg)), LEVELS,
                                   geo["weight"], geo["max_diff"], ppt=4, tag="geometric push %d seq %d" % (k, b))
            assert int(outs[k]["grec"][b]["n_geo"]) == ex["n_geo"] > 1000
            n += m
    assert n > 3 * 10


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_refusals():
    L = dvo.lib()
    f = C.c_int(-7)
    D = np.array([0.05, -0.02, 0.001, -0.001, 0.0], F32)
    g, d, s = tm.frames()
    bt = dvo.Batch(2, KH, SIZE[0], SIZE[1], LEVELS, CULLS, cfg=tm.cfg())
    assert L.dvo_batch_set_pyramid_filter(None, BINOMIAL3) == BAD and L.dvo_batch_pyramid_filter(None, C.byref(f)) == BAD
    assert L.dvo_batch_pyramid_filter(bt._p, None) == BAD
    for bad in (-1, 2, 7):
        assert L.dvo_batch_set_pyramid_filter(bt._p, bad) == BAD
    assert bt.pyramid_filter() == NONE
    # sensor undistortion and the filter exclude each other, in either order of the calls
    bt.set_distortion(D)
    assert L.dvo_batch_set_pyramid_filter(bt._p, BINOMIAL3) == BAD and bt.pyramid_filter() == NONE
    bt.set_pyramid_filter(NONE)                                   # (NONE is no filter: allowed)
    bt.set_distortion(None)
    bt.set_pyramid_filter(BINOMIAL3)
    with pytest.raises(dvo.DvoError):
        bt.set_distortion(D)
    assert not bt.distortion()[1] and bt.pyramid_filter() == BINOMIAL3
    bt.set_pyramid_filter(NONE); bt.set_pyramid_filter(BINOMIAL3)   # free until the first frame
    t = [tm.dev(x[:2]) for x in (g, d, s)]
    bt.push_device(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr())
    assert L.dvo_batch_set_pyramid_filter(bt._p, NONE) == BAD and bt.pyramid_filter() == BINOMIAL3     # fixed by the first push
    bt.set_pyramid_filter(BINOMIAL3)                              # (the value in force: allowed)
    bt.close()
    # ... and by the first prefetch; a plain batch cannot turn it on later
    for first in ("prefetch", "push"):
        bt = dvo.Batch(2, KH, SIZE[0], SIZE[1], LEVELS, CULLS, cfg=tm.cfg())
        if first == "prefetch":
            bt.prefetch_device(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr())
        else:
            bt.push_device(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr())
        assert L.dvo_batch_set_pyramid_filter(bt._p, BINOMIAL3) == BAD
        bt.set_pyramid_filter(NONE)
        if first == "prefetch":
            bt.push_device(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr())
        bt.synchronize()
        bt.close()
    # culls above 2, a mono handle
    bt = dvo.Batch(1, K640, 640, 480, 2, 3)
    assert L.dvo_batch_set_pyramid_filter(bt._p, BINOMIAL3) == BAD
    bt.close()
    mb = dvo.MonoBatch(2, K640, 640, 480, cfg=dvo.default_config(rng_seed=3))
    assert L.dvo_batch_set_pyramid_filter(mb._p, BINOMIAL3) == BAD and L.dvo_batch_set_pyramid_filter(mb._p, NONE) == BAD
    assert L.dvo_batch_pyramid_filter(mb._p, C.byref(f)) == BAD
    mb.close()
    # the operator
    rgb, d16 = _raw(4, 72, 88, 1, 1)
    for kw in (dict(flags=dvo.PYRAMID_ROWS_DECIMATED), dict(flags=dvo.PYRAMID_SPLIT), dict(filter=2), dict(filter=-1)):
        flags = kw.pop("flags", 0)
        src = (rgb[:, ::2], d16[:, ::2]) if flags & dvo.PYRAMID_ROWS_DECIMATED else (rgb, d16)
        with pytest.raises(dvo.DvoError):
            dvo.op_pyramid_frames_filtered(88, 72, 4, 1, kw.get("filter", BINOMIAL3), rgb=src[0], depth16=src[1], flags=flags)
    with pytest.raises(dvo.DvoError):
        dvo.op_pyramid_frames_filtered(640, 480, 2, 3, BINOMIAL3, gray=np.zeros((1, 480, 640), F32))


# ------------------------------------------------------------------------------------------------------------------ outcome
def test_filtered_batch_beats_plain_on_noisy_pairs():
    """The outcome scene of tests/pyramid_filter_ref.py (gray noise 0.04 on synth's pairs, motion 0.005 / 0.3 deg, seeds 42-49): one
    batch of eight sequences plain, one filtered.  The replica (tests/test_pyramid_filter_abi.py recomputes it) decides first: the GPU
    must win on every seed the replica wins by a factor of at least 1.25, and its summed-error ratio must be at most (R + 1) / 2."""
    o = fref.OUTCOME
    cfg = dvo.default_config(gn_pixels_per_thread=4, crop_enable=1 if o["crop"] else 0, step_default=o["steps"][0], step_level1=o["steps"][1],
                             step_level2=o["steps"][2], min_residual=o["min_residual"], min_update=o["min_update"], max_iterations=o["max_iterations"])
    pairs = [fref.outcome_pair(seed) for seed in o["seeds"]]
    B = len(pairs)
    err = {}
    for filt in (NONE, BINOMIAL3):
        bt = dvo.Batch(B, pairs[0][3], o["width"], o["height"], o["levels"], o["culls"], cfg=cfg)
        bt.set_pyramid_filter(filt)
        for k in (0, 1):
            t = [tm.dev(np.stack([p[j][k] for p in pairs])) for j in (0, 1, 2)]
            bt.push_device(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr())
            bt.synchronize()
        xi, _ = bt.last_poses()
        bt.close()
        err[filt] = np.array([fref.pose_error(xi[b], pairs[b][4]) for b in range(B)])
    wins = err[BINOMIAL3] < err[NONE]
    ratio = err[BINOMIAL3].sum() / err[NONE].sum()
    must = np.asarray(fref.REPLICA_PLAIN) >= 1.25 * np.asarray(fref.REPLICA_FILTERED)
    cap = 0.5 * (fref.REPLICA_RATIO + 1.0)
    print("\npyramid filter: plain %s\n                filtered %s\n                GPU wins %s (must %s), summed %.5f against %.5f, ratio %.4f (replica %.4f, cap %.4f)"
          % (np.round(err[NONE], 5).tolist(), np.round(err[BINOMIAL3], 5).tolist(), wins.tolist(), must.tolist(), err[BINOMIAL3].sum(),
             err[NONE].sum(), ratio, fref.REPLICA_RATIO, cap))
    assert must.sum() >= 6 and all(w or not m for w, m in zip(wins, must)) and ratio <= cap, (wins, must, ratio, cap)
