"""The keyframe maps as compacted world-frame point clouds (dvo_batch_export_points, include/dvo.h) on the GPU.

Every export is held to the contract-exact replica (tests/points_ref.py) bit for bit: offsets, src, the four floats and sigma, from what
the public readers return (the keyframe maps and twist of dvo_batch_keyframe_get, the count plane of dvo_batch_keyframe_fusion_counts,
dvo_op_se3_exp(-xi)).  Shapes: 320x240 frames, three levels; a sensor-depth batch at culls 1 has levels of 40x30, 80x60 and 160x120
(1 200, 4 800 and 19 200 pixels: 2, 5 and 19 chunks of 1 024 pixels, the last partly empty), a mono batch 20x15, 40x30 and 80x60; 326x246
gives a top level of 163x123 = 20 049 pixels, no multiple of 4 (the pixel-by-pixel tail), and 90x73 with four levels one of 45x36.
Batches of 1, 5 and 17 sequences."""
import ctypes as C
import functools

import numpy as np
import pytest

import dvo_amd as dvo
import orc
import points_ref as pref
from dvo_amd import synth
from util import K640

pytestmark = pytest.mark.gpu

SKIP, TRACK, RESTART = dvo.SEQ_SKIP, dvo.SEQ_TRACK, dvo.SEQ_RESTART
ALL, NEW = dvo.POINTS_ALL, dvo.POINTS_NEW   # (without the feature the file fails here, at import)
SIZE = (320, 240)
LEVELS, CULLS = 3, 1            # the sensor-depth batches; a mono batch is Frame(gray, K, 3, 2)
STEPS = (1.0, 0.75, 0.5)
KH = np.array(K640, np.float32).copy()
KH[0] *= 0.5
KH[1] *= 0.5
F32 = np.float32
CANARY = 64
CAN_F, CAN_I = F32(-777.25), 0x5A5A5A5A
EPS = 2.0 ** -24


def _cfg(**kw):
    kw.setdefault("max_iterations", 6)
    kw.setdefault("keyframe_min_translation", 1.0)
    kw.setdefault("keyframe_max_frames", 3)
    return dvo.default_config(gn_pixels_per_thread=4, crop_enable=0, step_default=STEPS[0], step_level1=STEPS[1], step_level2=STEPS[2],
                              min_residual=0.0, min_update=2e-5, **kw)


def _mono_cfg(**kw):
    kw.setdefault("keyframe_max_frames", 2)
    return dvo.default_config(rng_seed=3, gn_pixels_per_thread=4, **kw)


@functools.lru_cache(maxsize=None)
def _frames(size=SIZE):
    K = KH.copy()
    g, d, s, poses = synth.sequence(6, width=size[0], height_px=size[1], K=K, seed=42, sigma_value=0.5)
    return g.numpy(), d.numpy(), s.numpy(), poses


def _idx(B, k):
    return [(k + b) % 6 for b in range(B)]


def _cams(B):
    c = np.tile(KH.reshape(1, 9), (B, 1)).astype(np.float32)
    c[:, 0] *= 1.0 + 0.01 * np.arange(B); c[:, 4] *= 1.0 - 0.008 * np.arange(B)
    c[:, 2] += 0.7 * np.arange(B); c[:, 5] -= 0.4 * np.arange(B)
    return c


class Kind:
    """what differs between the two batch kinds for the replica: pyramid shape, and which maps a keyframe has"""

    def __init__(self, bt, mono, levels, culls, cams=None, K=KH, fused=False):
        self.bt, self.mono, self.levels, self.culls, self.cams, self.K, self.fused = bt, mono, levels, culls, cams, K, fused
        self.top = levels - 1

    def level_K(self, b, level):
        return pref.level_K(self.K if self.cams is None else self.cams[b], self.culls, self.levels, level)

    def seqs(self, level, select=ALL):
        """the replica's input: per sequence None (never started / deselected) or its keyframe's maps, K and Wk"""
        bt = self.bt
        key = bt.world_poses()[2]
        out = []
        for b in range(bt.n_seq):
            try:
                kf = bt.keyframe(b, level)
            except dvo.DvoError:
                out.append(None)      # the sequence has never started
                continue
            if select == NEW and not key[b]:
                out.append(None)
                continue
            s = dict(depth=kf["depth"], gray=kf["gray"], K=self.level_K(b, level), Wk=dvo.se3.exp(-kf["xi"]), xi=kf["xi"])
            if self.mono:
                s["sigma"] = kf["sigma"]
                if level == self.top:
                    s["age"] = kf["age"]
            elif self.fused and level == self.top:
                s["counts"] = bt.keyframe_fusion_counts(b)
            out.append(s)
        return out


def _export(bt, cfg=None, capacity=None, sigma=False, src=True):
    """one export into torch buffers with a canary region after each; returns numpy arrays (the written parts) and the total"""
    import torch
    B = bt.n_seq
    off = torch.full((B + 1 + CANARY,), CAN_I, dtype=torch.int32, device="cuda")
    if capacity is None:
        torch.cuda.synchronize()
        bt.export_points(cfg, 0, 0, 0, 0, off.data_ptr())
        capacity = int(bt.last_points()[-1])
    cap = int(capacity)
    xyzg = torch.full((cap + CANARY, 4), float(CAN_F), dtype=torch.float32, device="cuda")
    srct = torch.full((cap + CANARY,), CAN_I, dtype=torch.int32, device="cuda")
    sig = torch.full((cap + CANARY,), float(CAN_F), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    bt.export_points(cfg, cap, xyzg.data_ptr() if cap else 0, srct.data_ptr() if (src and cap) else 0, sig.data_ptr() if (sigma and cap) else 0,
                     off.data_ptr())
    bt.synchronize()
    o = off.cpu().numpy().view(np.uint32)
    total = int(o[B])
    n = min(total, cap)
    x = xyzg.cpu().numpy(); si = srct.cpu().numpy().view(np.uint32); sg = sig.cpu().numpy()
    # nothing at or past the capacity (and nothing past the written points) is touched
    assert (o[B + 1:] == CAN_I).all()
    assert (x[n:] == CAN_F).all() and (si[n:] == CAN_I).all() and (sg[n:] == CAN_F).all()
    if not src:
        assert (si == CAN_I).all()
    if not sigma:
        assert (sg == CAN_F).all()
    assert bt.last_points().tobytes() == o[:B + 1].tobytes()
    return dict(off=o[:B + 1].copy(), xyzg=x[:n].copy(), src=si[:n].copy() if src else None, sigma=sg[:n].copy() if sigma else None, total=total)


def _same(got, want, what, n=None):
    off, xyzg, src, sg = want
    assert got["off"].tobytes() == off.tobytes(), (what, got["off"], off)
    n = len(src) if n is None else n
    assert got["xyzg"].tobytes() == xyzg[:n].tobytes(), (what, "xyzg")
    if got["src"] is not None:
        assert got["src"].tobytes() == src[:n].tobytes(), (what, "src")
    if got["sigma"] is not None:
        assert got["sigma"].tobytes() == sg[:n].tobytes(), (what, "sigma")


def _check(kind, what, level, stride=1, select=ALL, **gates):
    """one export against the replica; returns the replica's total"""
    bt = kind.bt
    cfg = dvo.points_config(level=level, stride=stride, select=select, **gates)
    gates.setdefault("min_depth", dvo.default_config().min_depth)      # (the default configuration: the handle's)
    want = pref.export(kind.seqs(level, select), want_sigma=kind.mono, stride=stride, **gates)
    got = _export(bt, cfg, sigma=kind.mono)
    _same(got, want, (what, "level", level, "stride", stride, "select", select, gates))
    return int(want[0][-1])


# ---- sensor-depth keyframe batches ----------------------------------------------------------------------------------------------
def _sensor(B, size=SIZE, levels=LEVELS, culls=CULLS, cams=None, fusion=False, cfg_kw=None):
    bt = dvo.Batch(B, KH, size[0], size[1], levels, culls, cfg=_cfg(**(cfg_kw or {})))
    bt.set_keyframe_tracking(True)
    if fusion:
        bt.set_keyframe_fusion(dvo.KF_FUSION_ON, 0.05, 16)
    if cams is not None:
        bt.set_intrinsics(cams)
    return bt


def _push(bt, k, size=SIZE, depth_edit=None):
    g, d, s, _ = _frames(size)
    sel = _idx(bt.n_seq, k)
    dd = d[sel].copy()
    if depth_edit is not None:
        depth_edit(dd)
    bt.push_host(g[sel], dd, s[sel])


SENSOR_CASES = [("b1", dict(B=1)), ("b5", dict(B=5)), ("b17", dict(B=17)), ("b5_fused", dict(B=5, fusion=True)),
                ("b5_cameras", dict(B=5, cams=True)), ("b17_cameras_fused", dict(B=17, cams=True, fusion=True))]


@pytest.mark.parametrize("name,kw", SENSOR_CASES, ids=[c[0] for c in SENSOR_CASES])
def test_sensor_bit_for_bit(name, kw):
    """Six pushes (keyframes live for three frames: pushes 1 and 2 track and, with fusion, fuse, push 3 promotes, 4 and 5 fuse again):
    after every push the top level of every sequence, after the last every level x stride x selection, with fusion also min_count = 2."""
    B, fusion = kw["B"], kw.get("fusion", False)
    cams = _cams(B) if kw.get("cams") else None
    bt = _sensor(B, cams=cams, fusion=fusion)
    try:
        kind = Kind(bt, False, LEVELS, CULLS, cams, fused=fusion)
        promoted = 0
        for k in range(6):
            _push(bt, k)
            total = _check(kind, "push %d" % k, LEVELS - 1)
            assert total > B * 160 * 120 // 2
            if fusion and k in (1, 2):   # the fusing pushes: counts of k where a pixel fused every time
                t2 = _check(kind, "push %d min_count" % k, LEVELS - 1, min_count=k)
                assert 0 < t2 < total
            promoted += int(bt.world_poses()[2].sum()) if k else 0
        assert promoted >= B        # a keyframe other than the first, in every sequence
        for level in (0, LEVELS - 1):
            for stride in (1, 2, 3):
                for select in (ALL, NEW):
                    _check(kind, "last", level, stride, select)
        if fusion:
            for mc in (0, 2):
                _check(kind, "last min_count", LEVELS - 1, min_count=mc)
        _check(kind, "last max_depth", LEVELS - 1, max_depth=1.5)
    finally:
        bt.close()


# ---- mono batches -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _init_depth():
    d0 = orc.cull_image(_frames()[1][0], 2)
    return (d0 + np.random.RandomState(12).normal(0, 0.05, d0.shape)).astype(np.float32)


def _mono(B, cams=None, init=None, cfg_kw=None):
    K = KH if cams is None else cams.reshape(B, 3, 3)
    mb = dvo.MonoBatch(B, K, SIZE[0], SIZE[1], cfg=_mono_cfg(**(cfg_kw or {})), per_sequence_K=cams is not None)
    d = _init_depth() if init is None else init
    mb.setInitialDepth(d, np.full_like(d, 0.5))
    return mb


def _call(mb, k):
    g = _frames()[0]
    mb.odometrize_host(np.ascontiguousarray(g[_idx(mb.n_seq, k)]))


MONO_CASES = [("b1", dict(B=1)), ("b5", dict(B=5)), ("b17", dict(B=17)), ("b5_cameras", dict(B=5, cams=True))]


@pytest.mark.parametrize("name,kw", MONO_CASES, ids=[c[0] for c in MONO_CASES])
def test_mono_bit_for_bit(name, kw):
    """Four calls with keyframes every two frames: a second keyframe exists; every level x stride x selection after the last call."""
    B = kw["B"]
    cams = _cams(B) if kw.get("cams") else None
    mb = _mono(B, cams)
    try:
        kind = Kind(mb, True, 3, 2, cams)
        for k in range(4):
            _call(mb, k)
            _check(kind, "call %d" % k, 2)
        assert min(mb.keyframe(b)["n_keyframes"] for b in range(B)) >= 2
        for level in (0, 2):
            for stride in (1, 2, 3):
                for select in (ALL, NEW):
                    _check(kind, "last", level, stride, select)
    finally:
        mb.close()


def _threshold(values, upper):
    """a value of `values` such that between a tenth and nine tenths of them pass `v <= t` (upper) or `v >= t`; the one nearest a half"""
    v = np.sort(np.asarray(values, np.float64))
    best = None
    for t in np.unique(v):
        frac = (v <= t).mean() if upper else (v >= t).mean()
        if 0.1 <= frac <= 0.9 and (best is None or abs(frac - 0.5) < abs(best[1] - 0.5)):
            best = (float(t), float(frac))
    return best


def test_mono_sigma_and_age_gates_remove_a_real_share():
    """max_sigma and min_age chosen from the replica's maps so that between a tenth and nine tenths of the candidates survive.  Sequences
    1 and 2 restart at the fourth call: their keyframes are young (age 0) when the others' pixels have been propagated twice."""
    B = 5
    mb = _mono(B)
    try:
        kind = Kind(mb, True, 3, 2)
        for k in range(5):
            if k == 3:
                a = np.full(B, TRACK, np.uint8)
                a[1:3] = RESTART
                mb.set_actions(a)
            _call(mb, k)
        seqs = kind.seqs(2)
        md = dvo.default_config().min_depth
        cand = [pref.gates(s["depth"], min_depth=md) for s in seqs]
        n_cand = sum(int(c.sum()) for c in cand)
        ts = _threshold(np.concatenate([s["sigma"][c] for s, c in zip(seqs, cand)]), True)
        ta = _threshold(np.concatenate([s["age"][c] for s, c in zip(seqs, cand)]), False)
        assert ts is not None and ta is not None, (ts, ta)
        n_s = _check(kind, "sigma gate", 2, max_sigma=ts[0])
        n_a = _check(kind, "age gate", 2, min_age=ta[0])
        n_b = _check(kind, "both gates", 2, stride=2, max_sigma=ts[0], min_age=ta[0])
        print("candidates %d, max_sigma %.6g keeps %d (%.3f), min_age %.6g keeps %d (%.3f), both at stride 2: %d"
              % (n_cand, ts[0], n_s, n_s / n_cand, ta[0], n_a, n_a / n_cand, n_b))
        assert 0.1 * n_cand <= n_s <= 0.9 * n_cand and 0.1 * n_cand <= n_a <= 0.9 * n_cand
        # the sigma gate on a coarser level reads that level's own sigma map
        s0 = kind.seqs(0)
        t0 = _threshold(np.concatenate([s["sigma"][pref.gates(s["depth"], min_depth=md)] for s in s0]), True)
        if t0 is not None:
            _check(kind, "sigma gate level 0", 0, max_sigma=t0[0])
    finally:
        mb.close()


# ---- where compaction can go wrong ----------------------------------------------------------------------------------------------
def _edit_patterns(dd):
    """depth frames [5][240][320] whose top level (the pixels (2x, 2y)) is: 0 everything valid; 1 nothing; 2 only the last pixel of chunk
    0 and the first of chunk 1; 3 only one lane's four pixels; 4 valid but for a NaN, a +inf and a below-min_depth block"""
    W = 160
    top = lambda i: ((i // W) * 2, (i % W) * 2)
    keep = dd.copy()
    dd[1] = 0.0
    dd[2] = 0.0
    for i in (pref.CHUNK - 1, pref.CHUNK):
        dd[2][top(i)] = keep[2][top(i)]
    dd[3] = 0.0
    for i in range(2 * pref.CHUNK + 4 * 37, 2 * pref.CHUNK + 4 * 37 + 4):
        dd[3][top(i)] = keep[3][top(i)]
    dd[4, 20:40, 30:60] = np.nan
    dd[4, 100:110, 200:230] = np.inf
    dd[4, 150:156, 40:80] = 0.1


def test_compaction_edges():
    bt = _sensor(5)
    try:
        _push(bt, 0, depth_edit=_edit_patterns)
        kind = Kind(bt, False, LEVELS, CULLS)
        _check(kind, "patterns top", LEVELS - 1)
        got = _export(bt, dvo.points_config())
        n = np.diff(got["off"].astype(np.int64))
        assert n[0] == 160 * 120 and n[1] == 0 and n[2] == 2 and n[3] == 4
        assert n[4] == 160 * 120 - 10 * 15 - 5 * 15 - 3 * 20
        o = got["off"]
        assert got["src"][o[2]:o[3]].tolist() == [pref.CHUNK - 1, pref.CHUNK]
        assert got["src"][o[3]:o[4]].tolist() == list(range(2 * pref.CHUNK + 148, 2 * pref.CHUNK + 152))
        for level, stride in ((0, 1), (1, 1), (2, 2), (2, 3), (1, 3)):
            _check(kind, "patterns", level, stride)
    finally:
        bt.close()


def test_nothing_valid_anywhere():
    bt = _sensor(5)
    try:
        def none(dd):
            dd[:] = 0.0
        _push(bt, 0, depth_edit=none)
        got = _export(bt, dvo.points_config(), capacity=16)
        assert (got["off"] == 0).all() and got["total"] == 0 and len(got["xyzg"]) == 0
    finally:
        bt.close()


RAGGED = [("326x246", (326, 246), 3, 1), ("90x73", (90, 73), 4, 1)]


@pytest.mark.parametrize("name,size,levels,culls", RAGGED, ids=[r[0] for r in RAGGED])
def test_ragged_planes(name, size, levels, culls):
    """Level planes that are no multiple of the chunk (nor, at 163x123, of a lane's four pixels): the last chunk of a sequence ends
    inside the plane of the next one's memory and must not read or count it."""
    bt = _sensor(5, size=size, levels=levels, culls=culls)
    try:
        kind = Kind(bt, False, levels, culls)
        for k in range(2):
            _push(bt, k, size)
        w, h = (size[0] >> culls), (size[1] >> culls)
        assert (w * h) % pref.CHUNK != 0
        total = _check(kind, name, levels - 1)
        assert total == 5 * w * h          # (noise-free renders: every pixel valid, so a pixel of the neighbour's plane would be counted)
        for level in range(levels - 1):
            _check(kind, name, level)
        _check(kind, name, levels - 1, stride=3)
    finally:
        bt.close()


# ---- capacity -----------------------------------------------------------------------------------------------------------------------
def test_capacity_truncates_and_counts_in_full():
    mb = _mono(5)
    try:
        for k in range(3):
            _call(mb, k)
        full = _export(mb, None, sigma=True)
        total = full["total"]
        assert total > 3 and len(full["xyzg"]) == total
        part = _export(mb, None, capacity=total - 3, sigma=True)      # (the canary checks are in _export)
        assert part["off"].tobytes() == full["off"].tobytes() and part["total"] == total
        assert part["xyzg"].tobytes() == full["xyzg"][:total - 3].tobytes()
        assert part["src"].tobytes() == full["src"][:total - 3].tobytes() and part["sigma"].tobytes() == full["sigma"][:total - 3].tobytes()
        count = _export(mb, None, capacity=0)
        assert count["off"].tobytes() == full["off"].tobytes() and len(count["xyzg"]) == 0
        one = _export(mb, None, capacity=1, src=False)
        assert one["xyzg"].tobytes() == full["xyzg"][:1].tobytes() and one["off"].tobytes() == full["off"].tobytes()
        big = _export(mb, None, capacity=total + 100)
        assert big["xyzg"].tobytes() == full["xyzg"].tobytes()
    finally:
        mb.close()


# ---- selection ------------------------------------------------------------------------------------------------------------------
def test_new_selects_the_keyframe_makers_and_a_skipped_sequence_has_no_points():
    B = 5
    bt = _sensor(B)
    try:
        kind = Kind(bt, False, LEVELS, CULLS)
        seen = set()
        for k in range(4):
            a = np.full(B, TRACK, np.uint8)
            a[3] = SKIP                      # skipped on every push: never starts
            if k == 2:
                a[0] = RESTART               # the only keyframe made at this push
            bt.set_actions(a)
            _push(bt, k)
            key = bt.world_poses()[2]
            assert not key[3]
            seen.add(tuple(int(v) for v in key))
            for select in (ALL, NEW):
                _check(kind, "push %d" % k, LEVELS - 1, select=select)
            got_all = _export(bt, dvo.points_config())
            got_new = _export(bt, dvo.points_config(select=NEW))
            n_all = np.diff(got_all["off"].astype(np.int64)); n_new = np.diff(got_new["off"].astype(np.int64))
            assert n_all[3] == 0 and n_new[3] == 0
            for b in range(B):
                assert n_new[b] == (n_all[b] if key[b] else 0), (k, b)
        assert len(seen) >= 3, seen          # all, none, and a mixed push
    finally:
        bt.close()


def test_restart_exports_the_new_keyframe_at_the_identity():
    B = 5
    mb = _mono(B)
    try:
        kind = Kind(mb, True, 3, 2)
        for k in range(3):
            _call(mb, k)
        assert np.abs(mb.keyframe(2)["xi"]).max() > 0
        a = np.full(B, TRACK, np.uint8)
        a[2] = RESTART
        a[4] = SKIP
        mb.set_actions(a)
        _call(mb, 3)
        kf = mb.keyframe(2)
        assert (kf["xi"] == 0).all() and kf["n_keyframes"] == 1
        _check(kind, "after restart", 2)
        _check(kind, "after restart NEW", 2, select=NEW)
        got = _export(mb, None)
        o = got["off"]
        ident = pref.export_sequence(kf["depth"], kf["gray"], kind.level_K(2, 2), np.eye(4, dtype=F32), min_depth=dvo.default_config().min_depth)
        assert got["xyzg"][o[2]:o[3]].tobytes() == ident[0].tobytes()
        assert got["xyzg"][o[2]:o[3], 2].tobytes() == kf["depth"].reshape(-1)[got["src"][o[2]:o[3]]].tobytes()   # Zw = d at the identity
    finally:
        mb.close()


# ---- determinism and non-interference ------------------------------------------------------------------------------------------
def _state(bt, mono, B, levels):
    """poses, flags and every keyframe map of a batch, as bytes"""
    out = [v.tobytes() for v in bt.world_poses()]
    if not mono:
        out += [bt.last_poses()[0].tobytes(), bt.last_status().tobytes()]
    for b in range(B):
        for l in range(levels):
            kf = bt.keyframe(b, l)
            out += [kf["gray"].tobytes(), kf["depth"].tobytes(), kf["xi"].tobytes()]
            if mono:
                out += [kf["sigma"].tobytes()] + ([kf["age"].tobytes()] if l == levels - 1 else [])
    return out


def _logs(bt, B):
    out = []
    for b in range(B):
        lg = bt.last_track_log(b)
        out.append((tuple(lg["n_iter"]),) + tuple(np.asarray(x, np.float32).tobytes() for k in ("residual", "xi_after", "upd_norm") for x in lg[k]))
    return out


@pytest.mark.parametrize("mono", [False, True], ids=["sensor", "mono"])
def test_two_calls_agree_and_exporting_changes_nothing(mono):
    B = 5
    make = (lambda: _mono(B)) if mono else (lambda: _sensor(B, fusion=True))
    step = _call if mono else _push
    a, b = make(), make()
    try:
        for k in range(4):
            step(a, k)
            step(b, k)
            e1 = _export(a, dvo.points_config(stride=2, select=NEW), sigma=mono)
            e2 = _export(a, None, sigma=mono)
            e3 = _export(a, None, sigma=mono)
            for f in ("off", "xyzg", "src") + (("sigma",) if mono else ()):
                assert e2[f].tobytes() == e3[f].tobytes(), (k, f)
            assert e1["total"] <= e2["total"]
            assert _state(a, mono, B, 3) == _state(b, mono, B, 3), k
            if k:
                assert _logs(a, B) == _logs(b, B), k
            if not mono:
                assert a.last_keyframe_fusion().tobytes() == b.last_keyframe_fusion().tobytes()
                assert [a.keyframe_fusion_counts(q).tobytes() for q in range(B)] == [b.keyframe_fusion_counts(q).tobytes() for q in range(B)]
    finally:
        a.close(); b.close()


# ---- convention -----------------------------------------------------------------------------------------------------------------
CONVENTION_RATIO_REPLICA = pref.CONVENTION["ratio"]      # the replica's right / wrong figure on the CPU


def test_convention_against_the_ground_truth_surface():
    """A sensor-depth keyframe batch on synth.sequence: after the keyframe rule has fired, the exported world points agree with
    inv(T_world_kf) X_k in float64 (T_world_kf from dvo_batch_world_poses at the promoting push) to the float32 rounding of the chain,
    and lie on the ground-truth surface -- the wrong direction, T_world_kf X_k, does not."""
    c = pref.CONVENTION
    g, d, s, poses = _frames()
    bt = dvo.Batch(1, KH, SIZE[0], SIZE[1], LEVELS, CULLS, cfg=_cfg(keyframe_max_frames=c["max_frames"], max_iterations=15))
    try:
        bt.set_keyframe_tracking(True)
        T_kf = None
        for k in range(c["pushes"]):
            bt.push_host(g[k:k + 1], d[k:k + 1], s[k:k + 1])
            _, T, key = bt.world_poses()
            if key[0]:
                T_kf, k_kf = T[0].astype(np.float64), k
        assert k_kf == c["keyframe"], k_kf
        kind = Kind(bt, False, LEVELS, CULLS)
        kf = bt.keyframe(0, LEVELS - 1)
        np.testing.assert_allclose(dvo.se3.exp(kf["xi"]).astype(np.float64), T_kf, rtol=0, atol=1e-6)   # T_world of that push = exp(ref_xi)
        got = _export(bt, None)
        fig = pref.convention_figures(kf["depth"], kind.level_K(0, LEVELS - 1), T_kf, got["src"], got["xyzg"][:, :3])
        # |exported - float64 reference| <= 16 * 2^-24 * (|X_k| + |Y_k| + |Z_k| + |t|_1) per point: three roundings in back_project,
        # one per rotation entry, one for the translation, three fmafs per row, and inv(float T) against float(exp(-xi))
        assert fig["chain_worst_ratio"] <= 1.0, fig
        print("convention: median surface distance exported %.3e, float64 reference %.3e, replica float32 %.3e, wrong direction %.3e; "
              "ratio %.3e (replica on the CPU, ground-truth pose: %.3e); chain error / bound %.3f"
              % (fig["exported"], fig["reference"], fig["replica32"], fig["wrong"], fig["exported"] / fig["wrong"],
                 CONVENTION_RATIO_REPLICA, fig["chain_worst_ratio"]))
        margin = 2.0 * abs(fig["replica32"] - fig["reference"]) + 16 * EPS * 4.0
        assert abs(fig["exported"] - fig["reference"]) <= margin, (fig, margin)
        assert fig["exported"] / fig["wrong"] <= 0.5 * (CONVENTION_RATIO_REPLICA + 1.0), fig
    finally:
        bt.close()


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals():
    import torch
    L = dvo.lib()
    B = 5
    off = torch.zeros(B + 1, dtype=torch.int32, device="cuda")
    buf = torch.zeros(64, 4, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    offp, bufp = C.c_void_p(off.data_ptr()), C.c_void_p(buf.data_ptr())
    call = lambda h, c, cap=0, xyzg=None, src=None, sg=None, o=offp: L.dvo_batch_export_points(h, C.byref(c), C.c_uint32(cap), xyzg, src, sg, o)
    host = (C.c_uint32 * (B + 1))()
    plain = dvo.Batch(B, KH, SIZE[0], SIZE[1], LEVELS, CULLS, cfg=_cfg())
    bt = _sensor(B)
    mb = _mono(B)
    try:
        ok = dvo.points_config()
        _push(plain, 0)
        assert call(plain._p, ok) == dvo.DVO_ERR_BAD_ARGUMENT                      # a plain sensor-depth batch, as dvo_batch_world_poses
        assert L.dvo_batch_last_points(plain._p, host) == dvo.DVO_ERR_BAD_ARGUMENT
        for h in (bt, mb):
            assert call(h._p, ok) == dvo.DVO_ERR_NOT_READY                          # before the first push / call
            assert L.dvo_batch_last_points(h._p, host) == dvo.DVO_ERR_NOT_READY
        _push(bt, 0)
        _call(mb, 0)
        for h in (bt, mb):
            assert L.dvo_batch_last_points(h._p, host) == dvo.DVO_ERR_NOT_READY     # no export yet
            assert L.dvo_batch_export_points(h._p, None, 0, None, None, None, offp) == dvo.DVO_ERR_BAD_ARGUMENT
            assert call(h._p, ok, o=None) == dvo.DVO_ERR_BAD_ARGUMENT
            bad = [dict(struct_size=32), dict(struct_size=0), dict(select=2), dict(select=-1), dict(level=3), dict(level=-2), dict(stride=0),
                   dict(stride=-1), dict(min_depth=float("nan")), dict(min_depth=float("inf")), dict(min_depth=1.0, max_depth=0.5),
                   dict(max_depth=float("nan")), dict(max_sigma=float("nan")), dict(min_age=-1.0), dict(min_age=float("inf")),
                   dict(min_age=float("nan")), dict(min_count=-1), dict(min_count=256), dict(min_count=1)]
            for kw in bad:
                assert call(h._p, dvo.points_config(**kw)) == dvo.DVO_ERR_BAD_ARGUMENT, (h is mb, kw)
            assert call(h._p, ok, 16, None) == dvo.DVO_ERR_BAD_ARGUMENT             # capacity > 0 needs xyzg
            assert call(h._p, ok, 16, C.c_void_p(buf.data_ptr() + 4)) == dvo.DVO_ERR_BAD_ARGUMENT   # ... 16-byte aligned
            assert call(h._p, ok, 0x80000000, bufp) == dvo.DVO_ERR_BAD_ARGUMENT
            assert L.dvo_batch_last_points(h._p, None) == dvo.DVO_ERR_BAD_ARGUMENT
            assert L.dvo_batch_last_points(h._p, host) == dvo.DVO_ERR_NOT_READY     # the refused calls queued nothing
        # gates where they do not apply
        assert call(bt._p, dvo.points_config(max_sigma=0.3)) == dvo.DVO_ERR_BAD_ARGUMENT
        assert call(bt._p, dvo.points_config(min_age=1.0)) == dvo.DVO_ERR_BAD_ARGUMENT
        assert call(bt._p, ok, 16, bufp, None, bufp) == dvo.DVO_ERR_BAD_ARGUMENT    # sigma_dev on a sensor-depth batch
        assert call(mb._p, dvo.points_config(min_age=1.0, level=1)) == dvo.DVO_ERR_BAD_ARGUMENT
        assert call(mb._p, dvo.points_config(min_age=1.0)) == dvo.DVO_OK
        assert call(mb._p, dvo.points_config(max_sigma=0.3, level=0)) == dvo.DVO_OK
        assert call(bt._p, ok) == dvo.DVO_OK
        bt.synchronize(); mb.synchronize()
        assert L.dvo_batch_last_points(bt._p, host) == dvo.DVO_OK and host[B] == B * 160 * 120
        # a fused batch: min_count on the top level only
        bt.set_keyframe_fusion()
        assert call(bt._p, dvo.points_config(min_count=1)) == dvo.DVO_ERR_BAD_ARGUMENT   # no push has fused yet
        _push(bt, 1)
        assert call(bt._p, dvo.points_config(min_count=1)) == dvo.DVO_OK
        assert call(bt._p, dvo.points_config(min_count=1, level=1)) == dvo.DVO_ERR_BAD_ARGUMENT
        # per-sequence intrinsics changed since the last push: the keyframes belong to that push's cameras
        bt.set_intrinsics(_cams(B))
        assert call(bt._p, ok) == dvo.DVO_ERR_NOT_READY
        _push(bt, 2)
        assert call(bt._p, ok) == dvo.DVO_OK
        bt.synchronize()
    finally:
        plain.close(); bt.close(); mb.close()
