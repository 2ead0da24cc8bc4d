"""Batches above 1024 sequences: the paths that change shape only there -- list slots shared between sequences
(k_propagate_*, k_promote<1|4>: the `cursor += n_slots` rounds), more than one sequence per thread of k_points_scan, a sequence index
that crosses into blockIdx.z, and the per-sequence control of the tracker above 1024 -- at the smallest images at which the pipeline
still does real work.

Method (tests/big_batch.py): sequence q of the big batch is fed what base sequence base[q] of an M-sequence batch is fed (frames
gathered on the device from the M base renders; base from a fixed-seed permutation with different bases on both sides of 1024, 2048 and
32 768), so it must return base[q]'s bits.  The chain to an independent reference is closed in this file: the M-sequence batch is held
to the CPU oracle / numpy replicas, a sample of the big batch (0, 1023, 1024, 1025, 2047, 2048, B - 1, a replica of every base from the
index ranges of the list's second and third round, ...) is held to the same reference directly, and all B sequences are compared with
their base bit for bit.  gn_pixels_per_thread is pinned to 4: the automatic tile size depends on n_seq and sets the summation order.

Every path above 1024 is shown by an assertion on observed counts: the number of keyframe-creating sequences of every call (from the
returned flags), list_rounds(), scan_per() and grid_z() of the sizes that ran."""
import functools
import time

import numpy as np
import pytest

import big_batch as bb
import dvo_amd as dvo
import lockstep
import orc
import points_ref as pref
import test_gpu_mono_lockstep as tl
from lockstep import GpuFrame, Replay

pytestmark = pytest.mark.gpu

SKIP, TRACK, RESTART = dvo.SEQ_SKIP, dvo.SEQ_TRACK, dvo.SEQ_RESTART
MONO_SIZE = (192, 144)       # top map 48 x 36 over 24 x 18 and 12 x 9: every level a multiple of 4 pixels (k_promote<4>)
MONO_RAGGED = (200, 152)     # 50 x 38 over 25 x 19 and 12 x 9: k_promote<1>
CAMS = [tl.K640, tl.K_ANISO, tl.K_OFFCENTRE, tl.K_SKEW]
ROWS = 1 << 24                # rows of one piece of an export comparison
HANDLE_BYTES = {}            # {(kind, n_seq): device memory the handle holds after its first call / push}, for the report of the grid-z tests


def _dev(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return t


def _used():
    """device memory in use that is not torch's own (the handles allocate through HIP directly)"""
    import torch
    free, total = torch.cuda.mem_get_info()
    return total - free - torch.cuda.memory_reserved()


def _bits(t):
    import torch
    return t.contiguous().view(torch.int32)


# ---- the points export as the bulk readout of the keyframe maps --------------------------------------------------------------------
def _export(h, level, sigma, capacity=None, select=dvo.POINTS_ALL, min_depth=0.0):
    """(xyzg, src, sigma or None, offsets int64 [n_seq + 1]) on the device: stride 1, every gate open"""
    cfg = dvo.points_config(level=level, stride=1, select=select, min_depth=min_depth)
    xyzg, src, sig, off = h.export_points_torch(cfg, capacity=capacity, want_src=True, want_sigma=sigma)
    return xyzg, src, sig, off.long()


def _assert_export_replicated(big, small, base_t, what, capacity=None):
    """all B + 1 offsets are the running sum of the bases' counts and every sequence's rows are its base's rows, bit for bit"""
    import torch
    off_s = small[3]
    cnt = (off_s[1:] - off_s[:-1])[base_t]
    want_off = torch.cat([torch.zeros(1, dtype=torch.int64, device=cnt.device), torch.cumsum(cnt, 0)])
    assert torch.equal(big[3], want_off), (what, "offsets")
    total = int(want_off[-1])
    idx = torch.repeat_interleave(off_s[:-1][base_t] - want_off[:-1], cnt) + torch.arange(total, device=cnt.device)
    n = total if capacity is None else min(total, capacity)
    assert len(big[0]) == n, (what, len(big[0]), n)
    xs, xb = _bits(small[0]), _bits(big[0])
    for r0 in range(0, n, ROWS):          # (in pieces: one gather of every row of the 32 808-sequence exports would be a 2.5 GB tensor)
        ix = idx[r0:min(n, r0 + ROWS)]
        r1 = r0 + len(ix)
        assert torch.equal(xb[r0:r1], xs[ix]), (what, "xyzg", r0)
        assert torch.equal(big[1][r0:r1], small[1][ix]), (what, "src", r0)
        if big[2] is not None:
            assert torch.equal(_bits(big[2][r0:r1]), _bits(small[2][ix])), (what, "sigma", r0)
    return total


# ---- Part 1 and Part 4: mono batches ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _mono_base(w, h, cams):
    """per camera: (K, frames float [6][h][w], start depth); one camera unless cams"""
    out = []
    for K0 in (CAMS if cams else [tl.K640]):
        K = tl._scaled(K0, w, h)
        out.append((K, tl.render(K, w, h)[0], tl.init_depth(K, w, h)))
    return out


class MonoCase:
    """what every sequence of a batch is fed: `cam[q]` (an index into _mono_base), `order[q][k]` (the render of call k) and, with
    actions, `act[k][q]`; built for the M bases and, through base[], for the big batch"""

    def __init__(self, w, h, cams, orders, act=None, raw=False):
        self.w, self.h, self.cams, self.raw = w, h, cams, raw
        self.basis = _mono_base(w, h, cams)
        self.orders = np.asarray(orders)                     # [M][n_calls]
        self.M, self.n_calls = self.orders.shape
        self.cam = np.arange(self.M) % len(self.basis)
        self.act = None if act is None else np.asarray(act, np.uint8)   # [n_calls][M]
        g = np.stack([b[1] for b in self.basis]).reshape(-1, h, w)     # [n_cam * 6][h][w]
        if raw:
            g = np.clip(np.rint(g * 255), 0, 255).astype(np.uint8)
        self.host_frames = g
        self.frames = _dev(g)
        self.init = _dev(np.stack([b[2] for b in self.basis]))
        self.sig = _dev(np.stack([np.full_like(b[2], tl.INIT_SIGMA) for b in self.basis]))

    def image(self, m, k):
        return int(self.cam[m]) * bb.N_RENDER + int(self.orders[m][k])


def _mono_run(case, base, watch, stats_all=True, maps_all_at=(), exports_at=(), replay=True, levels_export=(0, 1, 2)):
    """One MonoBatch over len(base) sequences, sequence q fed as base base[q] of `case`.  Returns per call a dict: xi, key, status (with
    actions), nkf / vu (keyframe and valid-update counts: of every sequence with stats_all, else of `watch`), maps {q: [level dicts]} of
    `watch` (and of every sequence at the calls in maps_all_at), export {level: device tensors} at the calls in exports_at.  With
    replay, every sequence of `watch` runs in lockstep with the oracle (lockstep.Replay); returns (records, replays)."""
    import torch
    n = len(base)
    base = np.asarray(base)
    base_t = torch.as_tensor(base, device="cuda")
    cam_t = torch.as_tensor(case.cam, device="cuda")[base_t]
    Ks = [case.basis[case.cam[m]][0] for m in range(case.M)]
    cfg = dvo.default_config(rng_seed=tl.SEED, gn_pixels_per_thread=4)
    used0 = _used()
    if case.cams:
        mb = dvo.MonoBatch(n, np.stack([Ks[m] for m in base]), case.w, case.h, ring_keyframes=case.n_calls, cfg=cfg, per_sequence_K=True)
    else:
        mb = dvo.MonoBatch(n, Ks[0], case.w, case.h, ring_keyframes=case.n_calls, cfg=cfg)
    try:
        di, ds = case.init[cam_t].contiguous(), case.sig[cam_t].contiguous()
        torch.cuda.synchronize()
        mb.setInitialDepthDevice(di.data_ptr(), ds.data_ptr())
        reps = {}
        if replay:
            for q in watch:
                m = int(base[q])
                init = case.basis[case.cam[m]][2]
                reps[q] = Replay(Ks[m], case.w, case.h, tl.SEED, init, np.full_like(init, tl.INIT_SIGMA), name="sequence %d (base %d)" % (q, m))
        out = []
        for k in range(case.n_calls):
            img = torch.as_tensor([case.image(m, k) for m in range(case.M)], device="cuda")[base_t]
            fr = case.frames[img].contiguous()
            torch.cuda.synchronize()
            if case.act is not None:
                mb.set_actions(case.act[k][base])
                mb.set_start_depth_device(di.data_ptr(), ds.data_ptr())   # (spent by every call: a restart takes the first start's map)
            if case.raw:
                mb.odometrize_raw_device(fr.data_ptr(), 1)
            else:
                mb.odometrize_device(fr.data_ptr())
            mb.synchronize()
            if k == 0:
                HANDLE_BYTES[("mono", n)] = _used() - used0
            xi, _, key = mb.world_poses()
            rec = dict(xi=xi.copy(), key=key.copy(), status=mb.last_status().copy() if case.act is not None else None)
            who = range(n) if stats_all else watch
            st = {q: mb.stats(q) for q in who} if case.act is None else {}
            rec["nkf"] = {q: s["keyframes_created"] for q, s in st.items()}
            rec["vu"] = {q: s["valid_updates_last_frame"] for q, s in st.items()}
            rec["maps"] = {}
            started = (lambda q: True) if case.act is None else (lambda q, a=case.act[:k + 1, base]: bool((a[:, q] != SKIP).any()))
            for q in (range(n) if k in maps_all_at else watch):
                if started(q):
                    rec["maps"][q] = [mb.keyframe(q, l) for l in (range(3) if q in watch or n <= 64 else (2,))]
            if replay:
                for q in watch:
                    m = int(base[q])
                    kf = rec["maps"][q]
                    host = case.host_frames[case.image(m, k)]
                    gf = GpuFrame(key[q], xi[q], None if k == 0 else mb.last_track_log(q), lambda level, kf=kf: kf[level],
                                  kf[2]["n_keyframes"], kf[2]["valid_updates"])
                    reps[q].step(lockstep.raw_gray(host) if case.raw else host, gf)
            if k in exports_at:
                rec["export"] = {l: _export(mb, l, True) for l in levels_export}
                off = rec["export"][2][3]
                assert np.array_equal(mb.last_points().astype(np.int64), off.cpu().numpy())
            out.append(rec)
        return out, reps
    finally:
        mb.close()


def _same_maps(got, want, what):
    assert len(got) == len(want) or len(got) == 1, what
    for g, w in zip(got, want if len(got) == len(want) else [want[-1]]):
        for name in ("gray", "depth", "sigma", "age", "xi"):
            if g[name] is None:
                assert w[name] is None
                continue
            assert g[name].tobytes() == w[name].tobytes(), (what, name)
        assert (g["id"], g["n_keyframes"], g["valid_updates"]) == (w["id"], w["n_keyframes"], w["valid_updates"]), what


def _compare_mono(big, small, base, case):
    """every call: poses, flags, statuses and both counts of all B sequences, the maps of every sequence read, the exports"""
    import torch
    base_t = torch.as_tensor(np.asarray(base), device="cuda")
    for k, (rb, rs) in enumerate(zip(big, small)):
        what = "call %d" % k
        assert rb["xi"].tobytes() == rs["xi"][base].tobytes(), (what, "world poses")
        assert rb["key"].tobytes() == rs["key"][base].tobytes(), (what, "keyframe flags")
        if rb["status"] is not None:
            assert rb["status"].tobytes() == rs["status"][base].tobytes(), (what, "status")
        for f in ("nkf", "vu"):
            bad = [q for q, v in rb[f].items() if v != rs[f][int(base[q])]]
            assert not bad, (what, f, bad[:8])
        for q, maps in rb["maps"].items():
            _same_maps(maps, rs["maps"][int(base[q])], "%s sequence %d (base %d)" % (what, q, base[q]))
        for l, e in rb.get("export", {}).items():
            _assert_export_replicated(e, rs["export"][l], base_t, "%s export level %d" % (what, l))


def _assert_export_is_the_replica(rec, case, level=2):
    """the M-sequence batch's export against tests/points_ref.py from the maps its readers returned"""
    seqs = []
    for m in range(case.M):
        kf = rec["maps"][m][level]
        seqs.append(dict(depth=kf["depth"], gray=kf["gray"], sigma=kf["sigma"], age=kf["age"], Wk=dvo.se3.exp(-rec["maps"][m][2]["xi"]),
                         K=pref.level_K(case.basis[case.cam[m]][0], 2, 3, level)))
    off, xyzg, src, sg = pref.export(seqs, want_sigma=True, stride=1, min_depth=0.0)
    e = rec["export"][level]
    assert np.array_equal(e[3].cpu().numpy(), off.astype(np.int64))
    assert e[0].cpu().numpy().tobytes() == xyzg.tobytes() and e[1].cpu().numpy().view(np.uint32).tobytes() == src.tobytes()
    assert e[2].cpu().numpy().tobytes() == sg.tobytes()
    return int(off[-1])


def _key_counts(recs):
    return [int(r["key"].sum()) for r in recs]


MONO_CASES = [("b1025", 1025, 8, MONO_SIZE, False), ("b2600", 2600, 10, MONO_SIZE, False), ("b2600_ragged", 2600, 10, MONO_RAGGED, False),
              ("b1025_cameras", 1025, 8, MONO_SIZE, True)]


@pytest.mark.parametrize("name,B,M,size,cams", MONO_CASES, ids=[c[0] for c in MONO_CASES])
def test_mono_batch_above_1024(name, B, M, size, cams):
    """The schedule of big_batch.mono_orders: by the keyframe rule alone the calls create 0, 1, B - 1, 1024 and 1025..2048 keyframes (at
    B = 2600 also more than 2048), then three free calls with stereo updates.  b2600_ragged: level sizes that are no multiple of 4
    (k_promote<1>); b1025_cameras: per-sequence cameras (k_propagate_owner_cam, k_depth_update_cam)."""
    t0 = time.perf_counter()
    w, h = size
    counts = bb.skewed_counts(B, M)
    base = bb.replicate(B, counts)
    orders, n_ctl = bb.mono_orders(counts)
    case = MonoCase(w, h, cams, orders)
    watch = bb.sample(base)
    assert len(watch) >= 32 and bb.rounds_covered(base, watch)[1] == {int(m) for m in np.unique(base[1024:2048])}
    assert bb.rounds_covered(base, watch)[2] == {int(m) for m in np.unique(base[2048:3072])}
    last = case.n_calls - 1
    small, reps_s = _mono_run(case, np.arange(M), list(range(M)), exports_at=range(case.n_calls))
    n_keys = bb.classes_of([r["key"] for r in small], counts)[0]
    crossed = [k + 1 for k, v in enumerate(n_keys) if v > 1024]
    big, reps_b = _mono_run(case, base, watch, maps_all_at=crossed + [last], exports_at=range(case.n_calls))
    _compare_mono(big, small, base, case)
    # the device's own flags: every class of keyframe-creating sequence counts, and with them the rounds of a list slot
    n_big = _key_counts(big)[1:]
    assert n_big == n_keys, (n_big, n_keys)
    cls = {bb.key_class(v) for v in n_big}
    want = {"0", "1..1023", "1024", "1025..2048"} | ({">2048"} if B > 2049 else set())     # (B = 2600: all of big_batch.CLASSES)
    assert want <= cls and (B < 2600 or cls == set(bb.CLASSES)), n_big
    assert max(bb.list_rounds(v, B) for v in n_big) == (3 if B > 2049 else 2)      # the strided round(s) of every listed kernel ran
    assert bb.scan_per(B) == (3 if B > 2048 else 2)                                 # k_points_scan: sequences per thread of these exports
    vec = all((w >> s) * (h >> s) % 4 == 0 for s in (2, 3, 4))
    assert vec == (size == MONO_SIZE)                                               # which k_promote instance these sizes take
    # the reference: the oracle in lockstep, for the M bases and for the sample of the big batch
    cov_s, cov_b = lockstep.total(reps_s.values()), lockstep.total(reps_b.values())
    assert cov_b["key_translation"] >= 1 and cov_b["key_count"] >= len(watch), cov_b   # (every sequence: the frame-count rule once)
    assert cov_s["updates_written"] >= 1 and cov_b["updates_written"] >= 1, (cov_s, cov_b)
    total = _assert_export_is_the_replica(small[last], case)
    assert total > M * (w >> 2) * (h >> 2) // 2
    print("%s: %.1f s; keyframe-creating sequences per call %s; sample %d; oracle coverage of the sample %s"
          % (name, time.perf_counter() - t0, n_big, len(watch), cov_b))


def test_mono_batch_above_1024_with_planned_actions():
    """TRACK / SKIP / RESTART per base and call (k_mono_decide_plan, the planned kernels) at B = 1025, against the M-sequence batch with
    the same actions: poses, flags, statuses of every sequence after every call, the maps of the sample and, after the last call, of
    every sequence."""
    t0 = time.perf_counter()
    B, M = 1025, 8
    counts = bb.skewed_counts(B, M)
    base = bb.replicate(B, counts)
    orders, _ = bb.mono_orders(counts)
    rng = np.random.RandomState(5)
    act = rng.choice([SKIP, TRACK, RESTART], size=(len(orders[0]), M), p=(0.15, 0.65, 0.2)).astype(np.uint8)
    act[0] = TRACK
    act[0, base[1023]] = SKIP                                 # a late starter on one side of 1024
    act[3, base[1024]], act[3, base[1023]] = RESTART, TRACK   # a restart on the other
    case = MonoCase(MONO_SIZE[0], MONO_SIZE[1], False, orders, act=act)
    watch = bb.sample(base)
    last = case.n_calls - 1
    small, _ = _mono_run(case, np.arange(M), list(range(M)), replay=False, exports_at=[last])
    big, _ = _mono_run(case, base, watch, replay=False, maps_all_at=[last], exports_at=[last])
    _compare_mono(big, small, base, case)
    mixed = [k for k in range(case.n_calls) if len({int(a) for a in act[k]}) == 3]
    assert len(mixed) >= 3 and any(act[k, base[1023]] != act[k, base[1024]] for k in range(case.n_calls))
    st = np.stack([r["status"] for r in big])
    assert {dvo.SEQ_TRACKED, dvo.SEQ_SKIPPED, dvo.SEQ_STARTED} <= set(np.unique(st).tolist())
    assert max(_key_counts(big)[1:]) >= 1 and int(big[last]["export"][2][3][-1]) > 0
    print("planned actions: %.1f s; keyframe flags per call %s" % (time.perf_counter() - t0, _key_counts(big)))


def test_mono_batch_across_grid_z():
    """B = 32 768 + 40, raw u8 frames: a start; a call in which only the 20 replicas of the pinned base -- all at indices above 32 768 --
    create a keyframe; one in which every other sequence does (32 788: the keyframe path at sequence indices above 32 767, 33 rounds
    of a list slot); a tracked call one render on; an export of every level."""
    t0 = time.perf_counter()
    B, M, n_pin = bb.GRID_SEQ_Y + 40, 10, 20
    pin = np.arange(bb.GRID_SEQ_Y + 1, bb.GRID_SEQ_Y + 1 + n_pin)
    counts = bb.split_even(B - n_pin, M - 1) + [n_pin]
    base = bb.replicate(B, counts, pinned={M - 1: pin})
    assert bb.grid_z(B) == 2 and bb.scan_per(B) == 33 and bb.neighbour_mix(base) > 0.8
    orders = []
    for m in range(M):
        f = m % bb.N_RENDER
        j = (f + 3) % bb.N_RENDER
        orders.append([f, j, j, (j + 1) % bb.N_RENDER] if m == M - 1 else [f, f, j, (j + 1) % bb.N_RENDER])
    case = MonoCase(MONO_SIZE[0], MONO_SIZE[1], False, orders, raw=True)
    rng = np.random.RandomState(11)
    watch = sorted(set(bb.sample(base, n=40)) | {int(q) for q in pin[:4]} | {int(q) for q in rng.choice(np.arange(bb.GRID_SEQ_Y - 64, B), 24, replace=False)})
    assert len(watch) >= 64 and sum(q < bb.GRID_SEQ_Y for q in watch) >= 16 and sum(q >= bb.GRID_SEQ_Y for q in watch) >= 16
    last = case.n_calls - 1
    small, _ = _mono_run(case, np.arange(M), list(range(M)), exports_at=[2, last])
    big, reps = _mono_run(case, base, watch, stats_all=False, exports_at=[2, last])
    _compare_mono(big, small, base, case)
    n = _key_counts(big)
    assert n[0] == B and n[1] == n_pin and n[2] == B - n_pin, n
    assert np.nonzero(big[1]["key"])[0].min() > bb.GRID_SEQ_Y                       # fewer than 1024, all from indices above 32 768
    assert big[2]["key"][bb.GRID_SEQ_Y:].sum() == 40 - n_pin and bb.list_rounds(n[2], B) == 33
    _assert_export_is_the_replica(small[last], case)
    cov = lockstep.total(reps.values())
    print("mono across grid z: %.1f s; keyframe-creating sequences per call %s; sample %d; oracle coverage of the sample %s; the handle holds %.2f GiB"
          % (time.perf_counter() - t0, n, len(watch), cov, HANDLE_BYTES[("mono", B)] / 2.0 ** 30))


# ---- Part 2 and Part 4: sensor-depth batches with keyframe tracking, fusion, carry and the points export ---------------------------------
# The replicas, configuration and schedule style are those of tests/test_gpu_kf_carry.py (kf_carry_ref on kf_fusion_ref, points_ref) at a
# quarter of its size: 160 x 120 frames, three levels at culls 1 (80 x 60 over 40 x 30 and 20 x 15); the tests assert that the base
# sequences still fuse and carry thousands of pixels there.
SENSOR_SIZE = (160, 120)
KQ = np.array(tl.K640, np.float32).copy()
KQ[0] *= 0.25
KQ[1] *= 0.25


@functools.lru_cache(maxsize=None)
def _sensor_frames():
    from dvo_amd import synth
    g, d, s, _ = synth.sequence(6, width=SENSOR_SIZE[0], height_px=SENSOR_SIZE[1], K=KQ, seed=42, sigma_value=0.5)
    return g.numpy(), d.numpy(), s.numpy()


class _View:
    """the sequences `idx` of a batch, as a batch of len(idx) sequences, for tests/test_gpu_kf_carry.py's Mirror"""

    def __init__(self, bt, idx):
        self.bt, self.idx = bt, np.asarray(idx)

    def last_status(self):
        return self.bt.last_status()[self.idx]

    def last_poses(self):
        return tuple(v[self.idx] for v in self.bt.last_poses())

    def world_poses(self):
        return tuple(v[self.idx] for v in self.bt.world_poses())

    def last_keyframe_fusion(self):
        return self.bt.last_keyframe_fusion()[self.idx]

    def last_keyframe_carry(self):
        return self.bt.last_keyframe_carry()[self.idx]

    def keyframe(self, b, level=None):
        return self.bt.keyframe(int(self.idx[b]), level)

    def keyframe_fusion_counts(self, b):
        return self.bt.keyframe_fusion_counts(int(self.idx[b]))

    def frame(self, b, level=None):
        return self.bt.frame(int(self.idx[b]), level)


def _sensor_make(n, max_frames, carry=True):
    import test_gpu_kf_carry as kc
    bt = dvo.Batch(n, KQ, SENSOR_SIZE[0], SENSOR_SIZE[1], kc.LEVELS, kc.CULLS, cfg=kc._cfg(keyframe_max_frames=max_frames))
    bt.set_keyframe_tracking(True)
    bt.set_keyframe_fusion(dvo.KF_FUSION_ON, kc.MAX_DIFF, kc.MAX_COUNT)
    if carry:
        bt.set_keyframe_carry(dvo.KF_CARRY_ON, kc.MAX_DIFF)
    return bt


def _sensor_bulk(bt):
    """what is compared for every sequence after every push"""
    xi, T = bt.last_poses()
    wx, wT, key = bt.world_poses()
    return dict(xi=xi, T=T, world_xi=wx, world_T=wT, key=key, status=bt.last_status(), fusion=bt.last_keyframe_fusion(), carry=bt.last_keyframe_carry())


def _sensor_export(h, select=dvo.POINTS_ALL, capacity=None, min_count=0):
    cfg = dvo.points_config(select=select, min_count=min_count)            # the top level, stride 1, the handle's min_depth
    xyzg, src, _, off = h.export_points_torch(cfg, capacity=capacity, want_src=True, want_sigma=False)
    return xyzg, src, None, off.long()


def _sensor_run(B, M, base, act, listed, watch, exports, max_frames=bb.SENSOR_MAX_FRAMES):
    """The M-sequence batch and the B-sequence batch side by side, push by push, with the fusion-only M-sequence batch the replica reads
    the un-carried frames from.  exports: {push: [(select, capacity or None or 'below' / 'above')]}.  Returns the two mirrors and the
    number of keyframe flags of every push of the big batch."""
    import torch
    import test_gpu_kf_carry as kc
    g, d, s = (_dev(x) for x in _sensor_frames())
    base = np.asarray(base)
    base_t = torch.as_tensor(base, device="cuda")
    small, sh = _sensor_make(M, max_frames), _sensor_make(M, max_frames, carry=False)
    used0 = _used()
    big = _sensor_make(B, max_frames)
    try:
        m_small = kc.Mirror(small, sh, M, cams=[KQ] * M)
        m_big = kc.Mirror(_View(big, watch), _View(sh, base[watch]), len(watch), cams=[KQ] * len(watch))
        keys, keep, most = [], [], dict(n_fused=0, n_carried=0)
        for k in range(len(act)):
            sel = torch.as_tensor([(k + m) % 6 for m in range(M)], device="cuda")
            for bt, ix, a in ((small, sel, act[k]), (sh, sel, act[k]), (big, sel[base_t], act[k][base])):
                t = [x[ix].contiguous() for x in (g, d, s)]
                keep.append(t)
                torch.cuda.synchronize()
                bt.set_actions(a)
                bt.push_device(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr())
            if k == 0:
                big.synchronize()
                HANDLE_BYTES[("sensor", B)] = _used() - used0
            what = "push %d" % k
            m_small.after_push(what + " (base batch)")
            m_big.after_push(what + " (sample of the big batch)")
            rs, rb = _sensor_bulk(small), _sensor_bulk(big)
            for f, v in rb.items():
                assert v.tobytes() == rs[f][base].tobytes(), (what, f)
            keys.append(int(rb["key"].sum()))
            most["n_fused"] = max(most["n_fused"], int(rs["fusion"]["n_fused"].max()))
            most["n_carried"] = max(most["n_carried"], int(rs["carry"]["n_carried"].max()))
            assert keys[-1] == listed[k], (what, keys, listed)
            for select, cap in exports.get(k, ()):
                es = _sensor_export(small, select)
                if select == dvo.POINTS_ALL and cap is None:    # the chain: the base batch's export is the replica's, from the mirror's maps
                    (off, xyzg, src), (woff, wxyzg, wsrc, _) = kc._points(small, m_small, 0, select)
                    np.testing.assert_array_equal(off, woff)
                    assert xyzg.tobytes() == wxyzg.tobytes() and src.tobytes() == wsrc.tobytes()
                    assert np.array_equal(es[3].cpu().numpy(), woff.astype(np.int64))
                total = int(((es[3][1:] - es[3][:-1])[base_t]).sum())
                c = None if cap is None else (total - 1000 if cap == "below" else total + 1000)
                got = _assert_export_replicated(_sensor_export(big, select, c), es, base_t, "%s export select %d capacity %s" % (what, select, cap), capacity=c)
                assert got == total and (c is None or c > 0)
                if select == dvo.POINTS_NEW:
                    assert int((es[3][1:] > es[3][:-1])[base_t].sum()) == listed[k]     # the sequences that just made a keyframe, and only they
            del keep[:-3]
        # the geometry is not too small: a base sequence fuses more than 1000 of its 4800 pixels in one push, and a carry moves as many
        assert most["n_fused"] > 1000 and most["n_carried"] > 1000, most
        return m_small, m_big, keys
    finally:
        small.close(); sh.close(); big.close()


@pytest.mark.parametrize("B,M", [(1025, 8), (2600, 10)], ids=["b1025", "b2600"])
def test_sensor_batch_above_1024(B, M):
    """Twelve pushes: RESTART actions set the list length of k_kf_decide -> k_promote to exactly 0, 1, 1023, 1024, 1025 (and 2049 at B =
    2600) and B, and between them the frame-count rule promotes with fusion and carry on (more than 1024 sequences at once).  After
    every push poses, flags, statuses and both records of all B sequences equal their base's; the base batch and the sample of the big
    batch are held to the numpy replicas bit for bit (keyframe depth of every level, counts, frames, records)."""
    t0 = time.perf_counter()
    counts = bb.skewed_counts(B, M)
    base = bb.replicate(B, counts)
    act, listed = bb.sensor_schedule(counts, skip=SKIP, track=TRACK, restart=RESTART)
    watch = np.asarray(bb.sample(base))
    want = {0, 1, 1023, 1024, 1025, B} | ({2049} if B >= 2600 else set())
    assert want <= set(listed), listed
    ALL, NEW = dvo.POINTS_ALL, dvo.POINTS_NEW
    one, many = listed.index(1), max(k for k in range(1, len(listed)) if listed[k] > 1024)     # (the last push with more than 1024 new keyframes)
    assert listed[one] == 1 and listed[many] > 1024
    exports = {one: [(NEW, None), (ALL, None)], many: [(NEW, None), (ALL, "below"), (ALL, "above")], len(act) - 1: [(ALL, None), (NEW, None)]}
    m_small, m_big, keys = _sensor_run(B, M, base, act, listed, watch, exports)
    assert keys == listed
    assert max(bb.list_rounds(v, B) for v in keys) == (3 if B >= 2600 else 2) and bb.scan_per(B) == (3 if B > 2048 else 2)
    for m in (m_small, m_big):      # the replicas saw fusing, clearing and carrying pushes, and the carries moved thousands of pixels
        assert m.carried >= m.B and m.fused >= m.B and m.cleared >= m.B, (m.carried, m.fused, m.cleared)
        assert min(m.fractions) > 0.25, min(m.fractions)
    print("sensor b%d: %.1f s; listed sequences per push %s; sample %d; replica: carried %d, fused %d, cleared %d, n_carried / n_candidates min %.3f"
          % (B, time.perf_counter() - t0, keys, len(watch), m_big.carried, m_big.fused, m_big.cleared, min(m_big.fractions)))


def test_sensor_batch_across_grid_z():
    """B = 32 768 + 40: a start, a push in which the pinned base (20 replicas, all above 32 768) and base 0 restart while the others fuse,
    and a push in which the frame-count rule promotes every other sequence with the carry (both sides of 32 768; 29 rounds of a list
    slot), then an export of all and of the new keyframes."""
    t0 = time.perf_counter()
    B, M, n_pin = bb.GRID_SEQ_Y + 40, 10, 20
    pin = np.arange(bb.GRID_SEQ_Y + 1, bb.GRID_SEQ_Y + 1 + n_pin)
    counts = bb.split_even(B - n_pin, M - 1) + [n_pin]
    base = bb.replicate(B, counts, pinned={M - 1: pin})
    assert bb.grid_z(B) == 2
    act = np.full((3, M), TRACK, np.uint8)
    act[1, [0, M - 1]] = RESTART
    listed = [B, counts[0] + n_pin, B - counts[0] - n_pin]
    rng = np.random.RandomState(13)
    watch = np.asarray(sorted(set(bb.sample(base, n=40)) | {int(q) for q in pin[:4]} | {int(q) for q in rng.choice(np.arange(bb.GRID_SEQ_Y - 64, B), 24, replace=False)}))
    assert len(watch) >= 64 and (watch < bb.GRID_SEQ_Y).sum() >= 16 and (watch >= bb.GRID_SEQ_Y).sum() >= 16
    m_small, m_big, keys = _sensor_run(B, M, base, act, listed, watch, {2: [(dvo.POINTS_ALL, None), (dvo.POINTS_NEW, None)]}, max_frames=2)
    assert keys == listed and bb.list_rounds(keys[2], B) == 29
    restarted = int(np.isin(base[watch], (0, M - 1)).sum())
    assert m_big.carried == len(watch) - restarted and m_big.fused == len(watch) and restarted >= 5
    side = watch[~np.isin(base[watch], (0, M - 1))]
    assert (side < bb.GRID_SEQ_Y).sum() >= 16 and (side >= bb.GRID_SEQ_Y).sum() >= 8       # a replica-checked promotion on each side
    print("sensor across grid z: %.1f s; listed sequences per push %s; sample %d; the handle holds %.2f GiB"
          % (time.perf_counter() - t0, keys, len(watch), HANDLE_BYTES[("sensor", B)] / 2.0 ** 30))


# ---- Part 3: tracking only, B = 2600, one push pair per case ---------------------------------------------------------------------------
TRACK_B, TRACK_M = 2600, 10
TRACK_PAIRS = [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (0, 2), (1, 3), (2, 5), (0, 3), (5, 0)]     # renders (reference, tracked) of every base
TRACK_LEVELS, TRACK_CULLS = 3, 1
TRACK_SIGMA = 0.05      # at this sigma the oracle's iteration totals of the ten pairs differ widely (6 to 31) at 160 x 120; at 0.5 all but one are 3


def _log_bytes(log):
    return {k: [np.asarray(x).tobytes() for x in v] if isinstance(v, (list, tuple)) else np.asarray(v).tobytes() for k, v in log.items()}


TERMS = {
    "plain": (lambda bt: None, lambda bt: {}, None),
    "huber_adaptive": (lambda bt: bt.set_robust_weights(dvo.ROBUST_HUBER, 1.345), lambda bt: dict(s2=bt.last_robust_scales()), None),
    "median": (lambda bt: bt.set_robust_median(dvo.ROBUST_HUBER, 1.345), lambda bt: dict(s2=bt.last_robust_scales()),
               lambda bt, q: dict(log=bt.last_robust_log(q), hist=dict(h=bt.last_robust_histogram(q)))),
    "affine": (lambda bt: bt.set_affine_brightness(dvo.AFFINE_ESTIMATE), lambda bt: dict(ab=bt.last_affine()),
               lambda bt, q: dict(log=bt.last_affine_log(q))),
    "geometric": (lambda bt: bt.set_geometric(dvo.GEOMETRIC_ON, 10.0, 0.1), lambda bt: dict(geo=bt.last_geometric()),
                  lambda bt, q: dict(log=bt.last_geometric_log(q))),
    "geometric_affine": (lambda bt: bt.set_geometric_affine(10.0, 0.1), lambda bt: dict(geo=bt.last_geometric(), ab=bt.last_affine()),
                         lambda bt, q: dict(geo=bt.last_geometric_log(q), affine=bt.last_affine_log(q))),
    "step_control": (lambda bt: bt.set_step_control(dvo.LM_ON), lambda bt: dict(lm=bt.last_step_control()),
                     lambda bt, q: dict(log=bt.last_step_control_log(q))),
    "track_quality": (lambda bt: bt.set_track_quality(True), lambda bt: dict(quality=bt.last_track_quality()), None),
}


def _track_pair(n, idx_ref, idx_obj, term, watch):
    """one push pair of an n-sequence batch: (poses, statuses, the term's per-sequence records, {q: track log and the term's log})"""
    import torch
    g, d, s = (_dev(x) for x in _sensor_frames())
    s = torch.full_like(s, TRACK_SIGMA)
    setup, records, term_log = TERMS[term]
    # (step control ends a level on the residual test after one accepted step with the default thresholds: as tests/test_gpu_step_control.py,
    #  it runs with min_residual 0 and a small min_update, so that the iteration counts differ between the bases)
    kw = dict(min_residual=0.0, min_update=2e-5) if term == "step_control" else {}
    bt = dvo.Batch(n, KQ, SENSOR_SIZE[0], SENSOR_SIZE[1], TRACK_LEVELS, TRACK_CULLS, cfg=dvo.default_config(gn_pixels_per_thread=4, **kw))
    try:
        setup(bt)
        for ix in (idx_ref, idx_obj):
            t = [x[ix].contiguous() for x in (g, d, s)]
            torch.cuda.synchronize()
            bt.push_device(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr())
            bt.synchronize()
        xi = bt.last_poses()[0].copy()
        rec = {k: np.array(v) for k, v in records(bt).items()}
        logs = {int(q): (bt.last_track_log(int(q)), term_log(bt, int(q)) if term_log else {}) for q in watch}
        return xi, bt.last_status().copy(), rec, logs
    finally:
        bt.close()


@pytest.mark.parametrize("term", list(TERMS), ids=list(TERMS))
def test_tracking_batch_above_1024(term):
    """The active-list compaction and solve grids (8 sequences per workgroup: 325 solve workgroups), k_plan, k_track_begin and the
    opt-in terms' *_begin kernels at 2600 sequences: all B poses, statuses and per-sequence records of the term equal the base's,
    the sample's whole per-iteration log and the term's log too; the plain case is held to orc.optimize iteration by iteration
    (tests/test_gpu_parity_scale.py part (2), its assertions and tolerances) for the M bases and for the sample of the big batch."""
    import torch
    from util import TOL_BACKWARD, assert_composed, backward_error
    t0 = time.perf_counter()
    B, M = TRACK_B, TRACK_M
    base = bb.replicate(B, bb.split_even(B, M), seed=2600)
    assert bb.neighbour_mix(base) > 0.8
    watch = bb.sample(base)
    ref_m = torch.as_tensor([p[0] for p in TRACK_PAIRS], device="cuda")
    obj_m = torch.as_tensor([p[1] for p in TRACK_PAIRS], device="cuda")
    base_t = torch.as_tensor(base, device="cuda")
    xs, ss, rs, ls = _track_pair(M, ref_m, obj_m, term, range(M))
    xb, sb, rb, lb = _track_pair(B, ref_m[base_t], obj_m[base_t], term, watch)
    assert np.isfinite(xs).all() and (ss == dvo.SEQ_TRACKED).all()
    assert xb.tobytes() == xs[base].tobytes() and sb.tobytes() == ss[base].tobytes()
    assert set(rb) == set(rs)
    for k in rb:
        assert rb[k].tobytes() == rs[k][base].tobytes(), (term, k)
    for q in watch:
        (log, tlog), (log_s, tlog_s) = lb[q], ls[int(base[q])]
        assert _log_bytes(log) == _log_bytes(log_s), (term, q)
        assert {k: _log_bytes(v) for k, v in tlog.items()} == {k: _log_bytes(v) for k, v in tlog_s.items()}, (term, q)
    iters = [sum(ls[m][0]["n_iter"][:TRACK_LEVELS]) for m in range(M)]
    assert len(set(iters)) >= 4, iters            # differing iteration counts: the active lists shrink unevenly
    n_checked = 0
    if term == "plain":
        g, d, s = _sensor_frames()
        s = np.full_like(s, TRACK_SIGMA)
        frames = {}
        for who, logs, of in (("base", ls, lambda q: q), ("big", lb, lambda q: int(base[q]))):
            for q, (lg, _) in logs.items():
                r, o_ = TRACK_PAIRS[of(q)]
                if (r, o_) not in frames:
                    frames[(r, o_)] = (orc.OFrame(g[r], d[r], s[r], KQ, TRACK_LEVELS, TRACK_CULLS), orc.OFrame(g[o_], None, None, KQ, TRACK_LEVELS, TRACK_CULLS))
                ref, obj = frames[(r, o_)]
                xi = np.zeros(6, np.float32)
                for l in range(TRACK_LEVELS):
                    for it in range(lg["n_iter"][l]):
                        o = orc.optimize(obj.gray(l), ref.gray(l), ref.depth(l), ref.sigma(l), ref.K(l), xi, l)
                        assert o["n_valid"] == lg["n_valid"][l][it], (who, q, l, it)
                        np.testing.assert_allclose(lg["residual"][l][it], o["residual"], rtol=1e-4)
                        if o["n_valid"] > 0:
                            back = backward_error(o["H"], o["g"], lg["xi_update"][l][it])
                            assert back <= TOL_BACKWARD, (who, q, l, it, back)
                        else:
                            assert not lg["xi_update"][l][it].any()
                        assert_composed(xi, lg["xi_update"][l][it], lg["xi_after"][l][it], tag=(who, q, l, it))
                        xi = lg["xi_after"][l][it]
                        n_checked += 1
        assert n_checked >= (M + len(watch)) * TRACK_LEVELS
    print("tracking %s: %.1f s; iterations per base %s; oracle-checked iterations %d" % (term, time.perf_counter() - t0, iters, n_checked))
