"""What the GPU tests of a sensor-depth batch's opt-in tracking terms share (test_gpu_robust, test_gpu_robust_median, test_gpu_affine,
test_gpu_geometric, test_gpu_geometric_affine, test_gpu_step_control, and the files that combine them): the fixture, one batch driver,
one bit-for-bit comparison of two runs and one walker over the pushes of a run.  tests/term_replay.py is the reference-side half.

The fixture: 320x240 frames (328x248 for a raster finest level), 3 levels, culls 1, crop off, 4 pixels per thread, the converging step
constants of bench.py.  run() owns the order of the calls a batch sees; FAMILIES names the side records a push can leave, how they are
read and how they compare; same() compares two runs; walk() follows which push holds each sequence's reference.  What a term sets
(setup), what frames it is given (maps) and what a TRACKED sequence must satisfy (check) stay in the term's module.
Test infrastructure only."""
import collections
import contextlib
import functools

import numpy as np

import dvo_amd as dvo
import gn_sums
import orc
from util import K640

F32 = np.float32
SKIP, TRACK, RESTART = dvo.SEQ_SKIP, dvo.SEQ_TRACK, dvo.SEQ_RESTART
TRACKED, SKIPPED, STARTED, BAD = dvo.SEQ_TRACKED, dvo.SEQ_SKIPPED, dvo.SEQ_STARTED, dvo.SEQ_BAD_ACTION
HUBER, STUDENT = dvo.ROBUST_HUBER, dvo.ROBUST_STUDENT_T
SIZE = (320, 240)
LEVELS, CULLS, TOP = 3, 1, 2
STEPS = (1.0, 0.75, 0.5)
MIN_UPDATE = 2e-5
FLOOR = 1e-3
KH = np.array(K640, np.float32).copy()
KH[0] *= 0.5
KH[1] *= 0.5
PARAM = {HUBER: 1.345, STUDENT: 5.0}
GEO = dict(weight=10.0, max_diff=0.1)     # the default geometric config
D_LENS = np.array([0.05, -0.02, 0.001, -0.001, 0.0], F32)
EXPO = [(1.0, 0.0), (1.2, -0.03), (0.85, 0.04), (1.1, 0.02)]   # exposure of push k; sequence b scales the gain by 1 + 0.02 b
IDX = [[0, 1, 2, 3, 4], [1, 2, 3, 4, 5], [2, 3, 4, 5, 0], [3, 2, 5, 4, 1]]
# the config keywords of a schedule variant (a name that is not here, such as host_feed, runs the default schedule)
SCHEDULE_VARIANTS = dict(adaptive_off=dict(track_adaptive=-1), fused_tiles=dict(track_fused_tiles=8), single_launch=dict(track_single_launch=1),
                         lds_patch=dict(gn_use_lds_patch=2), two_streams=dict(track_streams=2))
# the setters that make up each reachable state of a sensor-depth batch, from "everything off" 
STATES = dict(N=[], R=["robust_weights"], M=["robust_median"], A=["affine_brightness"], RA=["robust_weights", "affine_brightness"],
              G=["geometric"], GA=["geometric_affine"], L=["step_control"])


# ------------------------------------------------------------------------------------------------------------------ the fixture
@contextlib.contextmanager
def oracle_steps(step3=STEPS, min_update=MIN_UPDATE):
    """the oracle's step literals follow the config of the tests inside (they enter rw); back to the reference's afterwards"""
    orc.set_tracker_params(step3=step3, min_residual=0.0, min_update=min_update)
    try:
        yield
    finally:
        orc.set_tracker_params()


def cfg(**kw):
    kw.setdefault("max_iterations", 6)
    return dvo.default_config(gn_pixels_per_thread=4, crop_enable=0, step_default=STEPS[0], step_level1=STEPS[1], step_level2=STEPS[2],
                              min_residual=0.0, min_update=MIN_UPDATE, **kw)


def rob(kind, mode=dvo.ROBUST_SCALE_ADAPTIVE):
    return dict(kind=kind, param=PARAM[kind], scale_mode=mode, scale_floor=FLOOR)


def md(kind, floor=FLOOR):
    return dict(kind=kind, param=PARAM[kind], scale_floor=floor)


def floor2(floor=FLOOR):
    return F32(floor) * F32(floor)


@functools.lru_cache(maxsize=None)
def _frames(size, sigma):
    from dvo_amd import synth
    g, d, s, _ = synth.sequence(6, width=size[0], height_px=size[1], K=KH, seed=42, sigma_value=sigma)
    return g.numpy(), d.numpy(), s.numpy()


def frames(size=SIZE, sigma=0.5):
    """six (gray, depth, sigma) frames of one synthetic scene, rendered once per size and sigma"""
    return _frames(tuple(size), float(sigma))


def oframe(i, K=KH, size=SIZE, sigma=0.5):
    g, d, s = frames(size, sigma)
    return orc.OFrame(g[i], d[i], s[i], K, LEVELS, CULLS)


def oframe_of(m, K=KH):
    """the oracle's frame of one (gray, depth, sigma)"""
    return orc.OFrame(m[0], m[1], m[2], K, LEVELS, CULLS)


def dev(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return t


def acts(B, n, seed):
    rng = np.random.RandomState(seed)
    a = rng.choice([SKIP, TRACK, RESTART], size=(n, B), p=(0.2, 0.65, 0.15)).astype(np.uint8)
    a[0] = TRACK
    return a


def wide_idx(B, pushes=3, table=True):
    """the frame assignment of tests/test_gpu_track_quality.py: neighbouring sequences and sequences 8 apart (the same slot of the next
    solve workgroup) are on different frames at every push.  table: up to five sequences take the rows of IDX"""
    if table and B <= 5:
        return [r[:B] for r in IDX[:pushes]]
    idx = [[(k + b) % 6 for b in range(B)] for k in range(pushes)]
    for r in idx:
        assert all(r[b] != r[b + 1] for b in range(B - 1)) and all(r[b] != r[b + 8] for b in range(B - 8))
    return idx


def sequence_cams(B, K=KH):
    """a camera per sequence: sequence 0 keeps K, the others differ from it and from each other"""
    cams = np.stack([np.asarray(K, F32).reshape(3, 3)] * B).astype(F32)
    for b in range(B):
        cams[b, 0, 0] *= 1.0 + 0.01 * b; cams[b, 1, 1] *= 1.0 - 0.005 * b
    return cams


def expose(gray, k, b):
    """gray under the exposure of push k and sequence b"""
    a, o = EXPO[k % len(EXPO)]
    return (F32(a * (1.0 + 0.02 * b)) * gray + F32(o)).astype(F32)


def defect(d, kind):
    """a block of the depth map d (rows h/4 .. h/2, columns w/4 .. w/2) becomes a hole, NaN, +inf or steps back by 0.5 m; returns its size"""
    h, w = d.shape
    blk = (slice(h // 4, h // 2), slice(w // 4, w // 2))
    if kind == "step":
        d[blk] += F32(0.5)
    else:
        d[blk] = dict(hole=0.0, nan=np.nan, inf=np.inf)[kind]
    return (h // 2 - h // 4) * (w // 2 - w // 4)


def raw_of(m):
    """the u8 gray and u16 depth (1 / 5000 m) frames of one (gray, depth, sigma)"""
    return np.clip(np.rint(m[0] * 255), 0, 255).astype(np.uint8), np.clip(np.rint(m[1] * 5000), 0, 65535).astype(np.uint16)


def level_poses(lg):
    """the input pose of each level's last logged iteration"""
    out = []
    for l in range(LEVELS):
        it = int(lg["n_iter"][l]) - 1
        out.append(lg["xi_after"][l][it - 1] if it > 0 else (lg["xi_after"][l - 1][int(lg["n_iter"][l - 1]) - 1] if l > 0 else np.zeros(6, np.float32)))
    return out


def se3_log_rel(P1, P0):
    return orc.se3_log((np.linalg.inv(P1) @ P0).astype(np.float32)).astype(np.float64)


# ---- the mono batches of the term tests: tests/test_gpu_mono_lockstep.py's frames
MONO_SEED = 3
MIDX = [[0, 1, 2], [1, 2, 3], [2, 3, 4], [3, 4, 5]]


def mono_frames():
    import test_gpu_mono_lockstep as ml
    g, _ = ml.render(K640)
    return g, ml.init_depth(K640), ml


def mono_plan(mb):
    """The plan of a two-sequence mono batch with the default tile config (gn_pixels_per_thread = 0) and an opt-in term: 2 x 75 tiles
    are far below 1024, so every level (40x30, 80x60, 160x120) runs <1, 1> in launch pairs on raster tiles.  Returns the depths."""
    import lockstep
    for l, tiles in enumerate((5, 19, 75)):
        assert mb.level_plan(l) == dict(ppt=1, group=1, tiles_2d=False, tiles=tiles, schedule=dvo.PLAN_PAIRS), (l, mb.level_plan(l))
    return gn_sums.plan_depths(mb, lockstep.LEVELS)


# ------------------------------------------------------------------------------------------------------------------ the side records
def logbits(lg):
    return (tuple(int(n) for n in lg["n_iter"][:LEVELS]),) + tuple(
        tuple(np.asarray(x, np.float32).tobytes() for x in lg[f][:LEVELS]) for f in ("residual", "upd_norm", "xi_after", "xi_update")) + (
        tuple(np.asarray(x, np.int32).tobytes() for x in lg["n_valid"][:LEVELS]),)


def rlogbits(lg):
    return (tuple(int(n) for n in lg["n_iter"][:LEVELS]), lg["s2"].tobytes(), lg["median_bin"].tobytes(), lg["count"].tobytes(),
            lg["prime_bin"], lg["prime_count"])


def alogbits(al):
    return (int(al["levels"]), tuple(int(n) for n in al["n_iter"]), al["a"].tobytes(), al["b"].tobytes(), F32(al["prime_a"]).tobytes(),
            F32(al["prime_b"]).tobytes())


def glogbits(gl):
    return (int(gl["levels"]), tuple(int(n) for n in gl["n_iter"]), gl["n_geo"].tobytes(), gl["sum_sq"].tobytes())


def lmbits(lg):
    return (tuple(int(n) for n in lg["n_iter"]), lg["lambda_"].tobytes(), lg["decision"].tobytes())


def _each(read, B):
    return [read(b) for b in range(B)]


# keys: what a push of the family fills; read(bt, B) -> those keys; bits(o) -> what two runs must agree on, bit for bit
Family = collections.namedtuple("Family", "keys read bits")
FAMILIES = dict(
    robust=Family(("s2",), lambda bt, B: dict(s2=bt.last_robust_scales()), lambda o: o["s2"].tobytes()),
    median=Family(("s2", "rlogs", "hist"),
                  lambda bt, B: dict(s2=bt.last_robust_scales(), rlogs=_each(bt.last_robust_log, B), hist=np.stack(_each(bt.last_robust_histogram, B))),
                  lambda o: (o["s2"].tobytes(), o["hist"].tobytes(), [rlogbits(l) for l in o["rlogs"]])),
    affine=Family(("ab", "alogs"), lambda bt, B: dict(ab=bt.last_affine(), alogs=_each(bt.last_affine_log, B)),
                  lambda o: (o["ab"].tobytes(), [alogbits(l) for l in o["alogs"]])),
    geometric=Family(("grec", "glogs"), lambda bt, B: dict(grec=bt.last_geometric(), glogs=_each(bt.last_geometric_log, B)),
                     lambda o: (o["grec"].tobytes(), [glogbits(l) for l in o["glogs"]])),
    step=Family(("rec", "lmlogs"), lambda bt, B: dict(rec=bt.last_step_control(), lmlogs=_each(bt.last_step_control_log, B)),
                lambda o: (o["rec"].tobytes(), [lmbits(l) for l in o["lmlogs"]])),
    start=Family(("start",), lambda bt, B: dict(start=bt.last_start_poses()), lambda o: o["start"].tobytes()),
)


# ------------------------------------------------------------------------------------------------------------------ the driver
def frame_maps(idx, size=SIZE, sigma=0.5):
    """maps(k, b) of run(): the frame idx[k][b] as rendered"""
    g, d, s = frames(size, sigma)
    return lambda k, b: (g[idx[k][b]], d[idx[k][b]], s[idx[k][b]])


def push(bt, maps, feed, keep):
    """one push of maps[b] = (gray, depth, sigma) through the feed; what a device feed uploads is appended to keep"""
    gi, di, si = (np.ascontiguousarray(np.stack([m[j] for m in maps])) for j in range(3))
    if feed == "host":
        bt.push_host(gi, di, si)
    elif feed in ("raw", "raw_host"):
        g8 = np.stack([raw_of(m)[0] for m in maps]); d16 = np.stack([raw_of(m)[1] for m in maps])
        if feed == "raw_host":
            bt.push_raw_host(g8, d16)
        else:
            import torch
            tg = dev(g8); td = torch.from_numpy(d16.view(np.int16)).cuda()
            torch.cuda.synchronize()
            keep.append((tg, td))
            bt.push_raw_device(tg.data_ptr(), 1, td.data_ptr())
    else:
        assert feed == "device", feed
        t = [dev(x) for x in (gi, di, si)]
        keep.append(t)
        bt.push_device(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr())


def run(cfg, B, idx, setup=None, reads=(), maps=None, at=None, acts=None, kf=False, feed="device", cams=None, cams_at=None, D=None,
        guess=None, size=SIZE, quality=True):
    """One batch of B sequences through len(idx) pushes.  idx[k][b]: the frame of sequence b at push k; maps(k, b) -> (gray, depth,
    sigma) replaces it.  setup(bt, keep) sets the terms (device rows it uploads go to keep, which lives until the batch is closed: the
    pushes are asynchronous); at = {push: fn(bt)} is called before that push; cams_at = (push, cams): set_intrinsics before that push;
    guess[k]: the given start poses of push k; reads: the FAMILIES read after every push.
    Returns per push dict(status, q, maps, plan, <the families' keys>, xi, T, logs, world); plan = level_plan of every level once the
    terms are set (the plan the pushes ran)."""
    maps = maps or frame_maps(idx, size)
    bt = dvo.Batch(B, KH, size[0], size[1], LEVELS, CULLS, cfg=cfg)
    if kf:
        bt.set_keyframe_tracking(True)
    if quality:
        bt.set_track_quality(True)
    if cams is not None:
        bt.set_intrinsics(cams)
    if D is not None:
        bt.set_distortion(D)
    if guess is not None:
        bt.set_pose_guess_mode(dvo.GUESS_GIVEN)
    keep = []
    if setup:
        setup(bt, keep)
    plan = [bt.level_plan(l) for l in range(LEVELS)]
    outs = []
    for k in range(len(idx)):
        if at and k in at:
            at[k](bt)
        m = [maps(k, b) for b in range(B)]
        if acts is not None:
            bt.set_actions(np.asarray(acts[k], np.uint8))
        if guess is not None:
            bt.set_pose_guess(np.asarray(guess[k], np.float32))
        if cams_at is not None and cams_at[0] == k:
            bt.set_intrinsics(cams_at[1])
        push(bt, m, feed, keep)
        o = dict(status=bt.last_status(), q=bt.last_track_quality() if quality else None, maps=m, plan=plan)
        for f in reads:
            o.update(FAMILIES[f].read(bt, B))
        if k > 0 or acts is not None or kf:
            xi, T = bt.last_poses()
            o.update(xi=xi.copy(), T=T.copy(), logs=[bt.last_track_log(b) for b in range(B)])
            if kf:
                o["world"] = bt.world_poses()
        outs.append(o)
    bt.close()
    return outs


# ------------------------------------------------------------------------------------------------------------------ the comparison
def same(a, b, families=None, pushes=None):
    """Two runs, bit for bit: status, poses, track logs, world poses and quality records always; the side records of `families`
    (None: every family either run has read, which both must then have read); pushes: only those pushes."""
    assert len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        if pushes is not None and k not in pushes:
            continue
        np.testing.assert_array_equal(x["status"], y["status"], err_msg="push %d" % k)
        for key in ("xi", "world"):
            assert (key in x) == (key in y), "push %d: %s in one run only" % (k, key)
        if "xi" in x:
            assert x["xi"].tobytes() == y["xi"].tobytes() and x["T"].tobytes() == y["T"].tobytes(), "push %d poses" % k
            assert [logbits(l) for l in x["logs"]] == [logbits(l) for l in y["logs"]], "push %d logs" % k
        if "world" in x:
            assert len(x["world"]) == len(y["world"])
            for u, v in zip(x["world"], y["world"]):
                assert np.asarray(u).tobytes() == np.asarray(v).tobytes(), "push %d world" % k
        assert (x["q"] is None) == (y["q"] is None), "push %d: quality records in one run only" % k
        if x["q"] is not None:
            assert x["q"].tobytes() == y["q"].tobytes(), "push %d quality records" % k
        for name, fam in FAMILIES.items():
            if families is None:
                has = [all(key in o for key in fam.keys) for o in (x, y)]     # (robust and median share s2: a family is all of its keys)
                assert has[0] == has[1], "push %d: the %s records in one run only" % (k, name)
                if not has[0]:
                    continue
            elif name not in families:
                continue
            assert fam.bits(x) == fam.bits(y), "push %d %s records" % (k, name)


# ------------------------------------------------------------------------------------------------------------------ the walker
def walk(outs, B, check, empty, kf=False, cams=None, cams_at=None, seqs=None, min_tracked=None, iters_per_seq=3):
    """Every sequence of every push of a run.  A TRACKED sequence (of seqs; None: all) goes to check(k, b, kr, o, K) -> the number of
    iterations it replayed, with kr the push that holds its reference -- the last push that started it or tracked it, with keyframe
    tracking (kf) the last that started it or promoted it -- and K its camera in force; of any other status, empty(o, b) must hold.
    At least min_tracked sequences (None: every sequence of seqs at every push but the first) and more than iters_per_seq iterations
    per sequence must have been checked.  Returns (sequences, iterations)."""
    ref_of = [None] * B
    n = n_it = 0
    for k, o in enumerate(outs):
        Ks = cams_at[1] if cams_at is not None and k >= cams_at[0] else cams
        for b in range(B):
            st = o["status"][b]
            if st == TRACKED and (seqs is None or b in seqs):
                n_it += check(k, b, ref_of[b], o, Ks[b] if Ks is not None else KH)
                n += 1
            elif st != TRACKED:
                assert empty(o, b), (k, b, st)   # SKIPPED / STARTED / BAD_ACTION: zero records and empty logs
            if kf:
                if st == STARTED or (st == TRACKED and o["world"][2][b]):
                    ref_of[b] = k
            elif st in (TRACKED, STARTED):
                ref_of[b] = k
    want = min_tracked if min_tracked is not None else (len(outs) - 1) * (B if seqs is None else len(seqs))
    assert n >= want and n_it > iters_per_seq * n, (n, n_it, want)
    return n, n_it
