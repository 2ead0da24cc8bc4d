"""Every tile shape of the batch Gauss-Newton kernels, and the automatic plan.

with_gn_shape (csrc/dvo_kernels.hip) dispatches nine (pixels per thread, gather group) pairs; every pair exists with shared and with
per-sequence intrinsics (_cam), and k_track_gn_ab with and without robust weights.  Tracker::init picks the shape per level, so a
default-config batch runs a different one on each level.  Here every instance of k_track_gn_rw, k_track_gn_ab and of the plain
k_track_gn on the list-driven batch path runs against its family's reference, and the automatic plan (gn_pixels_per_thread = 0) runs
with three different shapes on three levels (B = 103) and with <1, 1> everywhere (B = 5) for the five families: plain, robust, affine,
geometric, geometric + affine.

No test assumes which shape ran: every run reads the plan in force through Batch.level_plan (dvo_debug_batch_level_plan), asserts the
shapes it claims, and takes each level's reduction depth 2 * PPT + 9 from the reported PPT.  The references, bounds and tolerances are
the families' own (tests/robust_ref.py, affine_ref.py, geometric_ref.py, geometric_affine_ref.py, gn_sums.py); nothing is fitted here.

Shapes: the instance cases are tests/test_gpu_geometric.py::test_every_kernel_instance's -- two sequences at 320x240, 3 levels, culls 1,
crop off: 40x30 and 80x60 on raster tiles, 160x120 on 2-D tiles at 4 pixels per thread and on raster tiles otherwise; one sequence is
replayed.  The plain cases run tests/test_gpu_track_quality.py's harness on three sequences at 320x240 (4 levels).  The gather group
only groups loads: the runs of one PPT must agree bit for bit across its group sizes."""
import contextlib
import functools

import numpy as np
import pytest

import dvo_amd as dvo
import gn_sums
import orc
import robust_ref as rr
import term_batch as tb
import test_gpu_affine as ta
import test_gpu_geometric as tg
import test_gpu_geometric_affine as tz
import test_gpu_robust as tr
import test_gpu_track_quality as tq
from term_batch import GEO, HUBER, KH, LEVELS, STEPS, STUDENT, TOP

pytestmark = pytest.mark.gpu

F32 = np.float32
TRACKED = dvo.SEQ_TRACKED
ESTIMATE = dvo.AFFINE_ESTIMATE
IDX2 = tb.wide_idx(2)
SHAPES = [(1, 1), (2, 1), (2, 2), (4, 1), (4, 2), (4, 4), (8, 1), (8, 2), (8, 4)]
GROUPS = {2: (1, 2), 4: (1, 2, 4), 8: (1, 2, 4)}
LEVEL_SIZES = ((40, 30), (80, 60), (160, 120))                 # 320x240, 3 levels, culls 1
PLAIN_SIZE = (320, 240)
PLAIN_LEVEL_SIZES = ((20, 15), (40, 30), (80, 60), (160, 120))  # 320x240, 4 levels, culls 1 (tests/test_gpu_track_quality.py)


@pytest.fixture(scope="module", autouse=True)
def _oracle_steps():
    with tb.oracle_steps():
        yield


@contextlib.contextmanager
def _reference_steps():
    """the plain cases run tests/test_gpu_track_quality.py's config: the reference's constants"""
    orc.set_tracker_params()
    try:
        yield
    finally:
        orc.set_tracker_params(step3=STEPS, min_residual=0.0, min_update=2e-5)


@contextlib.contextmanager
def _group(name):
    """the reduction-bound ratios recorded inside carry `name` in front (DESIGN.md §6 tabulates them per group; no digit in a name)"""
    n0 = len(gn_sums.RATIOS)
    try:
        yield
    finally:
        gn_sums.RATIOS[n0:] = [(name + ": " + t, r) for t, r in gn_sums.RATIOS[n0:]]


def _shape_cfg(ppt, group, **kw):
    cfg = tb.cfg(gn_gather_group=group, **kw)
    cfg.gn_pixels_per_thread = ppt    # (_cfg fixes 4 pixels per thread; 0: the engine chooses per level)
    return cfg


def _tiles(w, h, ppt):
    """tiles per sequence and whether they are 2-D, restated from gn_tiling (csrc/dvo_kernels.h) for a level without crop window"""
    if ppt == 4 and w % 16 == 0:
        tw = 64 if w % 64 == 0 else (32 if w % 32 == 0 else 16)
        rows = (64 // tw) * 16
        if rows * 2 <= h:
            return (w // tw) * -(-h // rows), True
    return -(-(w * h) // (256 * ppt)), False


def _assert_plan(plan, shapes, sizes=LEVEL_SIZES, schedule=dvo.PLAN_PAIRS):
    """plan (level_plan per level) runs shapes[l] = (ppt, group) on level l, on the tiles gn_tiling gives that shape, in launch pairs;
    returns the reduction depth per level"""
    assert len(plan) == len(sizes) == len(shapes)
    for l, (p, (ppt, group), (w, h)) in enumerate(zip(plan, shapes, sizes)):
        tiles, t2d = _tiles(w, h, ppt)
        want = dict(ppt=ppt, group=group, tiles_2d=t2d, tiles=tiles, schedule=p["schedule"] if schedule is None else schedule)
        assert p == want, ("level %d" % l, p, want)
    return [gn_sums.reduction_depth(p["ppt"]) for p in plan]


def _cams(B, cam, K=KH):
    """per-sequence cameras (the _cam kernels): sequence 0 keeps K, the others differ from it and from each other"""
    return tb.sequence_cams(B, K) if cam else None


# ------------------------------------------------------------------------------------------------------------------ the accessor
def test_level_plan_follows_the_plan_in_force():
    """level_plan reads Tracker::lv as use_plan() left it: the plain plan of the config, the launch-pair plan while an opt-in term is
    on, the plain plan again once it is off.  A level outside the pyramid is refused, on both batch kinds."""
    L = dvo.lib()
    bt = dvo.Batch(2, KH, 320, 240, LEVELS, 1, cfg=tb.cfg(track_fused_tiles=8))
    plain = [bt.level_plan(l) for l in range(LEVELS)]
    assert [p["schedule"] for p in plain] == [dvo.PLAN_LEVEL, dvo.PLAN_LEVEL, dvo.PLAN_ITERATION], plain   # 2, 5 and 20 tiles of two sequences
    assert [(p["ppt"], p["group"], p["tiles"], p["tiles_2d"]) for p in plain] == [(4, 2, 2, False), (4, 2, 5, False), (4, 2, 20, True)]
    bt.set_robust_weights(**tb.rob(HUBER))
    _assert_plan([bt.level_plan(l) for l in range(LEVELS)], [(4, 2)] * 3)
    bt.set_robust_weights(dvo.ROBUST_NONE)
    assert [bt.level_plan(l) for l in range(LEVELS)] == plain
    bt.set_affine_brightness(ESTIMATE)
    _assert_plan([bt.level_plan(l) for l in range(LEVELS)], [(4, 2)] * 3)
    bt.set_affine_brightness(None)
    bt.set_geometric(**GEO)
    _assert_plan([bt.level_plan(l) for l in range(LEVELS)], [(4, 2)] * 3)
    for level in (-1, LEVELS, 1000):
        assert L.dvo_debug_batch_level_plan(bt._p, level, None, None, None, None, None) == dvo.DVO_ERR_BAD_ARGUMENT, level
        with pytest.raises(dvo.DvoError):
            bt.level_plan(level)
    assert L.dvo_debug_batch_level_plan(bt._p, 0, None, None, None, None, None) == 0    # every output may be NULL
    bt.close()
    bt = dvo.Batch(2, KH, 320, 240, LEVELS, 1, cfg=tb.cfg(gn_use_lds_patch=2))
    assert all(bt.level_plan(l)["schedule"] == dvo.PLAN_LDS_PATCH and not bt.level_plan(l)["tiles_2d"] for l in range(LEVELS))
    bt.set_robust_weights(**tb.rob(HUBER))    # (no LDS patch under an opt-in term)
    _assert_plan([bt.level_plan(l) for l in range(LEVELS)], [(4, 2)] * 3)
    bt.close()
    from util import K640
    mb = dvo.MonoBatch(2, K640, 640, 480, cfg=dvo.default_config(rng_seed=3))
    assert [mb.level_plan(l)["tiles"] for l in range(3)] == [5, 19, 75] and all(mb.level_plan(l)["ppt"] == 1 for l in range(3))
    for level in (-1, 3):
        assert L.dvo_debug_batch_level_plan(mb._p, level, None, None, None, None, None) == dvo.DVO_ERR_BAD_ARGUMENT, level
    mb.close()


# ------------------------------------------------------------------------------------------------------------------ the runs
def _kind(ppt, cam):
    """Huber and Student-t alternate over (PPT, cam), so that both kinds meet every PPT; one kind per (PPT, cam), so that the gather
    groups of a PPT can be compared bit for bit"""
    return (HUBER, STUDENT)[((1, 2, 4, 8).index(ppt) + int(cam)) % 2]


@functools.lru_cache(maxsize=None)
def _robust_run(ppt, group, cam):
    return tb.run(_shape_cfg(ppt, group), 2, IDX2, cams=_cams(2, cam), **tr._weights(tb.rob(_kind(ppt, cam))))


@functools.lru_cache(maxsize=None)
def _affine_run(ppt, group, cam, rob):
    return tb.run(_shape_cfg(ppt, group), 2, IDX2, cams=_cams(2, cam), **ta._term(IDX2, dict(mode=ESTIMATE), rob=tb.rob(HUBER) if rob else None))


@functools.lru_cache(maxsize=None)
def _geometric_run(ppt, group, cam):
    return tb.run(_shape_cfg(ppt, group), 2, IDX2, cams=_cams(2, cam), **tg._term(GEO))


@functools.lru_cache(maxsize=None)
def _geometric_affine_run(ppt, group, cam):
    return tb.run(_shape_cfg(ppt, group), 2, IDX2, cams=_cams(2, cam), **tz._term(IDX2, tz._zab()))


def _plain_cfg(ppt, group):
    """the reference's constants, crop off (the 80x60 level of 320x240 frames has no rows 20 .. 100 window to speak of), sigma 0.5 (see
    test_schedule_variants_match_the_oracle) and launch pairs on every level: the list-driven k_track_gn / k_track_gn_cam"""
    return dvo.default_config(gn_pixels_per_thread=ppt, gn_gather_group=group, crop_enable=0, track_single_launch=-1)


def _plain_cams(cam):
    return _cams(3, cam, K=tq._frames_of(PLAIN_SIZE, 0.5)[3])


@functools.lru_cache(maxsize=None)
def _plain_run(ppt, group, cam):
    """three sequences through _sensor_oracle: the finest level's records inside the reduction bound of the shape's depth"""
    with _reference_steps(), _group("plain and per-camera instances"):
        return tq._sensor_oracle(_plain_cfg(ppt, group), B=3, size=PLAIN_SIZE, sigma=0.5, cams=_plain_cams(cam), depth=gn_sums.reduction_depth(ppt),
                                 tag="ppt %d group %d cam %d " % (ppt, group, cam))


# ------------------------------------------------------------------------------------------------------------------ 2: robust, affine
@pytest.mark.parametrize("cam", [False, True])
@pytest.mark.parametrize("ppt,group", SHAPES)
def test_every_robust_kernel_instance(ppt, group, cam):
    """each (PPT, G) pair of k_track_gn_rw and k_track_gn_rw_cam on a batch of two; sequence 1 is replayed"""
    outs = _robust_run(ppt, group, cam)
    depths = _assert_plan(outs[0]["plan"], [(ppt, group)] * LEVELS)
    with _group("robust instances"):
        tr._lockstep(_shape_cfg(ppt, group), 2, tb.rob(_kind(ppt, cam)), cams=_cams(2, cam), outs=outs, seqs=(1,), depth=depths)


@pytest.mark.parametrize("rob", [False, True])
@pytest.mark.parametrize("cam", [False, True])
@pytest.mark.parametrize("ppt,group", SHAPES)
def test_every_affine_kernel_instance(ppt, group, cam, rob):
    """each (PPT, G, ROB) instance of k_track_gn_ab and k_track_gn_ab_cam on a batch of two, ESTIMATE mode under the exposure changes
    of tests/test_gpu_affine.py; sequence 1 is replayed"""
    outs = _affine_run(ppt, group, cam, rob)
    depths = _assert_plan(outs[0]["plan"], [(ppt, group)] * LEVELS)
    with _group("affine instances"):
        ta._replay(_shape_cfg(ppt, group), 2, dict(mode=ESTIMATE), rob=tb.rob(HUBER) if rob else None, cams=_cams(2, cam), outs=outs, seqs=(1,),
                   depth=depths)


# ------------------------------------------------------------------------------------------------------------------ 3: plain
def _logbits4(lg):
    """every field of a four-level track log"""
    return (tuple(int(n) for n in lg["n_iter"][:4]),) + tuple(
        tuple(np.asarray(x).tobytes() for x in lg[f][:4]) for f in ("residual", "upd_norm", "xi_after", "xi_update", "n_valid"))


@pytest.mark.parametrize("cam", [False, True])
@pytest.mark.parametrize("ppt,group", SHAPES)
def test_every_plain_kernel_instance(ppt, group, cam):
    """each (PPT, G) pair of k_track_gn (cam: k_track_gn_cam, a camera per sequence) on the list-driven batch path: the records against
    the oracle, the records against the logs, and every sequence bit for bit a one-sequence batch with the same config and its camera"""
    outs = _plain_run(ppt, group, cam)
    _assert_plan(outs[0]["plan"], [(ppt, group)] * 4, sizes=PLAIN_LEVEL_SIZES)
    cfg = _plain_cfg(ppt, group)
    assert tq._check_run(outs, cfg) == 3 * (len(outs) - 1)
    idx = tq._wide_idx(3)
    cams = _plain_cams(cam)
    for b in range(3):
        one = tq._sensor_run(cfg, 1, [[r[b]] for r in idx], size=PLAIN_SIZE, sigma=0.5, K=None if cams is None else cams[b])
        _assert_plan(one[0]["plan"], [(ppt, group)] * 4, sizes=PLAIN_LEVEL_SIZES)
        for k, (x, y) in enumerate(zip(outs, one)):
            where = "push %d seq %d" % (k, b)
            assert x["status"][b] == y["status"][0], where
            assert x["q"][b].tobytes() == y["q"][0].tobytes(), where + " record"
            if k > 0:
                assert x["xi"][b].tobytes() == y["xi"][0].tobytes() and x["T"][b].tobytes() == y["T"][0].tobytes(), where + " pose"
                assert _logbits4(x["logs"][b]) == _logbits4(y["logs"][0]), where + " log"


# ------------------------------------------------------------------------------------------------------------------ 4: the automatic plan
AUTO_WIDE = dict(B=103, shapes=[(1, 1), (2, 2), (4, 2)], seqs=(3, 50, 100))   # 103 = 12 * 8 + 7: sequence 100 sits in the partly filled solve workgroup
AUTO_SMALL = dict(B=5, shapes=[(1, 1)] * 3, seqs=(1, 4))


def _plain_lockstep(outs, B, seqs, depths):
    """the plain family through robust_ref with kind NONE (rho = 1: the plain sums): every logged iteration of `seqs` at its level's
    depth, the finest level's record inside the bound"""
    idx = tb.wide_idx(B)
    before = rr.nonempty_calls()
    n = n_it = 0
    for k in range(1, len(outs)):
        o = outs[k]
        assert (o["status"] == TRACKED).all()
        for b in seqs:
            where = "push %d seq %d of %d" % (k, b, B)
            lg, q = o["logs"][b], o["q"][b]
            last, m = rr.replay_call(lg, rr.oracle_terms(tb.oframe(idx[k][b]), tb.oframe(idx[k - 1][b]), False), LEVELS, rr.NONE, 1.0, rr.ADAPTIVE,
                                     floor2=tb.floor2(), tag=where, depth=depths)
            t, _, l, it = last
            assert l == TOP and it == int(lg["n_iter"][TOP]) - 1
            assert q["status"] == TRACKED and q["n_valid"] == int(lg["n_valid"][TOP][it]), where
            assert F32(q["residual"]).tobytes() == F32(lg["residual"][TOP][it]).tobytes(), where
            rr.assert_sums(q, t, rr.NONE, 1.0, rr.INF, depths[TOP], where)
            n += 1; n_it += m
    assert n == (len(outs) - 1) * len(seqs) and n_it > 3 * n and rr.nonempty_calls() >= before + n


def _auto_case(family, case):
    """one family on the automatic plan (gn_pixels_per_thread = 0, default gather group): the plan is asserted through the accessor and
    every level of the replayed sequences is held to the depth of the shape that level ran"""
    B, shapes, seqs = case["B"], case["shapes"], case["seqs"]
    cfg = _shape_cfg(0, 0)
    assert cfg.gn_pixels_per_thread == 0
    idx = tb.wide_idx(B)
    schedule = None if family == "plain" else dvo.PLAN_PAIRS    # (a small plain batch may take one launch per iteration)
    with _group("automatic plan " + family):
        if family == "plain":
            outs = tb.run(cfg, B, idx)
            _plain_lockstep(outs, B, seqs, _assert_plan(outs[0]["plan"], shapes, schedule=schedule))
        elif family == "robust":
            outs = tb.run(cfg, B, idx, **tr._weights(tb.rob(STUDENT)))
            tr._lockstep(cfg, B, tb.rob(STUDENT), outs=outs, seqs=seqs, depth=_assert_plan(outs[0]["plan"], shapes))
        elif family == "affine":
            outs = tb.run(cfg, B, idx, **ta._term(idx, dict(mode=ESTIMATE)))
            ta._replay(cfg, B, dict(mode=ESTIMATE), outs=outs, seqs=seqs, depth=_assert_plan(outs[0]["plan"], shapes))
        elif family == "geometric":
            outs = tb.run(cfg, B, idx, **tg._term(GEO))
            _assert_plan(outs[0]["plan"], shapes)
            tg._replay(cfg, B, GEO, outs=outs, seqs=seqs, ppt=[p["ppt"] for p in outs[0]["plan"]])
        else:
            outs = tb.run(cfg, B, idx, **tz._term(idx, tz._zab()))
            _assert_plan(outs[0]["plan"], shapes)
            tz._replay(cfg, B, outs=outs, seqs=seqs, ppt=[p["ppt"] for p in outs[0]["plan"]])
    if B > 8:
        assert len({p["ppt"] for p in outs[0]["plan"]}) == 3, "three different PPTs on three levels"


FAMILIES = ["plain", "robust", "affine", "geometric", "geometric_affine"]


@pytest.mark.parametrize("family", FAMILIES)
def test_automatic_plan_mixed_shapes(family):
    """B = 103 with the default tile config: 1024 tiles are reached at PPT 1 on 40x30 (5 tiles per sequence), at PPT 2 on 80x60 (10) and
    at PPT 4 on 160x120 (20 two-dimensional): <1, 1>, <2, 2>, <4, 2> from the coarsest level to the finest, depths 11 / 13 / 17"""
    _auto_case(family, AUTO_WIDE)


@pytest.mark.parametrize("family", FAMILIES)
def test_automatic_plan_small_batch(family):
    """B = 5: every level runs <1, 1>, the other end of what the automatic plan can choose"""
    _auto_case(family, AUTO_SMALL)


# ------------------------------------------------------------------------------------------------------------------ 5: the gather group
def _same_plain(a, b):
    tq._same_poses(a, b)
    for k, (x, y) in enumerate(zip(a, b)):
        assert x["q"].tobytes() == y["q"].tobytes(), "push %d records" % k
        if "logs" in x:
            assert [_logbits4(l) for l in x["logs"]] == [_logbits4(l) for l in y["logs"]], "push %d logs" % k


GROUP_RUNS = dict(
    plain=(lambda ppt, g: [_plain_run(ppt, g, cam) for cam in (False, True)], _same_plain),
    robust=(lambda ppt, g: [_robust_run(ppt, g, cam) for cam in (False, True)], tb.same),
    affine=(lambda ppt, g: [_affine_run(ppt, g, cam, rob) for cam in (False, True) for rob in (False, True)], tb.same),
    geometric=(lambda ppt, g: [_geometric_run(ppt, g, cam) for cam in (False, True)], tb.same),
    geometric_affine=(lambda ppt, g: [_geometric_affine_run(ppt, g, cam) for cam in (False, True)], tb.same),
)


@pytest.mark.parametrize("ppt", [2, 4, 8])
@pytest.mark.parametrize("family", FAMILIES)
def test_gather_group_only_groups_loads(family, ppt):
    """gn_gather_group changes the order of loads and nothing else -- poses, track logs, quality records and the family's
    own records and logs are the same bits for every group size of a PPT (the runs of the instance tests above, shared and per-sequence
    cameras; the geometric families run here for this comparison, their instances are replayed in their own files)"""
    runs, same = GROUP_RUNS[family]
    base = runs(ppt, GROUPS[ppt][0])
    for g in GROUPS[ppt][1:]:
        other = runs(ppt, g)
        assert len(base) == len(other)
        for a, b in zip(base, other):
            assert [p["group"] for p in a[0]["plan"]] != [p["group"] for p in b[0]["plan"]]
            same(a, b)


def test_zz_report_reduction_bound_ratios():
    """last in the file: under -s, the largest error / bound ratio of every comparison of this process, per group of DESIGN.md §6"""
    gn_sums.report("test_gpu_gn_instances")
    assert all(r <= 1.0 for _, r in gn_sums.RATIOS)
