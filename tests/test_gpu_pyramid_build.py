"""Every non-remap pyramid-build kernel against tests/pyramid_ref.py, bit for bit, at ragged sizes (dvo_op_pyramid_frames).

The op builds n_seq frames through the engine's own build_pyramid -- frame_args, fuse_prep, plan_copy, pyramid_can_split and
launch_pyramid are the code under test -- always with keep_sigma = true, and returns gray, depth, sigma and wgt of every level and
sequence plus the kernel the launcher chose.  Every comparison is on uint32 views of every level, map and sequence; the reference is
exact (integer luma, single float32 products, one float32 division), so there is no tolerance.  A map the build does not write must
come back as the 0xffffffff words the op fills the frame sets with, so a missing store shows as well as a wrong one.

Every case asserts the kernel the op reports (a test that does not know which kernel ran can pass without reaching the code it
names) and that its geometry fires the `lx >= w[l]` / `ly >= h[l]` guards: ((tw - 1) >> t) >= (tw >> t) for some level t, and the same
for the height, computed here.  CASES names, between its rows, all ten non-remap instances (test_the_cases_name_every_instance).

Which kernel a ragged geometry runs depends on n_seq: FrameSet::alloc lays the levels out back to back, coarsest first, so the
top-level pointers are 16-byte aligned only when n_seq * (pixels of the lower levels) is a multiple of 4.  At 88x72, culls 1, levels
4 (20 + 99 + 396 pixels below the 44x36 top) a batch of 4 or 8 takes k_pyramid_raw4 and a batch of 3 falls back to the scalar
k_pyramid; at 144x144, levels 5, a batch of 3 can neither split nor take the vector kernel.

Left out: a sequence index that crosses into blockIdx.z.  DVO_GRID_SEQ_Y is 32768, so no small batch reaches it."""
import functools

import numpy as np
import pytest

import dvo_amd as dvo
import pyramid_ref as pref

pytestmark = pytest.mark.gpu

F32 = np.float32
ROWS, FORCE, SPLIT = dvo.PYRAMID_ROWS_DECIMATED, dvo.PYRAMID_FORCE_WEIGHT_MAPS, dvo.PYRAMID_SPLIT
S, T, R = pref.SEQ_SKIP, pref.SEQ_TRACK, pref.SEQ_RESTART
CFG = dict(step_default=2.5, step_level1=1.25, step_level2=0.75, sigma_min=0.05, sigma_max=0.4)   # not the defaults: the op passes them on

SCALAR, SCALAR_PLAN = "k_pyramid<false>", "k_pyramid<true>"
RAW4 = {(c, p): "k_pyramid_raw4<%d, %s>" % (c, "true" if p else "false") for c in (1, 2) for p in (0, 1)}
SPLIT_OF = {c: "k_pyramid_raw4_coarse<%d> + k_pyramid_raw4_rest<%d>" % (c, c) for c in (1, 2)}
INSTANCES = {SCALAR, SCALAR_PLAN} | set(RAW4.values()) | {"k_pyramid_raw4_%s<%d>" % (s, c) for s in ("coarse", "rest") for c in (1, 2)}


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _raw(n, h, w, channels, seed):
    """random u8 / u16 frames, a different pattern per sequence: about 3 % isolated d == 0 pixels and blocks of them, black pixels and
    d16 = 65535 -- on kept and on dropped rows and columns alike.  Read-only: shared between the cases."""
    shape = (n, h, w) if channels == 1 else (n, h, w, channels)
    rgb = np.zeros(shape, np.uint8)
    d16 = np.zeros((n, h, w), np.uint16)
    for q in range(n):
        rng = np.random.RandomState(1000 * seed + q)
        g = rng.randint(0, 256, shape[1:]).astype(np.uint8)
        g[rng.rand(h, w) < 0.03] = 0
        d = rng.randint(1, 65535, (h, w)).astype(np.uint16)
        d[rng.rand(h, w) < 0.03] = 0
        d[rng.rand(h, w) < 0.02] = 65535
        for _ in range(3):
            by, bx = rng.randint(0, h - 9), rng.randint(0, w - 9)
            d[by:by + rng.randint(2, 9), bx:bx + rng.randint(2, 9)] = 0
        rgb[q], d16[q] = g, d
    d16[:, 0, 0] = [0 if q % 2 else 65535 for q in range(n)]     # the one pixel every level keeps
    rgb.setflags(write=False); d16.setflags(write=False)
    return rgb, d16


@functools.lru_cache(maxsize=None)
def _float(n, h, w, seed):
    """float gray, depth and sigma with NaN (gray and depth), -7, INVALID, +-inf, and sigma on both sides of [sigma_min, sigma_max]"""
    out = []
    for m in range(3):
        a = np.zeros((n, h, w), F32)
        for q in range(n):
            rng = np.random.RandomState(1000 * seed + 10 * q + m)
            x = (rng.rand(h, w) * (1.0, 4.0, 0.7)[m] + (0.0, 0.3, 0.001)[m]).astype(F32)
            for v in ((np.nan,) if m < 2 else ()) + (-7.0, pref.INVALID, -np.inf, np.inf, 0.0):
                x[rng.rand(h, w) < 0.03] = v
            x[0, 0] = (np.nan, -7.0, 0.6)[m] if q % 2 == 0 else (-7.0, np.nan, 0.002)[m]   # pixels every level keeps
            x[4, 8] = (np.nan, 2.0, -7.0)[m]
            a[q] = x
        a.setflags(write=False)
        out.append(a)
    return tuple(out)


def _cfg(custom):
    return (dvo.default_config(**CFG), CFG) if custom else (None, None)


def _assert_maps(got, want, n, what):
    for m in pref.MAPS:
        for l, ref in enumerate(want[m]):
            g = _bits(got[m][l])
            if ref is None:
                assert (g == pref.UNWRITTEN).all(), "%s: %s level %d is not written by this build, yet %d words changed" % (what, m, l, (g != pref.UNWRITTEN).sum())
                continue
            assert g.shape == ref.shape == (n,) + ref.shape[1:]
            bad = g != _bits(ref)
            assert not bad.any(), "%s: %s level %d: %d of %d words differ, first at (seq, y, x) = %s: got %r want %r" % (
                what, m, l, bad.sum(), bad.size, tuple(np.argwhere(bad)[0]), got[m][l][tuple(np.argwhere(bad)[0])], ref[tuple(np.argwhere(bad)[0])])


def _dec(a, culls, flags):
    return a if a is None or not (flags & ROWS) else a[:, ::1 << culls]


def _run_raw(w, h, levels, culls, n, channels=1, depth=True, flags=0, custom_cfg=False, seed=1, actions=None):
    """one op call on raw frames and its reference; with actions: the planned build, a SKIP sequence's second frame being garbage"""
    rgb, d16 = _raw(n, h, w, channels, seed)
    d16 = d16 if depth else None
    cfg, cd = _cfg(custom_cfg)
    dec = bool(flags & ROWS)
    if actions is None:
        got = dvo.op_pyramid_frames(w, h, levels, culls, rgb=_dec(rgb, culls, flags), depth16=_dec(d16, culls, flags), flags=flags, cfg=cfg)
        return got, pref.build_raw(w, h, levels, culls, _dec(rgb, culls, flags), _dec(d16, culls, flags), rows_decimated=dec, cfg=cd)
    rgb2, d2 = _raw(n, h, w, channels, seed + 50)
    rgb2, d2 = rgb2.copy(), (d2.copy() if depth else None)
    for q, a in enumerate(actions):
        if a == S:
            rgb2[q] = 0xA5
            if depth:
                d2[q] = 0x5A5A
    got = dvo.op_pyramid_frames(w, h, levels, culls, rgb=_dec(rgb, culls, flags), depth16=_dec(d16, culls, flags), flags=flags, cfg=cfg,
                                seq_action=np.array(actions, np.uint8), second=dict(rgb=_dec(rgb2, culls, flags), depth16=_dec(d2, culls, flags)))
    A = pref.build_raw(w, h, levels, culls, _dec(rgb, culls, flags), _dec(d16, culls, flags), rows_decimated=dec, cfg=cd)
    B = pref.build_raw(w, h, levels, culls, _dec(rgb2, culls, flags), _dec(d2, culls, flags), rows_decimated=dec, cfg=cd)
    return got, pref.planned(A, B, actions, levels)


def _run_float(w, h, levels, culls, n, depth=True, flags=0, custom_cfg=False, seed=2, actions=None):
    g, d, s = _float(n, h, w, seed)
    if not depth:
        d = s = None
    cfg, cd = _cfg(custom_cfg)
    dec = bool(flags & ROWS)
    f = lambda a: _dec(a, culls, flags)
    if actions is None:
        got = dvo.op_pyramid_frames(w, h, levels, culls, gray=f(g), depth=f(d), sigma=f(s), flags=flags, cfg=cfg)
        return got, pref.build(w, h, levels, culls, f(g), f(d), f(s), rows_decimated=dec, cfg=cd)
    g2, d2, s2 = (a.copy() for a in _float(n, h, w, seed + 50))
    if not depth:
        d2 = s2 = None
    for q, a in enumerate(actions):
        if a == S:
            for m in (g2, d2, s2):
                if m is not None:
                    m[q] = 12345.0
    got = dvo.op_pyramid_frames(w, h, levels, culls, gray=f(g), depth=f(d), sigma=f(s), flags=flags, cfg=cfg,
                                seq_action=np.array(actions, np.uint8), second=dict(gray=f(g2), depth=f(d2), sigma=f(s2)))
    A = pref.build(w, h, levels, culls, f(g), f(d), f(s), rows_decimated=dec, cfg=cd)
    B = pref.build(w, h, levels, culls, f(g2), f(d2), f(s2), rows_decimated=dec, cfg=cd)
    return got, pref.planned(A, B, actions, levels)


def _check(case_id, kind, kw, kernel):
    kw = dict(kw)
    w, h, levels, culls, n = (kw[k] for k in ("w", "h", "levels", "culls", "n"))
    assert pref.guards_fire(w, h, levels, culls) == (True, True), "the geometry fires no guard"
    got, want = (_run_raw if kind == "raw" else _run_float)(**kw)
    assert got["kernel"].name() == kernel, "%s ran %s" % (case_id, got["kernel"].name())
    _assert_maps(got, want, n, "%s [%s]" % (case_id, kernel))
    return got, want


MIX = (S, T, R, S, T, T, R, S)
ALL_SKIP = (S,) * 8
NO_SKIP = (T, R, T, T, R, T, T, R)
G1 = dict(w=88, h=72, levels=4, culls=1)      # top 44 x 36, then 22 x 18, 11 x 9, 5 x 4: two workgroups per sequence, the second partly empty
G2 = dict(w=176, h=144, levels=4, culls=2)    # the same levels at culls 2
S1 = dict(w=144, h=144, levels=5, culls=1)    # top 72 x 72, then 36, 18, 9, 4: the smallest ragged top the split build accepts
S2 = dict(w=288, h=288, levels=5, culls=2)

CASES = {}
# the vector kernel, plain: rows decimated by the host or whole frames (src_row_shift), weight maps forced (with a config of its own)
# or not, with depth and gray only
for c, geo in ((1, G1), (2, G2)):
    for rows in (0, ROWS):
        for force in (0, FORCE):
            for depth in (True, False):
                CASES["raw4-culls%d-%s-%s-%s" % (c, "rows" if rows else "whole", "forced" if force else "plain", "depth" if depth else "gray")] = (
                    "raw", dict(geo, n=4, flags=rows | force, custom_cfg=bool(force), depth=depth), RAW4[c, 0])
# whole frames of an odd height: the last source row is dropped, the vector kernel still runs
CASES["raw4-culls1-height73"] = ("raw", dict(G1, h=73, n=4), RAW4[1, 0])
# the scalar fallback at the same shapes: three sequences (top-level pointers off 16 bytes), widths that are no multiple of 4 << culls,
# an odd height, RGB and RGBA, and float maps at culls 0 and 1
for c, geo in ((1, G1), (2, G2)):
    CASES["scalar-culls%d-three-sequences" % c] = ("raw", dict(geo, n=3, flags=ROWS), SCALAR)
    CASES["scalar-culls%d-three-sequences-gray" % c] = ("raw", dict(geo, n=3, depth=False), SCALAR)
CASES["scalar-culls1-width90-height73"] = ("raw", dict(G1, w=90, h=73, n=4), SCALAR)
CASES["scalar-culls2-width178-height147"] = ("raw", dict(G2, w=178, h=147, n=4, custom_cfg=True), SCALAR)
CASES["scalar-culls1-width90-rows"] = ("raw", dict(G1, w=90, n=4, flags=ROWS), SCALAR)
CASES["scalar-rgb"] = ("raw", dict(G1, n=4, channels=3), SCALAR)
CASES["scalar-rgba-rows"] = ("raw", dict(G1, n=4, channels=4, flags=ROWS | FORCE), SCALAR)
CASES["scalar-rgb-gray-only-culls2"] = ("raw", dict(G2, n=4, channels=3, depth=False), SCALAR)
CASES["scalar-float-culls0"] = ("float", dict(w=37, h=29, levels=3, culls=0, n=3, custom_cfg=True), SCALAR)
CASES["scalar-float-culls0-gray"] = ("float", dict(w=37, h=29, levels=3, culls=0, n=3, depth=False), SCALAR)
CASES["scalar-float-culls1-rows"] = ("float", dict(G1, w=90, n=3, flags=ROWS), SCALAR)
# the split build
for c, geo in ((1, S1), (2, S2)):
    for rows in (0, ROWS):
        CASES["split-culls%d-%s" % (c, "rows" if rows else "whole")] = ("raw", dict(geo, n=4, flags=SPLIT | rows | (FORCE if rows else 0),
                                                                                  custom_cfg=bool(rows)), SPLIT_OF[c])
# ... asked for where pyramid_can_split must refuse: a top width of 44 (not a multiple of 8), three sequences (alignment), gray only, a plan
CASES["split-refused-top-width-44"] = ("raw", dict(G1, n=4, flags=SPLIT), RAW4[1, 0])
CASES["split-refused-three-sequences"] = ("raw", dict(S1, n=3, flags=SPLIT), SCALAR)
CASES["split-refused-gray-only"] = ("raw", dict(S2, n=4, flags=SPLIT, depth=False), RAW4[2, 0])
CASES["split-refused-plan"] = ("raw", dict(S1, n=8, flags=SPLIT, actions=MIX), RAW4[1, 1])
# planned builds of every family that accepts a plan: eight sequences, a mix of SKIP, TRACK and RESTART, all SKIP, no SKIP
for name, acts in (("mix", MIX), ("all-skip", ALL_SKIP), ("no-skip", NO_SKIP)):
    CASES["plan-raw4-culls1-%s" % name] = ("raw", dict(G1, n=8, flags=ROWS, actions=acts), RAW4[1, 1])
    CASES["plan-raw4-culls2-%s" % name] = ("raw", dict(G2, n=8, actions=acts, custom_cfg=True), RAW4[2, 1])          # raw4<2, true> with depth
    CASES["plan-scalar-rgb-%s" % name] = ("raw", dict(G1, n=8, channels=3, actions=acts), SCALAR_PLAN)              # have[] from raw_depth
    CASES["plan-scalar-float-culls0-%s" % name] = ("float", dict(w=37, h=29, levels=3, culls=0, n=8, actions=acts), SCALAR_PLAN)
CASES["plan-raw4-culls2-gray-mix"] = ("raw", dict(G2, n=8, depth=False, actions=MIX), RAW4[2, 1])
CASES["plan-scalar-rgba-gray-mix"] = ("raw", dict(G2, n=8, channels=4, depth=False, flags=ROWS, actions=MIX), SCALAR_PLAN)
CASES["plan-scalar-culls1-five-sequences"] = ("raw", dict(G1, n=5, actions=MIX[:5]), SCALAR_PLAN)
CASES["plan-scalar-float-culls1-gray"] = ("float", dict(G1, w=90, h=73, n=8, depth=False, actions=MIX), SCALAR_PLAN)


def test_the_cases_name_every_instance():
    named = set()
    for _, _, kernel in CASES.values():
        named |= set(kernel.split(" + "))
    assert named == INSTANCES and len(INSTANCES) == 10


@pytest.mark.parametrize("case", sorted(CASES))
def test_build_matches_reference(case):
    kind, kw, kernel = CASES[case]
    got, want = _check(case, kind, kw, kernel)
    # the frames do what the case needs: holes, valid pixels and (float maps at culls 0) the NaN reach the top level
    top = got["gray"][kw["levels"] - 1]
    if kw.get("depth", True):
        assert (top == pref.INVALID).any() and (top > 0).any()
        assert all(not np.array_equal(_bits(got["depth"][0][0]), _bits(got["depth"][0][q])) for q in range(1, kw["n"]))
    if kind == "float" and kw["culls"] == 0 and kw.get("actions") is None:
        assert np.isnan(top[0, 0, 0]) and np.isnan(top[0, 4, 8]) and not np.isnan(got["gray"][0]).any()
    if kw.get("actions") is not None and S in kw["actions"]:
        q = kw["actions"].index(S)
        assert not (top[q] == F32(0xA5) * F32(1.0 / 255.0)).all() and not (top[q] == 12345.0).any()    # the garbage frame was not read


@pytest.mark.parametrize("culls", [1, 2])
@pytest.mark.parametrize("rows", [0, ROWS])
def test_split_build_equals_the_single_kernel(culls, rows):
    """the two halves leave, bit for bit, what the unsplit op leaves; and the coarse kernel's own guards fire at this shape: in the
    coordinates of level top - 1 (36 x 36) some lower level drops a column and a row"""
    geo = S1 if culls == 1 else S2
    cw = (geo["w"] >> culls) >> 1
    assert any(((cw - 1) >> t) >= (cw >> t) for t in range(1, geo["levels"] - 1))
    two, _ = _run_raw(n=4, flags=SPLIT | rows, **geo)
    one, _ = _run_raw(n=4, flags=rows, **geo)
    assert two["kernel"].name() == SPLIT_OF[culls] and one["kernel"].name() == RAW4[culls, 0]
    for m in pref.MAPS:
        for l in range(geo["levels"]):
            assert np.array_equal(_bits(one[m][l]), _bits(two[m][l])), (m, l)


def test_skip_copies_forward_from_a_culls0_reference_through_pass_valid():
    """a SKIP sequence of a culls 0 set: the top level keeps the reference's NaN, every level below stores INVALID for it"""
    acts = (S, T, S)
    got, want = _run_float(37, 29, 3, 0, 3, actions=acts)
    assert got["kernel"].name() == SCALAR_PLAN
    for q in (0, 2):
        assert np.isnan(got["gray"][2][q, 0, 0]) == (q % 2 == 0) and np.isnan(got["gray"][2][q, 4, 8])
        assert got["gray"][1][q, 2, 4] == pref.INVALID and got["gray"][0][q, 1, 2] == pref.INVALID
    _assert_maps(got, want, 3, "culls 0 copy-forward")
