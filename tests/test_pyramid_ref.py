"""CPU tests of tests/pyramid_ref.py, the reference tests/test_gpu_pyramid_build.py holds the device to: its levels and the values
it lets through are the oracle's (orc.OFrame, orc.cull_image) bit for bit on float maps with NaN, -7, +-inf and INVALID pixels at
ragged sizes, its luma is the fixed-point BGR2GRAY on all 256 gray levels and in the channel-order cases, its weight is one float32
division, and a plan's copy-forward equals building the reference frame again."""
import numpy as np
import pytest

import orc
import pyramid_ref as pref

F32 = np.float32
K = np.array([100, 0, 20, 0, 100, 15, 0, 0, 1], F32)


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _maps(w, h, seed):
    rng = np.random.RandomState(seed)
    g = rng.rand(h, w).astype(F32)
    d = (0.5 + 3.0 * rng.rand(h, w)).astype(F32)
    s = (0.001 + 0.7 * rng.rand(h, w)).astype(F32)     # below sigma_min and above sigma_max too
    for m in (g, d, s):
        for v in (np.nan, -7.0, pref.INVALID, -np.inf, np.inf, 0.0):
            m[rng.rand(h, w) < 0.03] = v
        m[0, 0] = np.nan                                # a pixel every level keeps
    return g, d, s


# (w, h, levels, culls): ragged sizes -- some level drops a column / row of the level above -- and culls 0, 1, 2
SHAPES = [(37, 29, 3, 0), (88, 72, 4, 1), (90, 73, 4, 1), (176, 144, 4, 2), (178, 147, 4, 2), (144, 144, 5, 1)]


@pytest.mark.parametrize("w,h,levels,culls", SHAPES)
def test_levels_are_the_oracles(w, h, levels, culls):
    g, d, s = _maps(w, h, 3)
    ref = pref.build(w, h, levels, culls, g[None], d[None], s[None])
    of = orc.OFrame(g, d, s, K, levels, culls)
    for l in range(levels):
        assert of.size(l) == pref.level_shape(w, h, levels, culls, l)[::-1]
        for name, want in (("gray", of.gray(l)), ("depth", of.depth(l)), ("sigma", of.sigma(l))):
            assert np.array_equal(_bits(ref[name][l][0]), _bits(want)), (name, l)
        # and level l is the cull of the input by culls + (levels - 1 - l): from the header's sentence alone
        t = culls + levels - 1 - l
        if t > 0:
            assert np.array_equal(_bits(ref["gray"][l][0]), _bits(orc.cull_image(g, t)))
    assert np.isnan(ref["gray"][levels - 1][0, 0, 0]) == (culls == 0)      # only a culls 0 top level keeps a NaN
    assert ref["gray"][0][0, 0, 0] == pref.INVALID


def test_rows_decimated_input_gives_the_same_levels():
    w, h, levels, culls = 88, 72, 4, 1
    g, d, s = _maps(w, h, 4)
    whole = pref.build(w, h, levels, culls, g[None], d[None], s[None])
    rows = pref.build(w, h, levels, culls, g[None, ::2], d[None, ::2], s[None, ::2], rows_decimated=True)
    for m in pref.MAPS:
        for l in range(levels):
            assert np.array_equal(_bits(whole[m][l]), _bits(rows[m][l])), (m, l)


def test_pass_valid():
    a = np.array([np.nan, -np.inf, -7.0, -2.0, np.nextafter(F32(-2), F32(0)), -0.0, 0.0, 1.0, np.inf], F32)
    want = np.array([-2.0, -2.0, -2.0, -2.0, np.nextafter(F32(-2), F32(0)), -0.0, 0.0, 1.0, np.inf], F32)
    assert np.array_equal(_bits(pref.pass_valid(a)), _bits(want))


def test_weight_is_one_division_of_the_clamped_sigma():
    sig = np.array([-2.0, 0.0, 0.001, 0.01, 0.1, 0.3, 0.5, 0.7, 1.0, np.inf, -np.inf], F32)
    cl = np.array([0.01, 0.01, 0.01, 0.01, 0.1, 0.3, 0.5, 0.5, 0.5, 0.5, 0.01], F32)
    for step in pref.steps(4):
        assert np.array_equal(_bits(pref.weight(sig, step)), _bits(np.array([F32(step) / c for c in cl], F32)))
    assert [float(x) for x in pref.steps(5)] == [2.0, 1.5, 1.0, 2.0, 2.0]          # optimize.cpp:22-26
    assert np.isnan(pref.weight(np.array([np.nan], F32), F32(2.0)))[0]


def test_luma_on_all_gray_levels_and_channel_orders():
    v = np.arange(256, dtype=np.uint8)
    gray3 = np.stack([v, v, v], -1)
    assert np.array_equal(pref.luma(gray3), v.astype(np.uint32))                     # the coefficients sum to 2^14
    assert np.array_equal(pref.luma(np.concatenate([gray3, (255 - v)[:, None]], -1)), v.astype(np.uint32))   # alpha is not read
    # the channel order is R, G, B: cv::COLOR_BGR2GRAY's fixed-point weights (R 4899, G 9617, B 1868 of 2^14), rounded to nearest
    one = lambda r, g, b: int(pref.luma(np.array([[r, g, b]], np.uint8))[0])
    assert (one(255, 0, 0), one(0, 255, 0), one(0, 0, 255)) == (76, 150, 29)
    assert one(1, 0, 0) == 0 and one(0, 1, 0) == 1 and one(2, 0, 0) == 1            # (8192 + 4899 < 2^14 <= 8192 + 9617)
    rng = np.random.RandomState(0)
    px = rng.randint(0, 256, (5000, 4)).astype(np.uint8)
    want = [(int(p[0]) * 4899 + int(p[1]) * 9617 + int(p[2]) * 1868 + 8192) // 16384 for p in px]
    assert np.array_equal(pref.luma(px), np.array(want, np.uint32))
    assert np.array_equal(pref.luma(px[:, :3]), pref.luma(px))


def test_conversion():
    g8 = np.arange(256, dtype=np.uint8).reshape(1, 16, 16)
    d16 = np.arange(256, dtype=np.uint16).reshape(1, 16, 16) * 257
    d16[0, 3, 3] = 0
    g, d, s = pref.convert(g8, d16)
    assert np.array_equal(_bits(g[d16 > 0]), _bits(g8[d16 > 0].astype(F32) * F32(1.0 / 255.0)))
    assert (g[d16 == 0] == pref.INVALID).all() and (d16 == 0).sum() == 2
    assert np.array_equal(_bits(d), _bits(d16.astype(F32) * (F32(1.0) / F32(5000.0)))) and d.max() == F32(65535) * (F32(1) / F32(5000))
    assert np.array_equal(_bits(s), _bits(np.where(d16 > 0, F32(0.1), F32(1.0))))
    g, d, s = pref.convert(g8, d16, depth_scale=0.001)
    assert np.array_equal(_bits(d), _bits(d16.astype(F32) * F32(0.001)))
    g, d, s = pref.convert(g8)
    assert d is None and s is None and g[0, 0, 0] == 0 and g[0, 15, 15] == 1.0
    rgb = np.stack([g8, g8, g8], -1)
    assert np.array_equal(_bits(pref.convert(rgb)[0]), _bits(g))


def test_copy_forward_equals_building_the_reference_frame_again():
    w, h, levels, culls = 90, 73, 4, 0
    n = 3
    a = [np.stack(m) for m in zip(*[_maps(w, h, 10 + q) for q in range(n)])]
    b = [np.stack(m) for m in zip(*[_maps(w, h, 20 + q) for q in range(n)])]
    A = pref.build(w, h, levels, culls, *a)
    B = pref.build(w, h, levels, culls, *b)
    out = pref.planned(A, B, [pref.SEQ_SKIP, pref.SEQ_TRACK, pref.SEQ_RESTART], levels)
    for m in pref.MAPS:
        for l in range(levels):
            assert np.array_equal(_bits(out[m][l][0]), _bits(A[m][l][0])), (m, l)     # (a NaN at the culls 0 top included)
            assert np.array_equal(_bits(out[m][l][1:]), _bits(B[m][l][1:])), (m, l)
    assert not np.array_equal(_bits(A["gray"][0][0]), _bits(B["gray"][0][0]))


def test_guards_fire_is_computed_from_the_shape():
    assert pref.guards_fire(88, 72, 4, 1) == (True, True)      # top 44 x 36: 11 x 9 -> 5 x 4
    assert pref.guards_fire(176, 144, 4, 2) == (True, True)
    assert pref.guards_fire(144, 144, 5, 1) == (True, True)    # top 72: 9 -> 4
    assert pref.guards_fire(128, 96, 4, 1) == (False, False)   # every level a multiple of the next
    assert pref.guards_fire(640, 480, 4, 1) == (False, False)
