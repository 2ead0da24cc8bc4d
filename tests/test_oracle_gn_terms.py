"""orc.optimize_terms (the oracle's per-pixel Gauss-Newton terms) against orc.optimize on the inputs the GPU parity tests use.

The contributing pixels are the set bits of optimize's mask, in raster order; n_valid is their count; and float64 sums of the float
products reproduce optimize's H, g, sum_r2.  The oracle adds the same exact products in double in raster order (n roundings of at
most 2^-53 of a partial sum each), numpy adds them pairwise (fewer roundings), so the two differ by at most n * 2^-53 times the sum of
the absolute terms.  No GPU."""
import numpy as np
import pytest

import orc
from dvo_amd import synth
from gn_sums import exact_sums
from util import K640, frames, level_maps

INV = np.float32(-2.0)


def _check(og, rg, rd, rs, K, xi, level, crop=True):
    o = orc.optimize(og, rg, rd, rs, K, xi, level, crop=crop, want_mask=True)
    t = orc.optimize_terms(og, rg, rd, rs, K, xi, level, crop=crop)
    np.testing.assert_array_equal(t["index"], np.flatnonzero(o["mask"].ravel()))      # the mask's set bits, raster order
    assert t["n_valid"] == o["n_valid"] == len(t["index"]) == len(t["r"]) == len(t["rw"]) == t["J"].shape[0]
    assert t["J"].dtype == t["r"].dtype == t["rw"].dtype == np.float32 and t["shape"] == rg.shape
    np.testing.assert_array_equal(t["H"], o["H"]); np.testing.assert_array_equal(t["g"], o["g"])   # the same call underneath
    assert t["sum_r2"] == o["sum_r2"]
    ex = exact_sums(t)
    assert ex["n"] == o["n_valid"]
    eps = ex["n"] * 2.0 ** -53
    assert (np.abs(ex["H"] - o["H"]) <= eps * ex["A_H"]).all(), np.abs(ex["H"] - o["H"]) / np.maximum(ex["A_H"], 1e-300)
    assert (np.abs(ex["g"] - o["g"]) <= eps * ex["A_g"]).all(), np.abs(ex["g"] - o["g"]) / np.maximum(ex["A_g"], 1e-300)
    assert abs(ex["sum_r2"] - o["sum_r2"]) <= eps * ex["A_r"]
    assert (ex["A_H"] >= np.abs(ex["H"])).all() and (ex["A_g"] >= np.abs(ex["g"])).all()
    return o, t


@pytest.mark.parametrize("level", [0, 1, 2, 3])
def test_terms_reproduce_optimize_every_level(level):
    g, d, s, _ = frames()
    ref = orc.OFrame(g[0], d[0], s[0], K640, 4, 1)
    obj = orc.OFrame(g[1], d[1], s[1], K640, 4, 1)
    xi = np.array([0.002, -0.001, 0.003, 0.002, -0.001, 0.001], np.float32)
    o, _ = _check(obj.gray(level), *level_maps(ref, level), xi, level)
    assert o["n_valid"] > 500


def holed_frame():
    """the inputs of test_gpu_parity.test_gn_step_invalid_pixels_borders_and_crop_off"""
    g, d, s, _ = frames()
    ref = orc.OFrame(g[0], d[0], s[0], K640, 3, 2)
    obj = orc.OFrame(g[2], d[2], s[2], K640, 3, 2)
    rg, rd, rs, K = ref.gray(2), ref.depth(2), ref.sigma(2), ref.K(2)
    og = obj.gray(2)
    rng = np.random.RandomState(5)
    rg[rng.uniform(size=rg.shape) < 0.03] = INV
    og[rng.uniform(size=og.shape) < 0.03] = INV
    rd[rng.uniform(size=rd.shape) < 0.05] = 0.0
    rd[30:40, 50:60] = 0.15
    rs[:, :80] = 0.003; rs[:, 80:] = 0.8
    rg[60, 60:70] = 0.0
    xi = np.array([0.03, -0.02, 0.01, 0.01, 0.02, -0.015], np.float32)
    return og, rg, rd, rs, K, xi


@pytest.mark.parametrize("crop", [True, False])
def test_terms_on_the_holed_frame(crop):
    og, rg, rd, rs, K, xi = holed_frame()
    o, t = _check(og, rg, rd, rs, K, xi, 2, crop=crop)
    assert o["n_valid"] > 100
    if crop:   # optimize.cpp:33-36: nothing outside the window
        y, x = np.divmod(t["index"], rg.shape[1])
        assert x.min() >= 20 and x.max() <= 140 and y.min() >= 20 and y.max() <= 100


def test_terms_without_a_valid_pixel():
    z = np.zeros((30, 40), np.float32)
    K = np.array([[30, 0, 20], [0, 30, 15], [0, 0, 1]], np.float32)
    o, t = _check(z + 0.5, z + 0.5, z, z + 0.5, K, np.zeros(6, np.float32), 0)
    assert t["n_valid"] == 0 and t["index"].size == 0 and t["J"].shape == (0, 6)
    ex = exact_sums(t)
    assert not ex["H"].any() and not ex["A_H"].any() and ex["sum_r2"] == 0.0


@pytest.mark.parametrize("w,h,levels,culls,seed", [(322, 243, 3, 0, 11), (96, 320, 2, 0, 5)])
def test_terms_on_a_ragged_and_a_narrow_tile_size(w, h, levels, culls, seed):
    """one size of test_ragged_sizes_parity and one of test_narrow_2d_tiles_parity, every level, crop off as there"""
    K = np.array(synth.K_640, np.float32).copy()
    K[0] *= w / 640.0; K[1] *= h / 480.0
    g, d, s, _ = synth.sequence(2, width=w, height_px=h, K=K, seed=seed, sigma_value=0.5)
    g, d, s = g.numpy(), d.numpy(), s.numpy()
    ref = orc.OFrame(g[0], d[0], s[0], K, levels, culls)
    obj = orc.OFrame(g[1], d[1], s[1], K, levels, culls)
    xi = np.array([0.004, -0.003, 0.002, 0.003, -0.002, 0.004], np.float32)
    for l in range(levels):
        o, _ = _check(obj.gray(l), *level_maps(ref, l), xi, l, crop=False)
        assert o["n_valid"] > 0


def test_terms_are_canonical_and_sequential_whatever_the_oracle_mode():
    """optimize_terms is one thread and canonical arithmetic even while a sensitivity measurement has the oracle in another mode"""
    g, d, s, _ = frames()
    ref = orc.OFrame(g[0], d[0], s[0], K640, 4, 1)
    obj = orc.OFrame(g[1], d[1], s[1], K640, 4, 1)
    xi = np.array([0.002, -0.001, 0.003, 0.002, -0.001, 0.001], np.float32)
    a = orc.optimize_terms(obj.gray(1), *level_maps(ref, 1), xi, 1)
    orc.set_threads(3)
    try:
        with orc.literal(orc.LIT_ARITH):
            b = orc.optimize_terms(obj.gray(1), *level_maps(ref, 1), xi, 1)
    finally:
        orc.set_threads(1)
    for k in ("index", "J", "r", "rw", "H", "g"):
        np.testing.assert_array_equal(a[k], b[k])
