"""NaN and +-inf pixels in the four maps a Gauss-Newton step reads ("Non-finite pixels"): one builder of the cases and
the table of what the oracle makes of them, shared by tests/test_nonfinite_cases_oracle.py (CPU: pins the table on the oracle alone)
and tests/test_gpu_nonfinite_pixels.py (holds the kernels to it).

`obj_gray` is the per-pixel image (I1 of optimize.cpp:44), `ref_gray` the sampled one (I2 and both gradients), `ref_depth` and
`ref_sigma` the reference's maps.  is_valid(v) = -2 < v and is_invalid(v) = v <= -2 are BOTH false for NaN: the per-pixel gates use
is_invalid, getPixel and the fill loop of getSubpixel use is_valid, so the same NaN is "not invalid" in obj_gray and "not valid" in
ref_gray.  Huge finite values are no case here: the device forms the products in float32 and the oracle in double, so they overflow
on one side only, and gray is specified in [0, 1]."""
import functools

import numpy as np

import orc

NAN, PINF, NINF = np.float32(np.nan), np.float32(np.inf), np.float32(-np.inf)
MAPS = ("obj_gray", "ref_gray", "ref_depth", "ref_sigma")
SIZES = ((96, 50), (128, 33), (5, 7))     # raster tiles; 64-column 2-D tiles with a partial last tile; one partial tile
BIG = SIZES[:2]
PLACEMENTS = ("sprinkle", "full")          # 2 % of the map; the same plus a solid 7x7 block, every third pixel of row 0 and of column 0 and the last pixel
SINGLE = (51, 21)                          # placement "single": this pixel alone (inside both larger sizes and the level-2 crop)
LEVELS = (0, 1, 2)                         # the level index picks the step (2.0, 1.5, 1.0) and, at 2, the crop of optimize.cpp:33-36

# (map, value) -> class.  "finite": every per-pixel term of the oracle is finite.  Otherwise the per-entry pattern of the oracle's
# sums and update at the two larger sizes: '.' finite, 'n' NaN, '+' / '-' the infinities; H (21), g (6), sum_r2, xi_update (6).
# "gated": no marked pixel contributes; "filled": marked pixels contribute with values the fill quirk / the sigma clamp gives them.
FINITE = {
    ("ref_gray", "nan"): "filled", ("ref_gray", "-inf"): "filled",
    ("obj_gray", "-inf"): "gated",
    ("ref_depth", "nan"): "gated", ("ref_depth", "+inf"): "gated", ("ref_depth", "-inf"): "gated",
    ("ref_sigma", "+inf"): "filled", ("ref_sigma", "-inf"): "filled",
}
POISON = {
    ("obj_gray", "nan"): dict(H="." * 21, g="n" * 6, sum_r2="n", xi_update="n" * 6),
    ("obj_gray", "+inf"): dict(H="." * 21, g="n" * 6, sum_r2="+", xi_update="n" * 6),
    ("ref_gray", "+inf"): dict(H="n" * 21, g="n" * 6, sum_r2="+", xi_update="." * 6),      # non-finite diagonal: a zero update, no pseudo-inverse
    ("ref_sigma", "nan"): dict(H="." * 21, g="n" * 6, sum_r2=".", xi_update="n" * 6),
}
VALUES = {"nan": NAN, "+inf": PINF, "-inf": NINF}
CASES = tuple(sorted(FINITE)) + tuple(sorted(POISON))


def classes(v):
    """one character per entry: '.' finite, 'n' NaN, '+' +inf, '-' -inf"""
    v = np.asarray(v, np.float64).ravel()
    return "".join("n" if np.isnan(x) else "+" if x == np.inf else "-" if x == -np.inf else "." for x in v)


def build(where, value, placement="sprinkle", size=(96, 50), frac=0.02, seed=0, scale=0.01):
    """dict(obj_gray, ref_gray, ref_depth, ref_sigma, K, xi, mark): a smooth synthetic pair of `size` = (w, h) whose map `where` holds
    `value` (a key of VALUES, a float, or None for the clean pair) at the pixels of the boolean `mark`."""
    w, h = size
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)

    def tex(sx, sy):
        return (0.5 + 0.22 * np.sin(0.35 * (xx + sx)) * np.cos(0.27 * (yy + sy)) + 0.15 * np.sin(0.1 * (xx + sx) + 0.13 * (yy + sy))).astype(np.float32)
    maps = dict(ref_gray=tex(0, 0), obj_gray=tex(0.4, -0.3),
                ref_depth=(1.2 + 0.4 * np.sin(0.05 * xx) + 0.3 * np.cos(0.07 * yy)).astype(np.float32),
                ref_sigma=np.full((h, w), 0.1, np.float32))
    mark = rng.uniform(size=(h, w)) < frac
    if placement == "single":
        mark[:] = False
        mark[SINGLE[1], SINGLE[0]] = True
    elif placement == "full":
        mark[20:27, 40:47] = True
        mark[0, :] |= np.arange(w) % 3 == 0
        mark[:, 0] |= np.arange(h) % 3 == 0
        mark[-1, -1] = True
    else:
        assert placement == "sprinkle", placement
    if value is None:
        mark[:] = False
    else:
        maps[where][mark] = VALUES[value] if isinstance(value, str) else np.float32(value)
    f = 0.9 * max(w, h)
    maps["K"] = np.array([f, 0, w / 2 - 0.3, 0, f, h / 2 + 0.2, 0, 0, 1], np.float32)
    maps["xi"] = (scale * rng.standard_normal(6)).astype(np.float32)
    maps["mark"] = mark
    return maps


DIAGONAL = (0, 6, 11, 15, 18, 20)          # H(i, i) in the 21-entry upper triangle


def device_update_class(terms):
    """What the device's solve makes of the exact sums of `terms`, where it is not simply the oracle's answer:
    "oracle" -- H is finite (a non-finite g gives NaN on both sides), or no diagonal sum of H is > 0 (all of them NaN: both sides
    return the zero update without a pseudo-inverse); "nan" -- H holds a NaN or an infinity and a diagonal sum is > 0 (+inf
    included): orc_solve6 drops every NaN eigenvalue and answers zero, which the tracker takes for convergence, solve6 answers NaN,
    which the tracker refuses."""
    import gn_sums
    P = gn_sums.per_entry_products(terms)
    cls = [gn_sums.sum_class(P[:, k]) for k in range(21)]
    if all(c == "." for c in cls):
        return "oracle"
    positive = any(cls[k] == "+" or (cls[k] == "." and P[:, k].sum() > 0) for k in DIAGONAL)
    return "nan" if positive else "oracle"


def assert_update_class(upd, o, terms, tag=""):
    """the device's update `upd` against orc.optimize's `o` at the same pose: the oracle's NaN pattern, its exact zero where it
    answers zero -- or all NaN where device_update_class says so"""
    upd = np.asarray(upd, np.float32)
    if o["n_valid"] > 0 and device_update_class(terms) == "nan":
        assert not o["xi_update"].any(), (tag, "the oracle answers zero on a non-finite H", o["xi_update"])
        assert np.isnan(upd).all(), (tag, "D13: NaN where a sum of H is not finite", upd)
        return "nan"
    assert np.array_equal(np.isnan(upd), np.isnan(o["xi_update"])), (tag, upd, o["xi_update"])
    if not o["xi_update"].any():
        assert not upd.any(), (tag, upd)
        return "zero"
    return "oracle"


def maps_of(c):
    """the positional arguments of orc.optimize / dvo.optimize up to the pose"""
    return c["obj_gray"], c["ref_gray"], c["ref_depth"], c["ref_sigma"], c["K"], c["xi"]


@functools.lru_cache(maxsize=None)
def reference(where, value, placement, size, level):
    """(case, orc.optimize with its mask, orc.optimize_terms) of one case: computed once per process and never written to"""
    c = build(where, value, placement, size)
    o = orc.optimize(*maps_of(c), level, want_mask=True)
    t = orc.optimize_terms(*maps_of(c), level)
    return c, o, t


# ---- a full track: 128 x 96, 3 levels, culls = 0, one marked pixel at (x, y) = (51, 37): odd, so only the finest level holds it
TRACK_SIZE = (128, 96)
TRACK_PIXEL = (51, 37)
TRACK_CASES = (("obj_gray", "nan"), ("obj_gray", "+inf"), ("ref_sigma", "nan"), ("ref_gray", "+inf"), ("ref_gray", "nan"))
REFUSED = (("obj_gray", "nan"), ("obj_gray", "+inf"), ("ref_sigma", "nan"))     # every finest-level update is refused: the level runs to the cap


def build_track(where, value, pixel=TRACK_PIXEL, size=TRACK_SIZE):
    """the clean pair of build() at `size` with one marked pixel (None: none)"""
    c = build(where, None, size=size)
    if value is not None:
        c[where][pixel[1], pixel[0]] = VALUES[value]
        c["mark"][pixel[1], pixel[0]] = True
    f = 0.9 * size[0]
    c["K"] = np.array([f, 0, size[0] / 2 - 0.3, 0, f, size[1] / 2 + 0.2, 0, 0, 1], np.float32)
    return c


def oracle_frames(c, levels=3, culls=0):
    ref = orc.OFrame(c["ref_gray"], c["ref_depth"], c["ref_sigma"], c["K"], levels, culls)
    obj = orc.OFrame(c["obj_gray"], None, None, c["K"], levels, culls)
    return obj, ref
