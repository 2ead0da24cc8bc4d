"""Per-entry bound on the 28 Gauss-Newton sums of the device (H: 21, g: 6, sum_r2) against exact sums of the oracle's per-pixel terms.

DESIGN.md §3: the per-pixel values J[6], r, r*w are the same bits on the device and in the oracle; only the reduction differs.
DESIGN.md §6 ("The reduction bound") reads the shape of the device's reduction off the kernels and counts the float32 roundings on
its longest path (`depth`).  Every rounding is a relative error of at most u = 2^-24 of a partial sum, and no partial sum of an entry
exceeds that entry's sum of absolute terms A, so

    |S_gpu - S_exact| <= ((1 + u)^depth - 1) * A  <=  depth * u * (1 + 2^-10) * A        per entry.

The factor (1 + 2^-10) covers everything of second order (§6 has the figures): depth^2 u^2 / 2, the double-precision tails of the
device (one 2^-53 rounding per partial row), and the error of the float64 reference sums below.  The only number in this module is
`depth`, and it comes from the code: nothing here is tuned on a device result.
"""
import functools
import re

import numpy as np

U32 = 2.0 ** -24                 # unit roundoff of float32 (round to nearest)
SECOND_ORDER = 1.0 + 2.0 ** -10  # see the module docstring

RATIOS = []        # (tag, largest error / bound of that call): what DESIGN.md §6 tabulates; never a pass criterion (that is <= 1)
_nonempty_calls = 0
_reported = 0      # RATIOS[:_reported] have been printed by an earlier report()


def nonempty_calls():
    """How often assert_gn_sums has passed with a non-empty term list: a test reads it before and after its work and asserts that it
    grew, so that a helper which is silently skipped fails the test."""
    return _nonempty_calls


def must_be_used(test):
    """decorator of a test that relies on assert_gn_sums: it fails unless the helper passed at least once on a non-empty term list"""
    @functools.wraps(test)
    def run(*args, **kw):
        before = _nonempty_calls
        out = test(*args, **kw)
        assert _nonempty_calls > before, "assert_gn_sums was not called with a non-empty term list"
        return out
    return run


def exact_sums(terms):
    """The 21 + 6 + 1 sums of orc.optimize_terms() output in float64 and, beside each, the sum of the absolute values of its terms:
    H / A_H[k] = sum J_a J_b / sum |J_a J_b| (upper triangle, row major), g / A_g[a] = sum J_a rw / sum |J_a rw|, sum_r2 = A_r = sum r^2.

    The product of two float32 values is exact in float64 (48 significant bits), so only the summation rounds.  numpy sums a
    contiguous float64 vector pairwise (blocks of 128, eight running sums each): its error is below (log2(n) + 16) * 2^-53 * A, far
    below n * 2^-53 * A, and even that is more than four orders under the float32 bound (17 * 2^-24) at every size in the suite
    (n <= 2.1e6 at 1080p: n * 2^-53 = 2.3e-10 against 1e-6)."""
    J = np.ascontiguousarray(terms["J"], np.float64).reshape(-1, 6)
    r = np.ascontiguousarray(terms["r"], np.float64); rw = np.ascontiguousarray(terms["rw"], np.float64)
    H = np.zeros(21); A_H = np.zeros(21); g = np.zeros(6); A_g = np.zeros(6)
    k = 0
    for a in range(6):
        for b in range(a, 6):
            p = J[:, a] * J[:, b]
            H[k] = p.sum(); A_H[k] = np.abs(p).sum(); k += 1
        p = J[:, a] * rw
        g[a] = p.sum(); A_g[a] = np.abs(p).sum()
    s = float((r * r).sum())
    return dict(H=H, g=g, sum_r2=s, A_H=A_H, A_g=A_g, A_r=s, n=int(J.shape[0]))


def reduction_depth(ppt=None, kernel="gn_tile"):
    """Float32 roundings on the longest path from a per-pixel term to a finished sum ("The reduction bound").

    kernel = "gn_tile": k_track_gn, k_track_gn_cam, k_track_gn_fused, k_track_level and the tile loop of k_track_persist, i.e.
      everything built on gn_tile(), for raster tiles (256 * ppt pixels) and the 64-, 32- and 16-column 2-D tiles alike:
        ppt  Acc29::add of the thread's own pixels (one fmaf per pixel and accumulator; the gather group only reorders loads),
      + ppt  Acc29::add in the deferred loop (e = threadIdx.x; e < total; e += 256 with total <= 256 * ppt queued pixels),
      + 6    wave_reduce29_packed (permlane32, permlane16, row_shl/shr 8, row_shl/shr 4, two quad_perm steps: one add each),
      + 3    ((red[0] + red[1]) + red[2]) + red[3] over the four waves;
      the rest (sum_partial_rows / sum_partial_class, k_gn_solve) is double precision.
    kernel = "lds_patch": k_track_gn_tile evaluates border pixels in place (gn_sample_slow) and has no deferred loop: ppt + 6 + 3.

    ppt is the shape the level RAN: a test reads it per level from the plan in force (Batch.level_plan / MonoBatch.level_plan, i.e.
    dvo_debug_batch_level_plan; plan_depths() below), whether the config fixed it or left the choice to the engine
    (gn_pixels_per_thread = 0: Tracker::init halves from 4 per level, so the levels of one call differ).

    ppt = None is the fallback of a caller without a handle (the one-evaluation operators of a default config): the engine's choice
    is 1, 2 or 4, so the largest possible depth, that of 4, is used.  A batch test must not use it."""
    if ppt is None or ppt == 0:
        ppt = 4
    assert ppt in (1, 2, 4, 8), ppt
    assert kernel in ("gn_tile", "lds_patch"), kernel
    return (2 * ppt if kernel == "gn_tile" else ppt) + 6 + 3


def depth_for_cfg(cfg=None):
    """reduction_depth of the kernel a dvo_config selects (None: the defaults)"""
    ppt = getattr(cfg, "gn_pixels_per_thread", 0) if cfg is not None else 0
    lds = getattr(cfg, "gn_use_lds_patch", -1) if cfg is not None else -1
    return reduction_depth(ppt if ppt in (1, 2, 4, 8) else None, "lds_patch" if lds > 0 else "gn_tile")


def plan_depths(handle, levels):
    """reduction_depth per pyramid level of the plan in force on a Batch / MonoBatch (level_plan): the shape each level runs"""
    import dvo_amd
    out = []
    for l in range(levels):
        p = handle.level_plan(l)
        out.append(reduction_depth(p["ppt"], "lds_patch" if p["schedule"] == dvo_amd.PLAN_LDS_PATCH else "gn_tile"))
    return out


def at_level(x, level):
    """x[level] of a per-level sequence, x itself of a single value (a harness takes either for its depth / ppt)"""
    return x[level] if isinstance(x, (list, tuple)) else x


def factor(depth):
    """depth * 2^-24 * (1 + 2^-10): what multiplies an entry's sum of absolute terms A in its bound"""
    return depth * U32 * SECOND_ORDER


def bounds(ex, depth):
    """the per-entry bounds (H: 21, g: 6, sum_r2) for exact_sums() output"""
    f = factor(depth)
    return f * ex["A_H"], f * ex["A_g"], f * ex["A_r"]


def sum_groups(got, ex, bH, bg, br):
    """the (name, values, exact, bound) groups of the 28 sums for assert_entries"""
    return [("H", got["H"], ex["H"], bH), ("g", got["g"], ex["g"], bg), ("sum_r2", [got["sum_r2"]], [ex["sum_r2"]], [br])]


def assert_entries(groups, depth, tag=""):
    """The per-entry bound check, for (name, values, exact, bound) groups of device sums: an entry whose bound is zero (every term of
    it is zero) must be exactly zero, every other entry has error / bound <= 1.  depth only labels a failure (one value, or text where
    the groups differ).  Returns the largest ratio (0.0 without entries); the caller records it under its own tag."""
    worst = 0.0
    for name, val, ref, bnd in groups:
        val = np.asarray(val, np.float64).ravel(); ref = np.asarray(ref, np.float64).ravel(); bnd = np.asarray(bnd, np.float64).ravel()
        assert np.isfinite(bnd).all() and np.isfinite(ref).all(), "%s: the reference terms of %s are not finite" % (tag, name)
        err = np.abs(val - ref)
        for k in range(val.size):
            entry = "%s[%d]" % (name, k) if val.size > 1 else name
            if bnd[k] == 0.0:
                assert val[k] == 0.0, "%s: %s = %r, but every term of it is zero" % (tag, entry, val[k])
                continue
            ratio = err[k] / bnd[k]
            assert ratio <= 1.0, "%s: %s = %.17g, exact %.17g: error %.3g is %.3g times the bound %.3g (depth %s)" % (
                tag, entry, val[k], ref[k], err[k], ratio, bnd[k], depth)
            worst = max(worst, float(ratio))
    return worst


def assert_gn_sums(got, terms, depth, tag=""):
    """`got` (H, g, sum_r2, n_valid of the device) against the exact sums of `terms` (orc.optimize_terms): per entry
    |got - exact| <= depth * 2^-24 * (1 + 2^-10) * A; an entry whose A is zero must be exactly zero; n_valid is the term count.
    Returns the largest error / bound ratio (0.0 without terms) and appends (tag, ratio) to RATIOS."""
    global _nonempty_calls
    ex = exact_sums(terms)
    assert int(got["n_valid"]) == ex["n"], "%s: n_valid %d, %d terms" % (tag, int(got["n_valid"]), ex["n"])
    worst = assert_entries(sum_groups(got, ex, *bounds(ex, depth)), depth, tag)
    if ex["n"] > 0:
        _nonempty_calls += 1
    RATIOS.append((str(tag), worst))
    return worst


def per_entry_products(terms):
    """(n, 28) float64 products of the terms: 21 of H (upper triangle, row major), 6 of g, r^2.  A product of two float32 values is
    exact in float64 when both are finite; otherwise it is the same NaN / infinity in float32 and in float64 (inf * 0 is NaN in both)."""
    J = np.ascontiguousarray(terms["J"], np.float64).reshape(-1, 6)
    r = np.ascontiguousarray(terms["r"], np.float64); rw = np.ascontiguousarray(terms["rw"], np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        cols = [J[:, a] * J[:, b] for a in range(6) for b in range(a, 6)] + [J[:, a] * rw for a in range(6)] + [r * r]
    return np.stack(cols, axis=1) if J.shape[0] else np.zeros((0, 28))


def sum_class(p):
    """Class of the exact sum of the terms p, whatever the order they are added in: 'n' (NaN) if a term is NaN or if both infinities
    occur, '+' / '-' if infinities of one sign occur, '.' (finite) otherwise.  Finite float32 terms of the sizes at hand cannot carry
    a partial sum to an infinity, so a float32 tree and a float64 loop agree on the class: a derivation, no tolerance."""
    if np.isnan(p).any():
        return "n"
    pos, neg = bool((p == np.inf).any()), bool((p == -np.inf).any())
    return "n" if pos and neg else "+" if pos else "-" if neg else "."


def value_class(v):
    return "n" if np.isnan(v) else "+" if v == np.inf else "-" if v == -np.inf else "."


def assert_gn_sums_classes(got, terms, depth, tag=""):
    """assert_gn_sums for terms that may hold NaN / +-inf (a non-finite pixel that passed the gates), per entry of the 28:
    an entry whose terms are all finite obeys the bound of assert_gn_sums, depth * 2^-24 * (1 + 2^-10) * A, unchanged; every other
    entry must be of the class of its exact sum (sum_class): NaN, +inf or -inf.  n_valid is the term count.  Returns the largest
    error / bound ratio over the finite entries and appends (tag, ratio) to RATIOS."""
    global _nonempty_calls
    P = per_entry_products(terms)
    n = P.shape[0]
    assert int(got["n_valid"]) == n, "%s: n_valid %d, %d terms" % (tag, int(got["n_valid"]), n)
    val = np.concatenate([np.asarray(got["H"], np.float64).ravel(), np.asarray(got["g"], np.float64).ravel(), [float(got["sum_r2"])]])
    assert val.size == 28, val.size
    names = ["H[%d]" % k for k in range(21)] + ["g[%d]" % k for k in range(6)] + ["sum_r2"]
    finite = []
    for k in range(28):
        p = P[:, k]
        want = sum_class(p)
        if want != ".":
            assert value_class(val[k]) == want, "%s: %s = %r, but the exact sum of its terms is of class %r" % (tag, names[k], val[k], want)
            continue
        ref = float(p.sum())
        assert np.isfinite(val[k]), "%s: %s = %r, but every term of it is finite (exact %.17g)" % (tag, names[k], val[k], ref)
        finite.append((names[k], [val[k]], [ref], [factor(depth) * float(np.abs(p).sum())]))
    worst = assert_entries(finite, depth, tag)
    if n > 0:
        _nonempty_calls += 1
    RATIOS.append((str(tag), worst))
    return worst


def report(title):
    """what the last test of a file prints under -s: the ratios recorded since the previous report (the files of one pytest process
    share this module, and each prints its own), the largest first"""
    global _reported
    mine = RATIOS[_reported:]
    _reported = len(RATIOS)
    if not mine:
        print("\n%s: assert_gn_sums was not called" % title)
        return
    print("\n%s: %d calls of assert_gn_sums, largest error / bound = %.3f" % (title, len(mine), max(r for _, r in mine)))
    groups = {}      # a tag up to its first digit names the group ("kernel variants:", "sensor batch push", ...)
    for tag, r in mine:
        key = re.split(r"\d", tag, maxsplit=1)[0].strip() or tag
        n, worst = groups.get(key, (0, 0.0))
        groups[key] = (n + 1, max(worst, r))
    for key, (n, worst) in groups.items():
        print("    %-40s %4d calls, largest error / bound %.3f" % (key, n, worst))
    for tag, r in sorted(mine, key=lambda e: -e[1])[:5]:
        print("        %-100s %.3f" % (tag[:100], r))
