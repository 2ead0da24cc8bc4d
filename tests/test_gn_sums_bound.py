"""Self-test of the per-entry reduction bound of tests/gn_sums.py, on the oracle's terms alone.  No GPU.

What it shows: (1) a float32 reduction of the device's SHAPE stays inside the bound and a float32 running sum does not, so the bound
is a property of the tree and not a loose envelope; (2) subtly wrong sums -- a lost pixel, a row added twice, a Jacobian column off
by 2e-5, two entries exchanged, g off by 1e-4 -- are rejected by the bound, most of them while the max-scaled tolerances of
tests/util.py accept them; (3) the bound implies those tolerances on the suite's frames.

"Level 3 of the 640x480 frame" is what the GPU tests call so: util.frames() as a 4-level pyramid with one cull, 320 x 240 pixels."""
import numpy as np
import pytest

import gn_sums
import orc
from gn_sums import SECOND_ORDER, U32, assert_gn_sums, bounds, exact_sums, reduction_depth
from util import K640, TOL_H_REL, frames, level_maps

XI = np.array([0.002, -0.001, 0.003, 0.002, -0.001, 0.001], np.float32)   # the pose of test_gn_step_parity_every_level
DEPTH = reduction_depth(4)      # what the engine picks at most when left to choose
UPPER = [(a, b) for a in range(6) for b in range(a, 6)]


def level_terms(level, i_ref=0, i_obj=1):
    g, d, s, _ = frames()
    ref = orc.OFrame(g[i_ref], d[i_ref], s[i_ref], K640, 4, 1)
    obj = orc.OFrame(g[i_obj], d[i_obj], s[i_obj], K640, 4, 1)
    return orc.optimize_terms(obj.gray(level), *level_maps(ref, level), XI, level)


def per_pixel_products(t):
    """(n, 28) exact float64 products: 21 of H, 6 of g, r^2"""
    J = t["J"].astype(np.float64); r = t["r"].astype(np.float64); rw = t["rw"].astype(np.float64)
    cols = [J[:, a] * J[:, b] for a, b in UPPER] + [J[:, a] * rw for a in range(6)] + [r * r]
    return np.stack(cols, axis=1)


def as_result(v28, n):
    return dict(H=np.array(v28[:21], np.float64), g=np.array(v28[21:27], np.float64), sum_r2=float(v28[27]), n_valid=n)


def tree_model(t, ppt=4):
    """float32 model of the SHAPE of the device's reduction on raster tiles of 256 * ppt pixels -- per thread one rounding per pixel
    (thread = pixel index mod 256 inside the tile), a 6-level pairwise sum over the 64 lanes of a wave, ((w0 + w1) + w2) + w3 over
    the 4 waves, float64 over the workgroups.  The tree only: no device code, no lane permutation, no deferred queue."""
    h, w = t["shape"]
    T = 256 * ppt
    ntile = (w * h + T - 1) // T
    P = np.zeros((ntile * T, 28))
    P[t["index"]] = per_pixel_products(t)
    P = P.reshape(ntile, ppt, 256, 28)
    acc = np.zeros((ntile, 256, 28), np.float32)
    for k in range(ppt):                                   # fmaf(J_a, J_b, acc): exact product, one rounding
        acc = (acc.astype(np.float64) + P[:, k]).astype(np.float32)
    v = acc.reshape(ntile, 4, 64, 28)
    while v.shape[2] > 1:                                  # 6 levels
        v = (v[:, :, 0::2] + v[:, :, 1::2]).astype(np.float32)
    v = v[:, :, 0]
    row = ((v[:, 0] + v[:, 1]) + v[:, 2]) + v[:, 3]
    assert row.dtype == np.float32
    return as_result(row.astype(np.float64).sum(axis=0), len(t["index"]))


def old_lines_accept(got, ref):
    """the max-scaled comparison the GPU tests have always made (test_gpu_parity._gn_compare)"""
    try:
        np.testing.assert_allclose(got["H"], ref["H"], rtol=0, atol=TOL_H_REL * np.abs(ref["H"]).max())
        np.testing.assert_allclose(got["g"], ref["g"], rtol=0, atol=TOL_H_REL * max(np.abs(ref["g"]).max(), 1e-30))
        np.testing.assert_allclose(got["sum_r2"], ref["sum_r2"], rtol=2e-5)
    except AssertionError:
        return False
    return True


@pytest.mark.parametrize("level", [0, 1, 2, 3])
def test_a_reduction_of_the_devices_shape_stays_inside_the_bound(level):
    t = level_terms(level)
    for ppt in (1, 2, 4, 8):
        # the model has no deferred loop: ppt + 9 roundings, inside the bound of the kernels (2 * ppt + 9) a fortiori
        ratio = assert_gn_sums(tree_model(t, ppt), t, ppt + 9, "tree model level %d ppt %d" % (level, ppt))
        print("level %d, %d pixels per thread: largest error / bound of the float32 tree = %.3f" % (level, ppt, ratio))
        assert ratio > 0.0   # a float32 tree does round: the model is not the float64 sum in disguise


def test_a_float32_running_sum_breaks_the_bound():
    """depth n instead of ~17: the same terms, the same precision, another shape"""
    t = level_terms(3)
    P = per_pixel_products(t).astype(np.float32)
    run = np.cumsum(P, axis=0, dtype=np.float32)[-1]
    ex = exact_sums(t)
    bH, bg, br = bounds(ex, DEPTH)
    ratio = np.abs(run.astype(np.float64) - np.concatenate([ex["H"], ex["g"], [ex["sum_r2"]]])) / np.concatenate([bH, bg, [br]])
    print("float32 running sum over level 3 (%d terms): error / bound per entry, largest %.1f" % (ex["n"], ratio.max()))
    assert ratio.max() > 1.0
    with pytest.raises(AssertionError):
        assert_gn_sums(as_result(run, ex["n"]), t, DEPTH, "running sum")


def _mutations(t):
    """[(name, mutated result)]: every case is chosen from the oracle's terms alone"""
    ex = exact_sums(t)
    P = per_pixel_products(t)
    exact = np.concatenate([ex["H"], ex["g"], [ex["sum_r2"]]])
    h, w = t["shape"]
    out = []
    # (a) one contributing pixel lost: the one whose |J|^2 is the median of the level
    j2 = (t["J"].astype(np.float64) ** 2).sum(axis=1)
    p = int(np.argsort(j2, kind="stable")[len(j2) // 2])
    m = as_result(exact - P[p], ex["n"] - 1)
    m["n_valid"] = ex["n"]      # (the count is checked on its own: leave it right so that the SUMS have to give the loss away)
    out.append(("(a) the pixel of median |J|^2 (index %d) is lost" % int(t["index"][p]), m))
    # (b) the last contributing row of one 64 x 16 tile added twice: the tile that holds the image centre
    y, x = np.divmod(t["index"], w)
    tx, ty = (w // 2) // 64, (h // 2) // 16
    in_tile = (x // 64 == tx) & (y // 16 == ty)
    assert in_tile.any()
    last = in_tile & (y == y[in_tile].max())
    out.append(("(b) row %d of the 64 x 16 tile (%d, %d) is added twice (%d pixels)" % (y[in_tile].max(), tx, ty, last.sum()),
                as_result(exact + P[last].sum(axis=0), ex["n"])))
    # (c) J[2] of every pixel scaled by 1 + 2e-5
    t2 = dict(t); t2["J"] = t["J"].astype(np.float64).copy(); t2["J"][:, 2] *= 1 + 2e-5
    e2 = exact_sums(t2)
    out.append(("(c) J[2] of every pixel is scaled by 1 + 2e-5", dict(H=e2["H"], g=e2["g"], sum_r2=e2["sum_r2"], n_valid=ex["n"])))
    # (d) two entries of H exchanged: the first pair (row-major) closer than the old tolerance and further than twice both bounds
    bH = bounds(ex, DEPTH)[0]
    pair = None
    for i in range(21):
        for k in range(i + 1, 21):
            gap = abs(ex["H"][i] - ex["H"][k])
            if pair is None and gap < TOL_H_REL * np.abs(ex["H"]).max() and gap > 2 * bH[i] and gap > 2 * bH[k]:
                pair = (i, k)
    if pair is not None:
        Hs = ex["H"].copy(); Hs[[pair[0], pair[1]]] = Hs[[pair[1], pair[0]]]
        out.append(("(d) H%s and H%s are exchanged" % (UPPER[pair[0]], UPPER[pair[1]]), dict(H=Hs, g=ex["g"], sum_r2=ex["sum_r2"], n_valid=ex["n"])))
    # (e) g scaled by 1 + 1e-4
    out.append(("(e) g is scaled by 1 + 1e-4", dict(H=ex["H"], g=ex["g"] * (1 + 1e-4), sum_r2=ex["sum_r2"], n_valid=ex["n"])))
    return ex, out


def _visible(m, ex):
    """a mutation the bound cannot see is no test case: its change to at least one entry exceeds twice that entry's bound"""
    bH, bg, br = bounds(ex, DEPTH)
    return bool((np.abs(m["H"] - ex["H"]) > 2 * bH).any() or (np.abs(m["g"] - ex["g"]) > 2 * bg).any() or abs(m["sum_r2"] - ex["sum_r2"]) > 2 * br)


def test_mutations_are_rejected_by_the_bound_and_mostly_accepted_by_the_old_tolerance():
    """Every mutation is taken on level 3 of the 640x480 frame pair (reference 0, object 1) if that frame offers it.  If it does not
    (no visible case, or for (d) no pair of entries that close), the rule is: the first (level, reference, object) of util.frames()
    that does, by the same selection, levels from the finest down, then references, then objects in ascending order; the test
    prints which.  (d) needs this: no two of the 21 entries of H lie within 3e-5 * max|H| of each other on level 3 of any pair; the
    first level that offers such a pair is level 1 of reference frame 1, H(0,5) and H(1,4).)"""
    verdicts = {}
    order = [(l, i, j) for l in (3, 2, 1, 0) for i in range(4) for j in range(4) if i != j]
    assert order[0] == (3, 0, 1)
    for level, i_ref, i_obj in order:
        t = level_terms(level, i_ref, i_obj)
        ex, muts = _mutations(t)
        for name, m in muts:
            key = name[:3]
            if key in verdicts or not _visible(m, ex):
                continue
            assert _visible(m, ex)
            with pytest.raises(AssertionError):
                assert_gn_sums(m, t, DEPTH, name)
            old = old_lines_accept(m, ex)
            verdicts[key] = (old, (level, i_ref, i_obj))
            print("level %d of frames (%d, %d), %d terms: %s -- new bound: rejected; old tolerance: %s" % (
                level, i_ref, i_obj, ex["n"], name, "accepted" if old else "rejected"))
        if len(verdicts) == 5:
            break
    assert sorted(verdicts) == ["(a)", "(b)", "(c)", "(d)", "(e)"], sorted(verdicts)
    for key in ("(a)", "(b)", "(c)", "(e)"):
        assert verdicts[key][1] == (3, 0, 1), (key, verdicts[key])      # the 640x480 level-3 frame itself
    # the gap this bound closes: a lost pixel, a Jacobian column off by 2e-5 and two exchanged entries went through until now
    assert verdicts["(a)"][0] and verdicts["(c)"][0] and verdicts["(d)"][0], verdicts


@pytest.mark.parametrize("level", [0, 1, 2, 3])
def test_the_bound_implies_the_old_tolerance_on_the_suites_frames(level):
    """depth * 2^-24 * A <= 3e-5 * max|H| (for g: max|g|; for sum_r2: rtol 2e-5) for every entry, at the largest depth any kernel has
    (8 pixels per thread): the old lines stay in the tests, and this is why nobody needs to wonder which one binds."""
    depth = reduction_depth(8)
    for i_obj in (1, 2, 3):
        ex = exact_sums(level_terms(level, 0, i_obj))
        bH, bg, br = bounds(ex, depth)
        assert (bH <= TOL_H_REL * np.abs(ex["H"]).max()).all(), (level, i_obj, bH / np.abs(ex["H"]).max())
        assert (bg <= TOL_H_REL * np.abs(ex["g"]).max()).all(), (level, i_obj, bg / np.abs(ex["g"]).max())
        assert br <= 2e-5 * ex["sum_r2"]


def test_reduction_depth_is_what_design_section_6_derives():
    assert [reduction_depth(p) for p in (1, 2, 4, 8)] == [11, 13, 17, 25]
    assert [reduction_depth(p, "lds_patch") for p in (1, 2, 4, 8)] == [10, 11, 13, 17]
    assert reduction_depth() == reduction_depth(0) == reduction_depth(4)
    assert reduction_depth(8) * U32 * SECOND_ORDER < 1.5e-6      # "about one part in a million of an entry's own absolute sum"


def test_zero_terms_demand_exact_zeros_and_the_count_is_checked():
    t = level_terms(0)
    ex = exact_sums(t)
    good = dict(H=ex["H"], g=ex["g"], sum_r2=ex["sum_r2"], n_valid=ex["n"])
    before = gn_sums.nonempty_calls()
    assert assert_gn_sums(good, t, DEPTH, "exact") == 0.0
    assert gn_sums.nonempty_calls() == before + 1
    with pytest.raises(AssertionError):
        assert_gn_sums(dict(good, n_valid=ex["n"] + 1), t, DEPTH, "count")
    none = dict(index=np.zeros(0, np.int32), J=np.zeros((0, 6), np.float32), r=np.zeros(0, np.float32), rw=np.zeros(0, np.float32))
    zero = dict(H=np.zeros(21), g=np.zeros(6), sum_r2=0.0, n_valid=0)
    assert assert_gn_sums(zero, none, DEPTH, "empty") == 0.0
    assert gn_sums.nonempty_calls() == before + 1          # an empty term list does not count as a use of the helper
    with pytest.raises(AssertionError):
        assert_gn_sums(dict(zero, g=np.array([0, 0, 1e-30, 0, 0, 0])), none, DEPTH, "not zero")


# ---------------------------------------------------------------- assert_gn_sums_classes: terms that hold NaN / +-inf
def _class_case(where, value, level=1):
    import nonfinite_cases as nf
    _, o, t = nf.reference(where, value, "full", (96, 50), level)
    return dict(H=o["H"].copy(), g=o["g"].copy(), sum_r2=o["sum_r2"], n_valid=o["n_valid"]), t


@pytest.mark.parametrize("where,value", [("obj_gray", "nan"), ("obj_gray", "+inf"), ("ref_gray", "+inf"), ("ref_sigma", "nan")])
def test_classes_accept_the_oracle_and_reject_a_moved_entry_and_a_swapped_class(where, value):
    from gn_sums import assert_gn_sums_classes, per_entry_products, sum_class
    good, t = _class_case(where, value)
    depth = reduction_depth(1)
    before = gn_sums.nonempty_calls()
    # the oracle's own double sums: the finite entries far inside the bound, every other entry of the derived class
    assert assert_gn_sums_classes(good, t, depth, "oracle %s %s" % (where, value)) < 1e-6
    assert gn_sums.nonempty_calls() == before + 1
    with pytest.raises(AssertionError):      # assert_gn_sums itself keeps refusing such terms
        assert_gn_sums(good, t, depth, "refused")
    P = per_entry_products(t)
    cls = [sum_class(P[:, k]) for k in range(28)]
    assert "." != cls[27] or where == "ref_sigma"
    flat = lambda m: np.concatenate([m["H"], m["g"], [m["sum_r2"]]])
    unflat = lambda v: dict(H=v[:21].copy(), g=v[21:27].copy(), sum_r2=float(v[27]), n_valid=good["n_valid"])
    # (1) every finite entry in turn moved by twice its bound
    finite = [k for k in range(28) if cls[k] == "."]
    assert finite or where == "ref_gray"      # (+inf in the sampled image poisons all 28)
    for k in finite:
        v = flat(good)
        v[k] += 2 * depth * U32 * SECOND_ORDER * np.abs(P[:, k]).sum()
        with pytest.raises(AssertionError):
            assert_gn_sums_classes(unflat(v), t, depth, "moved")
    # (2) a finite entry turned NaN; (3) NaN <-> inf and +inf <-> -inf on every entry that is not finite
    for k in finite[:1]:
        v = flat(good); v[k] = np.nan
        with pytest.raises(AssertionError):
            assert_gn_sums_classes(unflat(v), t, depth, "finite -> NaN")
    swapped = 0
    for k in range(28):
        if cls[k] == ".":
            continue
        for other in {"n": (np.inf, -np.inf, 0.0), "+": (np.nan, -np.inf, 1e30), "-": (np.nan, np.inf, -1e30)}[cls[k]]:
            v = flat(good); v[k] = other
            with pytest.raises(AssertionError):
                assert_gn_sums_classes(unflat(v), t, depth, "swapped")
            swapped += 1
    assert swapped >= 3
    with pytest.raises(AssertionError):
        assert_gn_sums_classes(dict(good, n_valid=good["n_valid"] - 1), t, depth, "count")


def test_classes_on_finite_terms_are_the_plain_bound():
    from gn_sums import assert_gn_sums_classes
    t = level_terms(2)
    m = tree_model(t, 4)
    assert assert_gn_sums_classes(m, t, 13, "tree") == assert_gn_sums(m, t, 13, "tree")
    ex, muts = _mutations(t)
    for name, mut in muts:
        if _visible(mut, ex):
            with pytest.raises(AssertionError):
                assert_gn_sums_classes(mut, t, DEPTH, name)


def test_sum_class_is_order_independent():
    from gn_sums import sum_class
    inf = np.inf
    assert sum_class(np.array([1.0, inf, 2.0])) == "+" and sum_class(np.array([-inf, 1.0])) == "-"
    assert sum_class(np.array([inf, -inf])) == "n" and sum_class(np.array([1.0, np.nan, inf])) == "n"
    assert sum_class(np.zeros(0)) == "." and sum_class(np.array([1e30, -1e30])) == "."
    with np.errstate(invalid="ignore"):      # 0 * inf is NaN in float32 and in float64 alike
        assert np.isnan(np.float32(0) * np.float32(inf)) and np.isnan(0.0 * inf)
