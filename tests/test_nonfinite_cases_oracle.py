"""What the oracle makes of NaN and +-inf pixels (tests/nonfinite_cases.py, DESIGN.md §6 "Non-finite pixels"), on the oracle alone.
No GPU.  tests/test_gpu_nonfinite_pixels.py holds the kernels to the same cases; this file pins that every case is of the class it
is listed under and exercises what it claims to."""
import numpy as np
import pytest

import gn_sums
import nonfinite_cases as nf
import orc

GRID = [(size, placement, level) for size in nf.BIG for placement in nf.PLACEMENTS for level in nf.LEVELS] + \
       [(nf.SIZES[2], "full", level) for level in (0, 1)]      # (5 x 7 at level 2: the crop leaves no pixel)


def _terms_finite(t):
    return bool(np.isfinite(t["J"]).all() and np.isfinite(t["r"]).all() and np.isfinite(t["rw"]).all())


def _derived(t):
    P = gn_sums.per_entry_products(t)
    return "".join(gn_sums.sum_class(P[:, k]) for k in range(28))


@pytest.mark.parametrize("where,value", nf.CASES)
def test_every_case_is_of_its_class_and_exercises_what_it_claims(where, value):
    for size, placement, level in GRID:
        tag = (where, value, size, placement, level)
        c, o, t = nf.reference(where, value, placement, size, level)
        _, clean, _ = nf.reference(where, None, placement, size, level)
        mark = c["mark"]; mask = o["mask"].astype(bool)
        np.testing.assert_array_equal(t["index"], np.flatnonzero(mask.ravel()))
        assert o["n_valid"] == t["n_valid"] == int(mask.sum()), tag
        hit = int((mask & mark).sum())
        big = size in nf.BIG
        if big:
            assert mark.sum() >= 50, tag
            # (the level-2 crop keeps x in [20, 140], y in [20, 100]: 2143 and 1027 pixels of the clean pairs)
            assert o["n_valid"] >= (1000 if level < 2 else 800), (tag, o["n_valid"])
        # the class of the oracle's own sums is the class of the exact sum of its terms, entry by entry
        got = nf.classes(o["H"]) + nf.classes(o["g"]) + nf.classes([o["sum_r2"]])
        assert got == _derived(t), tag
        if (where, value) in nf.FINITE:
            assert _terms_finite(t), tag
            assert got == "." * 28 and np.isfinite(o["xi_update"]).all() and np.isfinite(o["residual"]), tag
            if nf.FINITE[(where, value)] == "gated":
                assert hit == 0, tag
                # nothing else changes: the mask is the clean pair's without the marked pixels
                np.testing.assert_array_equal(mask, clean["mask"].astype(bool) & ~mark)
            elif big and level < 2:
                # marked pixels contribute, with what the fill quirk of getSubpixel / the clamp of optimize.cpp:83 makes of them
                assert hit >= (100 if placement == "full" else 50), (tag, hit)
            continue
        assert not _terms_finite(t), tag
        if big:
            want = nf.POISON[(where, value)]
            assert nf.classes(o["H"]) == want["H"] and nf.classes(o["g"]) == want["g"], tag
            assert nf.classes([o["sum_r2"]]) == want["sum_r2"] and nf.classes(o["xi_update"]) == want["xi_update"], tag
        assert hit > 0 or where == "ref_gray", tag
        if where != "ref_gray":
            assert o["n_valid"] == clean["n_valid"], tag      # the marked pixels pass every gate
        else:
            assert o["n_valid"] < clean["n_valid"] and not o["xi_update"].any(), tag    # -inf gradients are is_invalid; the update is exactly zero
        res = np.float32(o["sum_r2"]) / np.float32(o["n_valid"])
        assert nf.classes([o["residual"]]) == nf.classes([res]), tag
        if where == "ref_sigma":
            assert o["residual"] == clean["residual"], tag    # r does not see sigma: the clean residual bit for bit


def test_the_clean_pair_is_the_documented_one():
    _, o, _ = nf.reference("obj_gray", None, "sprinkle", (96, 50), 1)
    assert o["n_valid"] == 4643
    c, o, _ = nf.reference("ref_gray", "nan", "full", (96, 50), 1)
    assert (int(c["mark"].sum()), int((o["mask"].astype(bool) & c["mark"]).sum()), o["n_valid"]) == (197, 150, 4583)
    _, o, _ = nf.reference("ref_depth", "+inf", "full", (96, 50), 1)
    assert o["n_valid"] == 4451
    _, o, _ = nf.reference("ref_gray", "+inf", "sprinkle", (96, 50), 1)
    assert o["n_valid"] == 4025
    _, o, _ = nf.reference("ref_sigma", "nan", "sprinkle", (96, 50), 1)
    np.testing.assert_allclose(o["residual"], 0.0041137, rtol=1e-4)


def test_nan_is_neither_valid_nor_invalid():
    """getPixel (is_valid) turns a NaN into INVALID, so a cull does; the per-pixel gate (is_invalid) lets it through"""
    img = np.full((8, 8), 0.5, np.float32)
    img[2, 2] = np.nan; img[2, 4] = -np.inf; img[4, 2] = np.inf
    out = orc.cull_image(img, 1)
    assert out[1, 1] == orc.INVALID and out[1, 2] == orc.INVALID and out[2, 1] == np.inf
    assert np.isnan(orc.cull_image(img, 0)[2, 2])       # no cull: a copy


@pytest.mark.parametrize("where,value", nf.TRACK_CASES)
def test_track_with_one_marked_pixel(where, value):
    """128 x 96, 3 levels, culls = 0: only the finest level holds the pixel."""
    obj, ref = nf.oracle_frames(nf.build_track(where, value))
    xi, lg = orc.track(obj, ref)
    cobj, cref = nf.oracle_frames(nf.build_track(where, None))
    _, clean = orc.track(cobj, cref)
    for l in (0, 1):      # the coarser levels never see the pixel
        assert lg["n_iter"][l] == clean["n_iter"][l]
        np.testing.assert_array_equal(lg["xi_after"][l], clean["xi_after"][l])
    before = lg["xi_after"][1][-1]
    if (where, value) in nf.REFUSED:
        assert lg["n_iter"][2] == orc.MAX_ITER == 15
        assert (lg["n_valid"][2] == 7922).all()
        for it in range(15):      # every update is refused: the twist never moves
            np.testing.assert_array_equal(lg["xi_after"][2][it].view(np.uint32), before.view(np.uint32))
        np.testing.assert_array_equal(xi.view(np.uint32), before.view(np.uint32))
        want = {"nan": "n", "+inf": "+"}[value] if where == "obj_gray" else "."
        assert nf.classes(lg["residual"][2]) == want * 15
        assert np.isnan(lg["upd_norm"][2]).all()
        if where == "ref_sigma":
            assert (lg["residual"][2] == clean["residual"][2][0]).all()      # the clean finite residual, repeated
    elif (where, value) == ("ref_gray", "+inf"):
        # a zero update: the norm test fires, "converged" with an infinite residual
        assert lg["n_iter"][2] == 1 and lg["residual"][2][0] == np.inf and lg["upd_norm"][2][0] == 0.0
        np.testing.assert_array_equal(xi.view(np.uint32), before.view(np.uint32))
    else:
        assert np.isfinite(xi).all() and np.isfinite(lg["residual"][2]).all() and lg["n_iter"][2] > 1      # an ordinary finite track
        assert not np.array_equal(xi, before)


def test_where_the_devices_solve_leaves_the_oracle():
    """DESIGN.md section 3, D13.  Many +inf pixels in the sampled image leave NaN in every diagonal sum of H: no diagonal entry is > 0
    and both solves return zero without a pseudo-inverse.  ONE such pixel leaves +inf on the diagonal: orc_solve6 goes through the
    pseudo-inverse, drops every NaN eigenvalue and answers zero; the device answers NaN (tests/test_gpu_nonfinite_pixels.py)."""
    for size in nf.BIG:
        for level in nf.LEVELS:
            for placement in nf.PLACEMENTS:
                _, o, t = nf.reference("ref_gray", "+inf", placement, size, level)
                assert nf.device_update_class(t) == "oracle" and nf.classes(o["H"][list(nf.DIAGONAL)]) == "n" * 6, (size, level, placement)
            c, o, t = nf.reference("ref_gray", "+inf", "single", size, level)
            assert c["mark"].sum() == 1 and o["n_valid"] > 800
            if level < 2:      # (at level 2 the step is smaller and the pose's taps may miss the pixel: whatever the rule derives)
                assert nf.device_update_class(t) == "nan" and "+" in nf.classes(o["H"][list(nf.DIAGONAL)]), (size, level)
                assert o["residual"] == np.inf
            if nf.device_update_class(t) == "nan":
                assert not o["xi_update"].any(), (size, level)
            for where, value in (("obj_gray", "nan"), ("obj_gray", "+inf"), ("ref_sigma", "nan")):      # H finite: never D13
                assert nf.device_update_class(nf.reference(where, value, "full", size, level)[2]) == "oracle"
    c = nf.build_track("ref_gray", "+inf")
    obj, ref = nf.oracle_frames(c)
    _, lg = orc.track(obj, ref)
    t = orc.optimize_terms(obj.gray(2), ref.gray(2), ref.depth(2), ref.sigma(2), ref.K(2), lg["xi_after"][1][-1], 2)
    assert nf.device_update_class(t) == "nan" and not orc.solve6(t["H"], t["g"]).any()      # the finest level's first iteration
