"""CPU: the constructed inputs of tests/update_cases.py reach the branches they are built for, shown by the oracle's branch census
(orc.mapper_update_census: k_depth_update's own predicates, restated literally in oracle/dvo_oracle.c, evaluated on the oracle's
values -- the kernel's coordinates are the oracle's bit for bit by the parity contract).  The GPU tests
(tests/test_gpu_depth_update_paths.py, tests/test_gpu_depth_update_batch.py) then hold the kernel to the oracle on these inputs.

Minimums, as conditions on the inputs: every class a case names counts at least 32 pixels (steps, or loop tests, for the classes
counted in those) in the case's uniform form and at least 1 in its mixed form, where at least 32 ordinary pixels -- searched and in
none of the case's classes -- of at least three different step counts sit beside them.

One exception: first_origin -- the first step's pt - dir is exactly (0, 0), the initial value of the kernel's previous centre, so that
need_n holds through its `first` term alone -- needs a segment that starts at exactly (0, 0): two window pixels of one scene can
(update_cases._first_at_origin), not 32.  Its minimum is update_cases.FEW.  No class is declared unreachable: the double band with go
true is reached by dband_go_diag (1 125 pixels), NaN at the gate of mapper.cpp:122 by depth_negative, the D5 clamp by border_bottom.
obj_twist_nan and obj_twist_inf have the uniform form only: a frame's twist belongs to the whole frame.
"""
import numpy as np
import pytest

import orc
import update_cases as uc

# every class of the census that some case must reach
MANDATORY = ("test_float", "test_double", "test_sqrt", "fband_go", "fband_stop", "dband_go", "dband_stop", "length_not_pos", "warp_fails", "age_beyond",
             "age_negative", "gate_nd_ge6", "d5_clamp", "gate_nan", "cap", "need_n", "step_not_inner", "ssd_reject", "best_outside",
             "grad_invalid", "accepted", "rejected", "head_103", "first_origin")


def _in_classes(flags, classes):
    m = np.zeros(flags.shape, bool)
    for k in classes:
        m |= orc.census_mask(flags, k)
    return m


@pytest.mark.parametrize("name", list(uc.NAMES))
def test_case_reaches_its_classes(name):
    forms, classes = uc.NAMES[name]
    for form in forms:
        c, r = uc.reference(name, form)
        counts = r["counts"]
        print(name, form, {k: v for k, v in counts.items() if v})
        assert counts["shortcut_differs"] == 0 and counts["head_short"] == 0, counts
        for k in classes:
            need = uc.FEW.get(k, 32) if form == "uniform" else 1
            assert counts[k] >= need, (name, form, k, counts[k])
        if form == "mixed":
            ordinary = (r["steps"] >= 0) & ~_in_classes(r["flags"], [k for k in classes if k != "test_float"])   # (every search has float-decided tests)
            assert ordinary.sum() >= 32, (name, int(ordinary.sum()))
            assert len(set(r["steps"][ordinary].tolist())) >= 3, (name, sorted(set(r["steps"][ordinary].tolist())))


def test_every_mandatory_class_has_a_case():
    named = {k for _, classes in uc.NAMES.values() for k in classes}
    assert set(MANDATORY) - named == set(), set(MANDATORY) - named
    assert set(MANDATORY) | {"searched", "steps", "longest", "head_short", "shortcut_differs", "out_of_frame"} == set(orc.CENSUS)


def test_loop_test_bands_are_reached_on_both_sides():
    """over the union of the cases: both outcomes of the float band and both outcomes of the double band"""
    tot = {k: 0 for k in orc.CENSUS}
    for name, form in uc.ALL:
        for k, v in uc.reference(name, form)[1]["counts"].items():
            tot[k] += v
    print(tot)
    assert tot["fband_go"] >= 32 and tot["fband_stop"] >= 32 and tot["dband_go"] >= 32 and tot["dband_stop"] >= 32
    assert tot["test_double"] >= 32 and tot["test_sqrt"] >= 32
    assert tot["shortcut_differs"] == 0 and tot["head_short"] == 0


def test_step_counts_on_both_sides_of_the_cap():
    """near_cap: searches of exactly 100, 101 and 102 steps (the last both with and without the cap's break) and heads of 101, 102 and 103"""
    c, r = uc.reference("near_cap", "uniform")
    steps = set(r["steps"][r["steps"] >= 0].tolist())
    assert {100, 101, 102} <= steps, sorted(steps)
    capped = orc.census_mask(r["flags"], "cap")
    assert (capped & (r["steps"] == 102)).any() and (~capped & (r["steps"] == 101)).any()
    h103 = orc.census_mask(r["flags"], "head_103")
    assert (capped & ~h103).sum() >= 1   # length in (101, 102): the cap's break below head bucket 103
    assert r["counts"]["longest"] == 102


def test_census_changes_no_result():
    """orc.mapper_update and orc.mapper_update_census leave the same maps and return the same count: one sweep case, one constructed"""
    outs = []
    for census in (False, True):
        kfs, obj, _, _, _ = uc.sweep_inputs(*uc.SWEEP[7])
        v = orc.mapper_update_census(kfs, obj, 17)[0] if census else orc.mapper_update(kfs, obj, 17)
        outs.append((v, kfs[2].depth(2), kfs[2].sigma(2), kfs[2].age()))
    assert outs[0][0] == outs[1][0] and outs[0][0] > 100
    for a, b in zip(outs[0][1:], outs[1][1:]):
        np.testing.assert_array_equal(uc.bits(a), uc.bits(b))
    c = uc.case("depth_negative", "mixed")
    a, b = uc.run_oracle(c, census=False), uc.run_oracle(c, census=True)
    assert a["valid"] == b["valid"]
    for k in ("depth", "sigma", "age"):
        np.testing.assert_array_equal(uc.bits(a[k]), uc.bits(b[k]))


def test_oracle_leaves_the_inputs_of_a_case_alone():
    c = uc.case("exact_x", "mixed")
    keep = {k: np.copy(c[k]) for k in ("depth", "sigma", "age")}
    r = uc.run_oracle(c)
    for k in keep:
        np.testing.assert_array_equal(uc.bits(keep[k]), uc.bits(c[k]))
    written = orc.census_mask(r["flags"], "accepted") | orc.census_mask(r["flags"], "rejected")
    assert written.sum() >= 32 and (uc.bits(r["depth"]) != uc.bits(c["depth"]))[written].all()
    np.testing.assert_array_equal(uc.bits(r["depth"])[~written], uc.bits(c["depth"])[~written])


# what the natural-input sweep of tests/test_gpu_parity.py reaches today: {seed: census}, pinned so that an edit of those inputs cannot
# lose a branch silently.  (All eight cases together: 76 371 searched pixels, 1 548 854 steps; 15 loop tests in the float band, none in
# the double band; no non-finite geometry, no age outside the history.)
def test_sweep_keeps_its_coverage():
    tot = {k: 0 for k in orc.CENSUS}
    for p in uc.SWEEP:
        kfs, obj, _, _, _ = uc.sweep_inputs(*p)
        _, c, _, _ = orc.mapper_update_census(kfs, obj, p[0])
        print(p[0], {k: v for k, v in c.items() if v})
        assert (c["cap"] > 0) == (p[0] in (6, 9, 11, 17)), (p[0], c["cap"])
        assert c["need_n"] > 0 and c["accepted"] > 0 and c["rejected"] > 0 and c["step_not_inner"] > 0, (p[0], c)
        assert c["steps"] - c["step_not_inner"] > 0   # the interior fast path's steps
        assert c["shortcut_differs"] == 0 and c["head_short"] == 0
        for k, v in c.items():
            tot[k] = max(tot[k], v) if k == "longest" else tot[k] + v
    assert tot["searched"] == 76371 and tot["steps"] == 1548854, tot
    assert tot["cap"] == 3650 and tot["need_n"] == 22876 and tot["accepted"] == 4625 and tot["rejected"] == 2364, tot
    # the gaps the constructed cases close: if the sweep ever reaches one of these, good -- update the record in DESIGN.md
    assert tot["test_double"] == 15 and tot["test_sqrt"] == 0
    for k in ("length_not_pos", "warp_fails", "age_beyond", "age_negative", "gate_nd_ge6", "gate_nan", "first_origin"):
        assert tot[k] == 0, (k, tot[k])

