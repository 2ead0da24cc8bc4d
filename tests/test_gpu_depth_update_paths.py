"""k_depth_update (dvo.mapper_update: dvo_op_depth_update, the host's age table and gray table) against orc.mapper_update on the
constructed inputs of tests/update_cases.py, bit for bit: depth, sigma, age and the valid-update count, NaN as the same class in the
same place.  tests/test_update_cases_oracle.py shows on the CPU, through the oracle's branch census, which of the kernel's own
branches each case reaches: the float / double / sqrt cascade of the loop test on both sides of each band, zero and NaN lengths,
failed warps, ages outside the history, the 102-step cap and the head's step-count buckets around it, the sample reuse (need_n, and
its `first` term alone), steps inside and outside the interior fast path, best matches outside the image, the D5 clamp, NaN at the
gate, both depthEstimate forms.

Every case runs with the mapping window of mapper.cpp:90 on, as the oracle has it, and off.  With the crop off the kernel also
visits the pixels left of x = 16 and above y = 12; their prior depth is NaN there, so that they leave at the warp (the maps of other
pixels are never read: the window's results cannot change) and the oracle's maps remain the reference, while the launch covers
another rectangle, the pixels fall into other workgroups and the counting sort sees other mixtures.
"""
import numpy as np
import pytest

import dvo_amd as dvo
import orc
import update_cases as uc

pytestmark = pytest.mark.gpu


def _run(c, depth, crop):
    return dvo.mapper_update(c["kf_gray"], c["kf_xi"], c["obj_gray"], c["obj_xi"], c["obj_rel"], c["obj_id"], c["K"], depth, c["sigma"],
                             c["age"], cfg=dvo.default_config(rng_seed=c["seed"], crop_enable=1 if crop else 0))


@pytest.mark.parametrize("crop", [True, False], ids=["crop", "nocrop"])
@pytest.mark.parametrize("name,form", uc.ALL, ids=["%s-%s" % nf for nf in uc.ALL])
def test_depth_update_case(name, form, crop):
    c, ref = uc.reference(name, form)
    depth, exp_d = c["depth"], ref["depth"]
    if not crop:
        yy, xx = np.mgrid[0:c["h"], 0:c["w"]]
        outside = (xx < 16) | (yy < 12)
        depth = np.where(outside, uc.NAN, depth).astype(np.float32)
        exp_d = np.where(outside, uc.NAN, exp_d).astype(np.float32)
    got_d, got_s, got_a, got_v = _run(c, depth, crop)
    np.testing.assert_array_equal(uc.bits(got_a), uc.bits(ref["age"]), err_msg="age")
    np.testing.assert_array_equal(uc.bits(got_d), uc.bits(exp_d), err_msg="depth")
    np.testing.assert_array_equal(uc.bits(got_s), uc.bits(ref["sigma"]), err_msg="sigma")
    assert got_v == ref["valid"]
    # the update was written wherever the census says the oracle wrote one, and nowhere else
    written = orc.census_mask(ref["flags"], "accepted") | orc.census_mask(ref["flags"], "rejected")
    assert got_v == int(orc.census_mask(ref["flags"], "accepted").sum())
    accepted = orc.census_mask(ref["flags"], "accepted")   # (a rejected update resets sigma to 0.5, which many priors already are)
    assert (uc.bits(got_d) != uc.bits(depth))[written].all() and (uc.bits(got_s) != uc.bits(c["sigma"]))[accepted].all()
    np.testing.assert_array_equal(uc.bits(got_d)[~written], uc.bits(depth)[~written])
    np.testing.assert_array_equal(uc.bits(got_s)[~written], uc.bits(c["sigma"])[~written])
    rejected = orc.census_mask(ref["flags"], "rejected")
    assert (got_a[rejected] == 0).all()
    np.testing.assert_array_equal(uc.bits(got_a)[~rejected], uc.bits(c["age"])[~rejected])


def test_sparse_and_full_K_agree_where_the_skew_is_zero():
    """depthEstimate's two forms on the SAME scene: a K whose zeros are exact takes the k_sparse form; the same K with its skew entry set
    to the smallest subnormal takes the full form -- 30 products, where the skew term adds 4.9e-324 times a coordinate to sums of
    order 1: the same doubles.  Both must give the oracle's bits (which has the full form only)."""
    c, ref = uc.reference("k_sparse", "mixed")
    K = c["K"].copy()
    K[0, 1] = np.float32(1e-45)
    assert K[0, 1] != 0
    c2 = dict(c, K=K)
    r2 = uc.run_oracle(c2, census=False)
    for k in ("depth", "sigma", "age"):
        np.testing.assert_array_equal(uc.bits(r2[k]), uc.bits(ref[k]))   # (the oracle: the skew changes nothing)
    got = _run(c2, c["depth"], True)
    for g, k in zip(got, ("depth", "sigma", "age")):
        np.testing.assert_array_equal(uc.bits(g), uc.bits(ref[k]), err_msg=k)
    assert got[3] == ref["valid"] >= 32
