"""The mapping update as a MONO BATCH runs it (dvo_op_depth_update_batch: MonoBatch::queue_depth_update -- k_age_table over the keyframe
ring with n_hist = -1, then k_depth_update with ring_gray, meta and clamp_age = 1, or k_depth_update_cam with the batch's own
per-sequence tables) against orc.mapper_update, bit for bit, on five sequences that each carry a DIFFERENT constructed case of
tests/update_cases.py (mixed form), so that a wrong sequence index, ring slot or camera shows.

Ring of 3 with 1, 7, 3, 4 and 4 keyframes created: the ring is not full, full, and has wrapped (4: the oldest retained keyframe sits
in slot 1; 7: in slot 1 too, after two rounds).  Every keyframe has a gray of its own.  One sequence has need = 1: its maps must come
back untouched.  The reference of a sequence is orc.mapper_update on its retained keyframes with age' = min(age, n_hist - 1): a pixel
whose age points past the ring is searched against the oldest retained keyframe (include/dvo.h, dvo_mono_stats::clamped_pixels), keeps
its age unless the update resets it, and is counted -- `clamped` must equal the census's count of bi < 0 on the ages as given.
"""
import numpy as np
import pytest

import dvo_amd as dvo
import orc
import update_cases as uc

pytestmark = pytest.mark.gpu

R, FW, FH = 3, 4 * uc.W, 4 * uc.H
# (case, keyframes created so far, need)
SEQS = [("dband_go_diag", 1, 0), ("age_beyond", 7, 0), ("kf_twist_nan", 3, 0), ("depth_negative", 4, 0), ("invalid_blobs", 4, 1)]
# five cameras at map level, the skewed (depthEstimate's full-K form) and the anisotropic one among them
CAMS = [uc.K64, uc.K_SKEW, uc.K_ANISO, np.array([[60, 0, 31], [0, 60, 23.5], [0, 0, 1]], np.float32),
        np.array([[66, 0, 33.5], [0, 62, 24.5], [0, 0, 1]], np.float32)]
PAD_XI = ([-0.125, 0.0625, 0, 0, 0, 0], [0.1875, -0.125, 0, 0, 0, 0])


def full_res(K):
    Kf = np.asarray(K, np.float32) * np.float32(4)
    Kf[2, 2] = 1
    return Kf


def build_seq(q, K=None):
    """sequence q: its case with older keyframes (grays and poses of their own) put in front up to min(n_total, R), frame id 4 + q"""
    name, n_total, need = SEQS[q]
    c = dict(uc.case(name, "mixed"))
    n_hist = min(n_total, R)
    yy, xx = np.mgrid[0:uc.H, 0:uc.W]
    pad = n_hist - len(c["kf_gray"])
    assert pad >= 0
    c["kf_gray"] = [uc.texture(xx + 3.3 * (i + 1) + q, yy - 1.7 * (i + 1)) for i in range(pad)] + list(c["kf_gray"])
    c["kf_xi"] = [np.asarray(PAD_XI[i], np.float32) for i in range(pad)] + list(c["kf_xi"])
    c["obj_id"] = 4 + q
    if K is not None:
        c["K"] = np.asarray(K, np.float32)
    c.update(n_total=n_total, n_hist=n_hist, need=need)
    return c


def expected(c):
    """the oracle on the retained keyframes under the ring's contract: (depth, sigma, age, valid, clamped)"""
    if c["need"]:
        return c["depth"], c["sigma"], c["age"], 0, 0
    clamped = uc.run_oracle(c)["counts"]["age_beyond"]                      # bi < 0 on the ages as given
    r = uc.run_oracle(c, age=np.minimum(c["age"], np.float32(c["n_hist"] - 1)))
    assert r["counts"]["age_beyond"] == 0
    age = np.where(orc.census_mask(r["flags"], "rejected"), np.float32(0), c["age"])   # (a reset clears the age; nothing else changes it)
    return r["depth"], r["sigma"], age, r["valid"], clamped


def run_op(seqs, K):
    n = len(seqs)
    kg = np.full((n, R, uc.H, uc.W), np.nan, np.float32); kx = np.zeros((n, R, 6), np.float32)
    for q, c in enumerate(seqs):
        for i in range(c["n_hist"]):
            kg[q, i] = c["kf_gray"][i]; kx[q, i] = c["kf_xi"][i]
    st = lambda k: np.stack([c[k] for c in seqs])
    return dvo.op_depth_update_batch(FW, FH, R, K, [c["n_total"] for c in seqs], kg, kx, st("obj_gray"), st("obj_xi"), st("obj_rel"),
                                     [c["need"] for c in seqs], [c["obj_id"] for c in seqs], st("depth"), st("sigma"), st("age"),
                                     cfg=dvo.default_config(rng_seed=7))


def check(got, q, exp, what):
    for g, e, k in zip(got[:3], exp[:3], ("depth", "sigma", "age")):
        np.testing.assert_array_equal(uc.bits(g[q]), uc.bits(e), err_msg="%s: sequence %d %s" % (what, q, k))
    assert (int(got[3][q]), int(got[4][q])) == (exp[3], exp[4]), (what, q, int(got[3][q]), int(got[4][q]), exp[3], exp[4])


@pytest.mark.parametrize("cams", [False, True], ids=["shared_K", "per_sequence_K"])
def test_batch_update_matches_the_oracle_per_sequence(cams):
    seqs = [build_seq(q, CAMS[q] if cams else None) for q in range(len(SEQS))]
    K = np.stack([full_res(c["K"]) for c in seqs]) if cams else full_res(uc.K64)
    got = run_op(seqs, K)
    exps = [expected(c) for c in seqs]
    for q, c in enumerate(seqs):
        check(got, q, exps[q], "batch of 5")
    # the cases did what they are there for: the aged-out pixels were clamped, searched and some of them written; every running sequence
    # wrote updates; the sequence that creates a keyframe is untouched (checked bit for bit above) and counted nothing
    assert exps[1][4] >= 32 and exps[1][3] >= 32
    beyond = seqs[1]["age"] > R - 1
    assert (uc.bits(got[0][1]) != uc.bits(seqs[1]["depth"]))[beyond].sum() >= 8
    assert all(e[3] >= 32 for e in exps[:4]) and exps[4][3:] == (0, 0)
    assert [int(x) for x in got[4]] == [0, exps[1][4], 0, 0, 0]
    # ... and every sequence alone, through the same operator, gives the same bits
    for q, c in enumerate(seqs):
        one = run_op([c], K[q:q + 1] if cams else K)
        for a, b, k in zip(one[:3], got[:3], ("depth", "sigma", "age")):
            np.testing.assert_array_equal(uc.bits(a[0]), uc.bits(b[q]), err_msg="alone: sequence %d %s" % (q, k))
        assert (int(one[3][0]), int(one[4][0])) == (int(got[3][q]), int(got[4][q]))


def test_ring_slots_follow_the_number_of_keyframes_created():
    """the same three retained keyframes with 3, 4, 5 and 6 keyframes created (oldest retained in slot 0, 1, 2, 0): the same results"""
    base = build_seq(1)
    seqs = [dict(base, n_total=n) for n in (3, 4, 5, 6)]
    got = run_op(seqs, full_res(uc.K64))
    exp = expected(base)
    for q in range(4):
        check(got, q, exp, "n_total %d" % seqs[q]["n_total"])
