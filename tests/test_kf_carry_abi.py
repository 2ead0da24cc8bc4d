"""CPU tests of the keyframe carry (include/dvo.h, dvo_batch_set_keyframe_carry): the entry points are declared, exported
and bound, NULL and bad arguments are refused before anything touches the GPU, the header states the contract, the C++ facade compiles,
the replica (tests/kf_carry_ref.py) keeps its anchors, and the new kernels need no scratch and no LDS and stay within the VGPRs measured
when they were written (k_kf_carry 31, k_kf_carry_cam 31, k_kf_carry_prep 60, k_kf_carry_commit 8) plus one allocation unit of 8."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import dvo_amd as dvo
import kf_carry_ref as cref
import kf_fusion_ref as kref
from kf_common import assert_map_kernels_fit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("dvo_kf_carry_config_default", "dvo_batch_set_keyframe_carry", "dvo_batch_last_keyframe_carry")
F32 = np.float32
KC_ON, KC_OFF = dvo.KF_CARRY_ON, dvo.KF_CARRY_OFF   # (without the feature the file fails here, at import)


def _header():
    return open(os.path.join(ROOT, "include", "dvo.h")).read()


def test_declared_exported_and_listed():
    txt = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert re.search(r"#define\s+DVO_KF_CARRY_OFF\s+0\b", txt) and re.search(r"#define\s+DVO_KF_CARRY_ON\s+1\b", txt)
    assert re.search(r"typedef\s+struct\s+dvo_kf_carry_config\s*\{\s*int\s+struct_size;\s*int\s+mode;\s*float\s+max_diff;\s*\}", txt)
    assert re.search(r"typedef\s+struct\s+dvo_kf_carry_record\s*\{\s*int\s+struct_size,\s*n_candidates,\s*n_carried,\s*n_gated;\s*\}", txt)
    assert re.search(r"\bvoid\s+dvo_kf_carry_config_default\s*\(\s*dvo_kf_carry_config\s*\*", txt)
    assert re.search(r"\bint\s+dvo_batch_set_keyframe_carry\s*\(\s*dvo_batch\s*\*\s*\w+\s*,\s*const\s+dvo_kf_carry_config\s*\*", txt)
    assert re.search(r"\bint\s+dvo_batch_last_keyframe_carry\s*\(\s*dvo_batch\s*\*\s*\w+\s*,\s*dvo_kf_carry_record\s*\*", txt)
    for n in NAMES:
        assert hasattr(dvo.lib(), n), n
        assert n in dvo.EXPORTS, n


def test_the_header_states_the_contract():
    txt = " ".join(_header().split())
    for phrase in ("BEFORE the tracked frame is copied over", "d >= min_depth and d < inf", "transform(Bk, ...) -> (Xk, Yk, Zk)",
                   "OLD keyframe's top-level depth", "fabsf(zi - Zk) <= max_diff", "d_prior = its z",
                   "c_prior = the minimum of the four taps' counts", "(float)(c_prior + 1) * (1.0f / (float)(c_prior + 2))",
                   "fmaf(d_prior - d, r, d)", "min(c_prior + 1, max_count)", "keeps d and gets count 0", "n_carried",
                   "dvo_batch_frame_get returns the carried", "turning fusion off turns the carry off",
                   "leaves maps and counts as they are"):
        assert phrase in txt, phrase


def test_default_config_and_struct_sizes():
    c = dvo.KfCarryConfig(0, 0.0, struct_size=0)
    dvo.lib().dvo_kf_carry_config_default(C.byref(c))
    assert (c.struct_size, c.mode) == (12, dvo.KF_CARRY_ON) and F32(c.max_diff) == F32(0.05)
    dvo.lib().dvo_kf_carry_config_default(None)
    assert C.sizeof(dvo.KfCarryConfig) == 12 and C.sizeof(dvo.KfCarryRecord) == 16
    assert dvo.KF_CARRY_RECORD_DTYPE.itemsize == 16
    assert (dvo.KF_CARRY_OFF, dvo.KF_CARRY_ON) == (0, 1)
    d = dvo.KfCarryConfig()
    assert (d.struct_size, d.mode) == (12, 1) and F32(d.max_diff) == F32(0.05)


def test_the_batch_binds_it():
    for m in ("set_keyframe_carry", "last_keyframe_carry"):
        assert callable(getattr(dvo.Batch, m, None)), m
        assert not hasattr(dvo.MonoBatch, m), m


def test_null_arguments_are_refused():
    L = dvo.lib()
    c = dvo.KfCarryConfig()
    rec = (dvo.KfCarryRecord * 1)()
    assert L.dvo_batch_set_keyframe_carry(None, C.byref(c)) == dvo.DVO_ERR_BAD_ARGUMENT
    assert L.dvo_batch_set_keyframe_carry(None, None) == dvo.DVO_ERR_BAD_ARGUMENT
    assert L.dvo_batch_last_keyframe_carry(None, rec) == dvo.DVO_ERR_BAD_ARGUMENT
    assert L.dvo_batch_last_keyframe_carry(None, None) == dvo.DVO_ERR_BAD_ARGUMENT


def test_facade_compiles(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("g++ not available")
    src = tmp_path / "snippet.cpp"
    src.write_text(r"""
#include "dvo.hpp"
#include <vector>
int use()
{
    const dvo::Mat3 K{525.f, 0.f, 319.5f, 0.f, 525.f, 239.5f, 0.f, 0.f, 1.f};
    dvo::BatchTracker bt(4, K, 640, 480);
    bt.setKeyframeTracking();
    bt.setKeyframeFusion();
    bt.setKeyframeCarry();
    bt.setKeyframeCarry(DVO_KF_CARRY_ON, 0.03f);
    bt.setKeyframeCarry(DVO_KF_CARRY_OFF);
    std::vector<dvo_kf_carry_record> r = bt.lastKeyframeCarry();
    return (int)r.size() + r[0].n_carried + r[0].n_candidates + r[0].n_gated;
}
""")
    r = subprocess.run([gxx, "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


# ---- the replica's anchors ------------------------------------------------------------------------------------------------------
K_TOP = np.array([[262.5, 0, 79.75], [0, 262.5, 59.75], [0, 0, 1]], F32)
EYE = np.eye(4, dtype=F32)
MIN_DEPTH = 0.2


def _scene(h=31, w=43, seed=0):
    rng = np.random.RandomState(seed)
    ys, xs = np.mgrid[0:h, 0:w]
    top = (1.5 + 0.01 * xs + 0.005 * ys + rng.normal(0, 0.001, (h, w))).astype(F32)
    return [kref.cull(top, 2), kref.cull(top, 1), top]


def _exact(top):
    """pixels that project onto themselves under the identity (a = b = 0) and have all four taps inside"""
    h, w = top.shape
    k = kref.intr(K_TOP)
    ys, xs = np.mgrid[0:h, 0:w]
    u, v = kref.project(k, *kref.back_project(k, xs.astype(F32), ys.astype(F32), top))
    return (u == xs) & (v == ys) & (xs < w - 1) & (ys < h - 1)


def _min4(c):
    m = c.astype(np.int64).copy()
    m[:-1, :-1] = np.minimum(np.minimum(c[:-1, :-1], c[:-1, 1:]), np.minimum(c[1:, :-1], c[1:, 1:]))
    return m


def test_identity_with_equal_maps_keeps_depth_and_raises_counts():
    """F = Bk = I and the old keyframe equal to the frame: wherever a pixel projects onto itself zi = d and d_prior - d = 0, so d_new == d
    bit for bit, and c_new = min(c_prior + 1, max_count) with c_prior the minimum of the four taps' counts."""
    levels = _scene()
    h, w = levels[-1].shape
    counts = np.random.RandomState(1).randint(0, 9, (h, w)).astype(np.uint8)
    new, cnt, rec = cref.carry(levels, levels[-1], counts, K_TOP, EYE, EYE, MIN_DEPTH, 0.05, 6)
    ex = _exact(levels[-1])
    assert ex.sum() > 100 and rec["n_candidates"] == h * w and rec["n_gated"] == 0
    assert rec["n_carried"] == int((cnt > 0).sum()) and rec["n_carried"] > (h - 2) * (w - 2) // 2
    assert new[-1][ex].tobytes() == levels[-1][ex].tobytes()
    want = np.minimum(_min4(counts) + 1, 6)
    assert (cnt[ex] == want[ex]).all()
    assert (cnt[ex] == 6).any() and (cnt[ex] == 1).any()          # saturation, and c_prior = 0 through one zero tap
    assert (_min4(counts)[ex] < counts[ex]).any()                  # the minimum, not the pixel's own tap
    assert np.abs(new[-1] - levels[-1]).max() <= 0.012
    k = kref.intr(K_TOP)
    ys, xs = np.mgrid[0:h, 0:w]
    u, v = kref.project(k, *kref.back_project(k, xs.astype(F32), ys.astype(F32), levels[-1]))
    out = (u >= F32(w - 1)) | (v >= F32(h - 1))
    assert out.sum() > 10 and (cnt[out] == 0).all()                # u = w - 1 exactly is outside
    assert new[-1][out].tobytes() == levels[-1][out].tobytes()


def test_zero_counts_give_one_half_and_higher_counts_their_share():
    levels = _scene()
    h, w = levels[-1].shape
    old = (levels[-1] - F32(0.03)).astype(F32)
    ex = _exact(levels[-1])
    for c0 in (0, 1, 5):
        counts = np.full((h, w), c0, np.uint8)
        new, cnt, rec = cref.carry(levels, old, counts, K_TOP, EYE, EYE, MIN_DEPTH, 0.05, 16)
        r = F32(F32(c0 + 1) * (F32(1) / F32(c0 + 2)))
        if c0 == 0:
            assert r == F32(0.5)
        want = kref.rr.fmaf((old - levels[-1]).astype(F32), np.full_like(old, r), levels[-1])
        assert new[-1][ex].tobytes() == want[ex].tobytes()
        assert (cnt[ex] == c0 + 1).all()


def test_max_count_saturates():
    levels = _scene()
    h, w = levels[-1].shape
    ex = _exact(levels[-1])
    for c0, mc, want in ((1, 2, 2), (2, 2, 2), (200, 2, 2), (254, 255, 255), (255, 255, 255)):
        _, cnt, _ = cref.carry(levels, levels[-1], np.full((h, w), c0, np.uint8), K_TOP, EYE, EYE, MIN_DEPTH, 0.05, mc)
        assert (cnt[ex] == want).all(), (c0, mc)


@pytest.mark.parametrize("bad", [np.nan, np.inf, 0.0, 0.1])
def test_bad_pixels_and_taps_change_nothing(bad):
    levels = _scene()
    h, w = levels[-1].shape
    counts = np.full((h, w), 3, np.uint8)
    fr = [l.copy() for l in levels]
    fr[-1][10:14, 10:14] = bad                     # the frame's own pixels
    new, cnt, rec = cref.carry(fr, levels[-1], counts, K_TOP, EYE, EYE, MIN_DEPTH, 0.05, 16)
    assert new[-1][10:14, 10:14].tobytes() == fr[-1][10:14, 10:14].tobytes() and (cnt[10:14, 10:14] == 0).all()
    assert rec["n_candidates"] == h * w - 16
    old = levels[-1].copy()
    old[20:24, 20:24] = bad                        # the old keyframe's taps
    new, cnt, rec = cref.carry(levels, old, counts, K_TOP, EYE, EYE, MIN_DEPTH, 0.05, 16)
    assert new[-1][20:24, 20:24].tobytes() == levels[-1][20:24, 20:24].tobytes() and (cnt[20:24, 20:24] == 0).all()
    assert np.all(np.isfinite(new[-1])) and rec["n_carried"] > 0
    ex = _exact(levels[-1])
    assert (cnt[19, 19:24][ex[19, 19:24]] == 0).all()      # the upper / left neighbours gather a bad tap


def test_depth_edge_and_gate():
    levels = _scene()
    h, w = levels[-1].shape
    counts = np.full((h, w), 2, np.uint8)
    old = levels[-1].copy()
    old[:, 20:] += F32(0.3)                         # a 0.3 m step: taps straddling it trip the spread gate, the far side the |zi - Zk| gate
    new, cnt, rec = cref.carry(levels, old, counts, K_TOP, EYE, EYE, MIN_DEPTH, 0.05, 16)
    # pixel x = 20 gathers columns (19, 20) when its u rounds just below 20 (the spread gate) and (20, 21) otherwise (the |zi - Zk| gate)
    assert (cnt[:, 20:] == 0).all()
    assert new[-1][:, 20:].tobytes() == levels[-1][:, 20:].tobytes()
    assert (cnt[:, :19] > 0).sum() > (h - 1) * 19 // 2
    assert rec["n_gated"] >= (h - 1) * (w - 22) and rec["n_gated"] <= h * (w - 20)
    off = (levels[-1] + F32(0.1)).astype(F32)       # an offset surface: every pixel with taps fails only at the gate
    new, cnt, rec = cref.carry(levels, off, counts, K_TOP, EYE, EYE, MIN_DEPTH, 0.05, 16)
    assert rec["n_carried"] == 0 and (cnt == 0).all() and new[-1].tobytes() == levels[-1].tobytes()
    assert rec["n_gated"] >= (h - 2) * (w - 2)


def test_coarser_levels_are_culls_of_the_top():
    levels = _scene(h=31, w=43)                     # 15x21 and 7x10: truncating sizes
    h, w = levels[-1].shape
    old = (levels[-1] + F32(0.01)).astype(F32)
    new, cnt, rec = cref.carry(levels, old, np.zeros((h, w), np.uint8), K_TOP, EYE, EYE, MIN_DEPTH, 0.05, 16)
    assert rec["n_carried"] > 0 and new[-1].tobytes() != levels[-1].tobytes()
    assert new[1].tobytes() == kref.cull(new[-1], 1).tobytes() and new[1].shape == (15, 21)
    assert new[0].tobytes() == kref.cull(new[-1], 2).tobytes() and new[0].shape == (7, 10)
    assert new[1].tobytes() != levels[1].tobytes() and new[0].tobytes() != levels[0].tobytes()


def test_step_composes_the_push():
    levels = _scene()
    h, w = levels[-1].shape
    old = [(l + F32(0.01)).astype(F32) for l in levels]
    counts = np.full((h, w), 2, np.uint8)
    args = (K_TOP, EYE, EYE, MIN_DEPTH, 0.05, 0.05, 16)
    kf, c, fr, rc, rf = cref.step(cref.CARRY, kref.CLEAR, old, counts, levels, *args)
    want, wc, wr = cref.carry(levels, old[-1], counts, K_TOP, EYE, EYE, MIN_DEPTH, 0.05, 16)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(kf, want)) and c.tobytes() == wc.tobytes() and rc == wr
    assert all(a.tobytes() == b.tobytes() for a, b in zip(fr, want)) and rf == dict(n_candidates=0, n_fused=0, n_gated=0)
    kf, c, fr, rc, rf = cref.step(cref.CARRY, kref.CLEAR, old, counts, levels, *args, carry_on=False)   # carry off: today's clear
    assert all(a.tobytes() == b.tobytes() for a, b in zip(kf, levels)) and (c == 0).all() and rc == cref.ZERO
    kf, c, fr, rc, rf = cref.step(cref.NONE, kref.CLEAR, old, counts, levels, *args)                    # a start, a non-finite twist
    assert all(a.tobytes() == b.tobytes() for a, b in zip(kf, levels)) and (c == 0).all() and rc == cref.ZERO
    kf, c, fr, rc, rf = cref.step(cref.NONE, kref.FUSE, old, counts, levels, *args)
    want, wc, wr = kref.fuse(old, counts, levels[-1], K_TOP, EYE, EYE, MIN_DEPTH, 0.05, 16)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(kf, want)) and c.tobytes() == wc.tobytes() and rf == wr and rc == cref.ZERO
    kf, c, fr, rc, rf = cref.step(cref.NONE, kref.NONE, old, counts, levels, *args)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(kf, old)) and c.tobytes() == counts.tobytes()
    assert cref.modes(True, True, False, np.zeros(6)) == (cref.CARRY, kref.CLEAR)
    assert cref.modes(True, True, False, np.array([0, 0, np.nan, 0, 0, 0])) == (cref.NONE, kref.CLEAR)
    assert cref.modes(True, True, True, np.zeros(6)) == (cref.NONE, kref.CLEAR)
    assert cref.modes(True, False, False, np.zeros(6)) == (cref.NONE, kref.FUSE)
    assert cref.modes(False, False, False, np.zeros(6)) == (cref.NONE, kref.NONE)


# ---- register pins ----------------------------------------------------------------------------------------------------------------
def test_kernels_fit_the_budget():
    assert_map_kernels_fit((("_ZN3dvo10k_kf_carryENS_11KfCarryArgsE", 31 + 8), ("_ZN3dvo14k_kf_carry_camENS_11KfCarryArgsE", 31 + 8),
                            ("_ZN3dvo15k_kf_carry_prepENS_10KfPrepArgsE", 60 + 8),
                            ("_ZN3dvo17k_kf_carry_commitENS_17KfCarryCommitArgsE", 8 + 8)))
