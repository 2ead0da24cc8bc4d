"""CPU tests of keyframe depth fusion (include/dvo.h, dvo_batch_set_keyframe_fusion): the entry points are declared,
exported and bound, NULL and bad arguments are refused before anything touches the GPU, the header states the contract, the C++ facade
compiles, the replica (tests/kf_fusion_ref.py) keeps its anchors, and the new kernels need no scratch and stay within the VGPRs measured
when they were written (k_kf_fuse 31, k_kf_fuse_prep 58) plus one allocation unit of 8."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import dvo_amd as dvo
import kf_fusion_ref as kref
from kf_common import assert_map_kernels_fit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("dvo_kf_fusion_config_default", "dvo_batch_set_keyframe_fusion", "dvo_batch_last_keyframe_fusion", "dvo_batch_keyframe_fusion_counts")
F32 = np.float32
KF_ON, KF_OFF = dvo.KF_FUSION_ON, dvo.KF_FUSION_OFF   # (without the feature the file fails here, at import)


def _header():
    return open(os.path.join(ROOT, "include", "dvo.h")).read()


def test_declared_exported_and_listed():
    txt = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert re.search(r"#define\s+DVO_KF_FUSION_OFF\s+0\b", txt) and re.search(r"#define\s+DVO_KF_FUSION_ON\s+1\b", txt)
    assert re.search(r"typedef\s+struct\s+dvo_kf_fusion_config\s*\{\s*int\s+mode;\s*float\s+max_diff;\s*int\s+max_count;\s*\}", txt)
    assert re.search(r"typedef\s+struct\s+dvo_kf_fusion_record\s*\{\s*int\s+struct_size,\s*n_candidates,\s*n_fused,\s*n_gated;\s*\}", txt)
    assert re.search(r"\bvoid\s+dvo_kf_fusion_config_default\s*\(\s*dvo_kf_fusion_config\s*\*", txt)
    assert re.search(r"\bint\s+dvo_batch_set_keyframe_fusion\s*\(\s*dvo_batch\s*\*\s*\w+\s*,\s*const\s+dvo_kf_fusion_config\s*\*", txt)
    assert re.search(r"\bint\s+dvo_batch_last_keyframe_fusion\s*\(\s*dvo_batch\s*\*\s*\w+\s*,\s*dvo_kf_fusion_record\s*\*", txt)
    assert re.search(r"\bint\s+dvo_batch_keyframe_fusion_counts\s*\(\s*dvo_batch\s*\*\s*\w+\s*,\s*int\s+\w+\s*,\s*uint8_t\s*\*", txt)
    for n in NAMES:
        assert hasattr(dvo.lib(), n), n
        assert n in dvo.EXPORTS, n


def test_the_header_states_the_contract():
    txt = " ".join(_header().split())
    for phrase in ("no contraction beyond the fmaf()s named", "d >= min_depth", "holes are never filled", "0 <= u < w - 1",
                   "max4 - min4 <= max_diff", "fmaf(a, z10 - z00, z00)", "fmaf(b, bot - top, top)", "fabsf(zi - Zf) <= max_diff",
                   "1.0f / (float)(c + 2)", "fmaf(d_obs - d, r, d)", "min(c + 1, max_count)", "dvo_op_se3_exp(-xi)",
                   "order-free, deterministic", "weight maps are not touched"):
        assert phrase in txt, phrase


def test_default_config_and_struct_sizes():
    c = dvo.KfFusionConfig()
    dvo.lib().dvo_kf_fusion_config_default(C.byref(c))
    assert (c.mode, c.max_count) == (dvo.KF_FUSION_ON, 16) and F32(c.max_diff) == F32(0.05)
    dvo.lib().dvo_kf_fusion_config_default(None)
    assert C.sizeof(dvo.KfFusionConfig) == 12 and C.sizeof(dvo.KfFusionRecord) == 16
    assert dvo.KF_FUSION_RECORD_DTYPE.itemsize == 16
    assert (dvo.KF_FUSION_OFF, dvo.KF_FUSION_ON) == (0, 1)


def test_the_batch_binds_it():
    for m in ("set_keyframe_fusion", "last_keyframe_fusion", "keyframe_fusion_counts"):
        assert callable(getattr(dvo.Batch, m, None)), m
        assert not hasattr(dvo.MonoBatch, m), m


def test_null_arguments_are_refused():
    L = dvo.lib()
    c = dvo.KfFusionConfig(dvo.KF_FUSION_ON, 0.05, 16)
    rec = (dvo.KfFusionRecord * 1)()
    buf = (C.c_uint8 * 4)()
    assert L.dvo_batch_set_keyframe_fusion(None, C.byref(c)) == dvo.DVO_ERR_BAD_ARGUMENT
    assert L.dvo_batch_set_keyframe_fusion(None, None) == dvo.DVO_ERR_BAD_ARGUMENT
    assert L.dvo_batch_last_keyframe_fusion(None, rec) == dvo.DVO_ERR_BAD_ARGUMENT
    assert L.dvo_batch_keyframe_fusion_counts(None, 0, buf) == dvo.DVO_ERR_BAD_ARGUMENT


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
    bt.setKeyframeFusion(DVO_KF_FUSION_ON, 0.03f, 8);
    bt.setKeyframeFusion(DVO_KF_FUSION_OFF);
    std::vector<dvo_kf_fusion_record> r = bt.lastKeyframeFusion();
    std::vector<uint8_t> c = bt.keyframeFusionCounts(1);
    return (int)(r.size() + c.size()) + r[0].n_fused;
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
    levels = [kref.cull(top, 2), kref.cull(top, 1), top]
    return levels, np.zeros((h, w), np.uint8)


def test_identity_leaves_depth_and_raises_counts():
    """A frame identical to the keyframe with F = Bk = I: u = x and v = y exactly are not guaranteed by the projection, but wherever the
    pixel projects onto itself (a = b = 0) zi = d and d_obs - d = 0: the depth is unchanged bit for bit and the count rises."""
    levels, counts = _scene()
    new, cnt, rec = kref.fuse(levels, counts, levels[-1], K_TOP, EYE, EYE, MIN_DEPTH, 0.05, 16)
    h, w = counts.shape
    assert rec["n_candidates"] == h * w and rec["n_gated"] == 0
    assert rec["n_fused"] == int((cnt == 1).sum()) and rec["n_fused"] > (h - 2) * (w - 2) // 2
    k = kref.intr(K_TOP)
    ys, xs = np.mgrid[0:h, 0:w]
    X, Y, Z = kref.back_project(k, xs.astype(F32), ys.astype(F32), levels[-1])
    u, v = kref.project(k, X, Y, Z)
    exact = (u == xs) & (v == ys) & (cnt == 1)
    assert exact.sum() > 100
    assert new[-1][exact].tobytes() == levels[-1][exact].tobytes()
    # everywhere the blend stays within the taps' spread of the keyframe's own value
    assert np.abs(new[-1] - levels[-1]).max() <= 0.012


def test_max_count_one_keeps_a_third():
    levels, counts = _scene()
    frame = (levels[-1] + F32(0.03)).astype(F32)
    l1, c1, _ = kref.fuse(levels, counts, frame, K_TOP, EYE, EYE, MIN_DEPTH, 0.05, 1)
    l2, c2, _ = kref.fuse(l1, c1, frame, K_TOP, EYE, EYE, MIN_DEPTH, 0.05, 1)
    l3, c3, _ = kref.fuse(l2, c2, frame, K_TOP, EYE, EYE, MIN_DEPTH, 0.05, 1)
    assert c1.max() == 1 and c2.max() == 1 and c3.max() == 1
    m = (c1 == 1)
    r3 = F32(1) / F32(3)
    # second and third fusion: c = 1, r = 1 / 3, on the identity pixels d_obs = the frame's own value
    k = kref.intr(K_TOP)
    ys, xs = np.mgrid[0:counts.shape[0], 0:counts.shape[1]]
    u, v = kref.project(k, *kref.back_project(k, xs.astype(F32), ys.astype(F32), l2[-1]))
    ex = m & (u == xs) & (v == ys) & (xs < counts.shape[1] - 1) & (ys < counts.shape[0] - 1)   # (u = w - 1 exactly is outside)
    assert ex.sum() > 50
    want = kref.rr.fmaf((frame - l2[-1]).astype(F32), np.full_like(frame, r3), l2[-1])
    assert l3[-1][ex].tobytes() == want[ex].tobytes()


@pytest.mark.parametrize("bad", [np.nan, np.inf, 0.0, 0.1])
def test_bad_pixels_and_taps_change_nothing(bad):
    levels, counts = _scene()
    kf = [l.copy() for l in levels]
    kf[-1][10:14, 10:14] = bad
    new, cnt, rec = kref.fuse(kf, counts, levels[-1], K_TOP, EYE, EYE, MIN_DEPTH, 0.05, 16)
    assert new[-1][10:14, 10:14].tobytes() == kf[-1][10:14, 10:14].tobytes() and (cnt[10:14, 10:14] == 0).all()
    frame = levels[-1].copy()
    frame[20:24, 20:24] = bad
    new, cnt, rec = kref.fuse(levels, counts, frame, K_TOP, EYE, EYE, MIN_DEPTH, 0.05, 16)
    # every pixel one of whose four taps is bad is unchanged: the block and its upper / left neighbours at most
    assert new[-1][20:24, 20:24].tobytes() == levels[-1][20:24, 20:24].tobytes() and (cnt[20:24, 20:24] == 0).all()
    assert np.all(np.isfinite(new[-1]))
    assert rec["n_fused"] > 0


def test_depth_edge_and_gate():
    levels, counts = _scene()
    frame = levels[-1].copy()
    frame[:, 20:] += F32(0.3)                       # a step: pixels whose taps straddle it are not fused, the far side is gated
    new, cnt, rec = kref.fuse(levels, counts, frame, K_TOP, EYE, EYE, MIN_DEPTH, 0.05, 16)
    assert (cnt[:, 21:] == 0).all() and rec["n_gated"] >= (counts.shape[0] - 1) * (counts.shape[1] - 22)
    assert new[-1][:, 21:].tobytes() == levels[-1][:, 21:].tobytes()


def test_coarser_levels_are_culls_of_the_top():
    levels, counts = _scene(h=31, w=43)             # 15x21 and 7x10: truncating sizes
    frame = (levels[-1] + F32(0.01)).astype(F32)
    new, cnt, rec = kref.fuse(levels, counts, frame, K_TOP, EYE, EYE, MIN_DEPTH, 0.05, 16)
    assert rec["n_fused"] > 0 and new[-1].tobytes() != levels[-1].tobytes()
    assert new[1].tobytes() == kref.cull(new[-1], 1).tobytes() and new[1].shape == (15, 21)
    assert new[0].tobytes() == kref.cull(new[-1], 2).tobytes() and new[0].shape == (7, 10)
    lv, c, r = kref.clear(new, cnt)
    assert (c == 0).all() and r == dict(n_candidates=0, n_fused=0, n_gated=0)


# ---- register pins ----------------------------------------------------------------------------------------------------------------
def test_kernels_fit_the_budget():
    assert_map_kernels_fit((("_ZN3dvo9k_kf_fuseENS_10KfFuseArgsE", 31 + 8), ("_ZN3dvo13k_kf_fuse_camENS_10KfFuseArgsE", 31 + 8),
                            ("_ZN3dvo14k_kf_fuse_prepENS_10KfPrepArgsE", 58 + 8)))
