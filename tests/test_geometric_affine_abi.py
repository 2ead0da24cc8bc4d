"""CPU tests of the geometric term composed with affine brightness compensation (include/dvo.h, dvo_batch_set_geometric_affine and
dvo_op_gn_step_geometric_affine): the two entry points are declared, exported, bound and in the C++ facade, every
refusal that needs no device is returned, the header states the contract, the reference of tests/geometric_affine_ref.py meets its
two anchors bit for bit -- the entry (1, 0) is geometric_ref.geometric_track, weight 0 is affine_ref.affine_track on own-depth inputs
-- and the hot kernel instances compile without scratch inside their wave budget, the solve twin no worse than k_gn_solve_ab."""
import ctypes as C
import inspect
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import affine_ref as ar
import dvo_amd as dvo
import geometric_affine_ref as ga
import geometric_ref as gr
import orc
from dvo_amd import synth
from util import K640

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "direct-visual-odometry_amd")
SIGNATURES = {
    "dvo_batch_set_geometric_affine": (r"int", r"dvo_batch\s*\*\s*\w+\s*,\s*const\s+dvo_geometric_config\s*\*\s*\w+\s*,\s*const\s+dvo_affine_config\s*\*\s*\w+"),
    "dvo_op_gn_step_geometric_affine": (r"int", r"int\s+dev\s*,\s*const\s+dvo_config\s*\*[^;]*const\s+float\s*\*\s*obj_depth[^;]*const\s+float\s*\*\s*ref_depth[^;]*"
                                                r"int\s+level\s*,\s*float\s+weight\s*,\s*float\s+max_diff\s*,\s*float\s+a\s*,\s*float\s+b\s*,\s*"
                                                r"dvo_gn_result\s*\*\s*\w+\s*,\s*double\s+\w+\[2\]\s*,\s*double\s+\w+\[5\]\s*,\s*float\s+\w+\[2\]"),
}


@pytest.mark.parametrize("name", sorted(SIGNATURES))
def test_declared_exported_and_listed(name):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dvo.h")).read(), flags=re.S)
    ret, args = SIGNATURES[name]
    assert re.search(r"\b%s\s+%s\s*\(\s*%s\s*\)\s*;" % (ret, name, args), txt), name
    assert hasattr(dvo.lib(), name)
    assert name in dvo.EXPORTS
    assert "dvo_*" in open(os.path.join(PKG, "csrc", "libdvo.map")).read()   # (the map exports the C ABI by its prefix)


def test_header_states_the_contract():
    txt = open(os.path.join(ROOT, "include", "dvo.h")).read()
    flat = re.sub(r"\s+", " ", re.sub(r"\n \*", " ", txt))
    for phrase in ("c = fmaf(a, I1, b); r = I2 - c; rw = r * wgt, slots 0..28", "The geometric row does not see (a, b)",
                   "(M1, M2, M11, M12, N = n_valid)", "the pair writes the affine entry and nothing else",
                   "(a, b) = (1, 0) makes every sum the geometric term's alone, bit for bit",
                   "weight = 0 makes the 27 sums and the moments the affine estimator's on own-depth inputs, bit for bit",
                   "dvo_batch_set_geometric(OFF / NULL) leaves the affine family on",
                   "dvo_batch_set_affine_brightness(OFF / NULL) leaves the geometric family on",
                   "k_track_gn_zab + k_gn_solve_zab", "Robust weights with the geometric term, mono batches and dvo_vo handles are out of scope"):
        assert phrase in flat, phrase


def test_bindings():
    assert callable(getattr(dvo.Batch, "set_geometric_affine", None))
    assert not hasattr(dvo.MonoBatch, "set_geometric_affine")    # sensor-depth batches only
    assert callable(dvo.op_gn_step_geometric_affine)
    d = {k: v.default for k, v in inspect.signature(dvo.Batch.set_geometric_affine).parameters.items() if k != "self"}
    assert d == dict(weight=10.0, max_diff=0.1, affine_mode=dvo.AFFINE_ESTIMATE, min_pixels=64, min_contrast=1e-3, gain_min=0.25, gain_max=4.0)
    assert {k: d[k] for k in ar.GUARDS} == ar.GUARDS


def test_null_and_bad_arguments_are_refused():
    L = dvo.lib()
    g = dvo.geometric_default_config()
    a = dvo.AffineConfig(C.sizeof(dvo.AffineConfig), dvo.AFFINE_ESTIMATE, 64, 1e-3, 0.25, 4.0)
    assert L.dvo_batch_set_geometric_affine(None, C.byref(g), C.byref(a)) == dvo.DVO_ERR_BAD_ARGUMENT
    assert L.dvo_batch_set_geometric_affine(None, None, None) == dvo.DVO_ERR_BAD_ARGUMENT
    out = dvo.GnResult()
    f = C.c_float
    sums = (C.c_double * 2)(); mom = (C.c_double * 5)(); nxt = (C.c_float * 2)()
    img = (C.c_float * 16)(); K = (C.c_float * 9)(); xi = (C.c_float * 6)()
    # NULL maps, NULL outputs, a weight or max_diff outside its range: refused before a device is opened
    call = lambda *p: L.dvo_op_gn_step_geometric_affine(0, None, *p)
    tail = (C.byref(out), sums, mom, nxt)
    assert call(None, None, None, None, None, 4, 4, None, None, 0, f(1.0), f(0.1), f(1.0), f(0.0), *tail) == dvo.DVO_ERR_BAD_ARGUMENT
    assert call(img, img, img, img, None, 4, 4, K, xi, 0, f(1.0), f(0.1), f(1.0), f(0.0), *tail) == dvo.DVO_ERR_BAD_ARGUMENT
    for k in (1, 2, 3):
        t = list(tail); t[k] = None
        assert call(img, img, img, img, img, 4, 4, K, xi, 0, f(1.0), f(0.1), f(1.0), f(0.0), *t) == dvo.DVO_ERR_BAD_ARGUMENT, k
    for weight, max_diff in ((-1.0, 0.1), (float("nan"), 0.1), (float("inf"), 0.1), (1.0, 0.0), (1.0, -0.1), (1.0, float("nan")), (1.0, float("inf"))):
        assert call(img, img, img, img, img, 4, 4, K, xi, 0, f(weight), f(max_diff), f(1.0), f(0.0), *tail) == dvo.DVO_ERR_BAD_ARGUMENT, (weight, max_diff)


def test_facade_method_compiles(tmp_path):
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
    bt.setGeometricAffine();
    bt.setGeometricAffine(30.0f, 0.05f, DVO_AFFINE_GIVEN);
    bt.setGeometricAffine(10.0f, 0.1f, DVO_AFFINE_ESTIMATE, 128, 1e-2f, 0.5f, 2.0f);
    std::vector<dvo_geometric_record> r = bt.lastGeometric();
    std::vector<float> ab = bt.lastAffine();
    bt.setGeometric(DVO_GEOMETRIC_OFF);
    bt.setAffineBrightness(DVO_AFFINE_OFF);
    return (int)r.size() + (int)ab.size();
}
""")
    r = subprocess.run([gxx, "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


# ------------------------------------------------------------------------------------------------ the reference's two anchors
LEVELS, CULLS = 3, 1
KH = np.array(K640, np.float32).copy()
KH[0] *= 0.5
KH[1] *= 0.5


@pytest.fixture(scope="module")
def two_frames():
    """the tracked frame under another exposure, so that the estimated entries are far from (1, 0)"""
    g, d, s, _ = synth.sequence(2, width=320, height_px=240, K=KH, seed=42, sigma_value=0.5)
    g, d, s = g.numpy(), d.numpy(), s.numpy()
    g1 = (np.float32(0.85) * g[1] + np.float32(0.04)).astype(np.float32)
    return orc.OFrame(g1, d[1], s[1], KH, LEVELS, CULLS), orc.OFrame(g[0], d[0], s[0], KH, LEVELS, CULLS)


def _same_call(xa, la, xb, lb):
    assert list(la["n_iter"]) == list(lb["n_iter"])
    assert np.asarray(xa, np.float32).tobytes() == np.asarray(xb, np.float32).tobytes(), (xa, xb)
    for l in range(LEVELS):
        assert la["residual"][l].tobytes() == lb["residual"][l].tobytes() and la["xi_after"][l].tobytes() == lb["xi_after"][l].tobytes(), l


def test_identity_entry_is_the_geometric_reference(two_frames):
    obj, ref = two_frames
    cfg = dvo.default_config()
    wp = gr.weight_params()
    xg, lg = gr.geometric_track(obj, ref, LEVELS, 10.0, 0.1, False, cfg.max_iterations, cfg.min_update, cfg.min_residual, wp=wp)
    xc, lc = ga.geometric_affine_track(obj, ref, LEVELS, 10.0, 0.1, ga.GIVEN, False, cfg.max_iterations, cfg.min_update, cfg.min_residual, wp=wp)
    _same_call(xc, lc, xg, lg)
    assert all(np.array_equal(lc["n_geo"][l], lg["n_geo"][l]) and lc["n_geo"][l].min() > 100 for l in range(LEVELS))
    # and the exact sums of one evaluation: the compensated terms with (1, 0) are the plain terms
    px = ga.frame_pixels(obj, ref, False, wp)(2, np.zeros(6, np.float32))
    a, b = ga.exact(px, 10.0, 0.1, 1.0, 0.0), gr.exact(px, 10.0, 0.1)
    for k in ("H", "g", "A_H", "A_g"):
        np.testing.assert_array_equal(a[k], b[k])
    assert (a["sum_r2"], a["S29"], a["n"], a["n_geo"]) == (b["sum_r2"], b["S29"], b["n"], b["n_geo"]) and a["n_geo"] > 1000


@pytest.mark.parametrize("mode", ["estimate", "given"])
def test_weight_zero_is_the_affine_reference_on_own_depth(two_frames, mode):
    obj, ref = two_frames
    wp = gr.weight_params()
    kw = dict(given_ab=(1.15, -0.03)) if mode == "given" else {}
    m = ga.ESTIMATE if mode == "estimate" else ga.GIVEN
    # (no residual stop and at most six iterations per level: several entries per level)
    xa, la = ar.affine_track(obj, ga.OwnDepth(obj, ref), LEVELS, m, False, 6, 2e-5, 0.0, wp=wp[:3], **kw)
    xc, lc = ga.geometric_affine_track(obj, ref, LEVELS, 0.0, 0.1, m, False, 6, 2e-5, 0.0, wp=wp, **kw)
    _same_call(xc, lc, xa, la)
    assert np.array(lc["ab"][0], np.float32).tobytes() == np.array(la["ab"][0], np.float32).tobytes()
    assert np.array(lc["ab"][LEVELS - 1], np.float32).tobytes() == np.array(la["ab"][LEVELS - 1], np.float32).tobytes()
    assert np.array(lc["prime"], np.float32).tobytes() == np.array(la["prime"], np.float32).tobytes()
    if mode == "estimate":   # the entry moved away from (1, 0) and lags by one iteration: the first one is the priming entry
        assert abs(float(lc["prime"][0]) - 1.0) > 0.05 and lc["ab"][0][0] == lc["prime"]
        used = [e for lv in lc["ab"] for e in lv]
        assert len(used) > LEVELS and len(set(used)) > 2


def test_reference_depths():
    assert gr.depths(4) == (21, 17, 13) and ga.moment_depth(4) == 17 and ga.moment_depth(1) == 11


# ------------------------------------------------------------------------------------------------ registers of the hot instances
# k_track_gn_zab / k_track_gn_zab_cam <4, 1 | 2, raster | 2-D tiles>: built for DVO_GN_ZAB_WAVES = 3 waves per SIMD -- 512 / 3 rounded
# down to the allocation granule of 8 = 168 VGPRs -- without scratch; k_gn_solve_zab against k_gn_solve_ab
ZAB_WAVES = 3
ZAB_VGPR_BUDGET = (512 // ZAB_WAVES) // 8 * 8


def _meta(txt, name):
    m = re.search(r"\.amdhsa_kernel %s.*?\.end_amdhsa_kernel" % re.escape(name), txt, re.S)
    assert m, "kernel not found: " + name
    body = m.group(0)
    return (int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", body).group(1)), int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body).group(1)))


def test_hot_composed_kernels_fit_the_register_budget():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    src = open(os.path.join(PKG, "csrc", "dvo_kernels.hip")).read()
    assert re.search(r"#define DVO_GN_ZAB_WAVES %d\b" % ZAB_WAVES, src)
    cont = open(os.path.join(PKG, "Makefile")).read().split("FLAGS   =", 1)[1].split("\n")
    flags = (cont[0].rstrip("\\") + " " + cont[1]).split()
    flags = [f.replace("$(ARCH)", "gfx950") for f in flags if f != "-fPIC"]
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "k.s")
        subprocess.run([hipcc] + flags + ["-S", "--cuda-device-only", "-o", out, os.path.join(PKG, "csrc", "dvo_kernels.hip")],
                       check=True, capture_output=True, timeout=900)
        txt = open(out).read()
    checked = 0
    args = "EEEvNS_6GnArgsENS_8AffineGnENS_5GeoGnE"
    for kernel in ("_ZN3dvo14k_track_gn_zab", "_ZN3dvo18k_track_gn_zab_cam"):
        for variant in ("ILi4ELi1ELb0", "ILi4ELi1ELb1", "ILi4ELi2ELb0", "ILi4ELi2ELb1"):   # <PPT 4, G 1 | 2, T2D>
            vgpr, scratch = _meta(txt, kernel + variant + args)
            assert scratch == 0, "%s%s spills %d bytes of scratch per lane" % (kernel, variant, scratch)
            assert vgpr <= ZAB_VGPR_BUDGET, "%s%s needs %d VGPRs (budget %d = %d waves per SIMD)" % (kernel, variant, vgpr, ZAB_VGPR_BUDGET, ZAB_WAVES)
            checked += 1
    assert checked == 8
    ab = _meta(txt, "_ZN3dvo13k_gn_solve_abENS_9SolveArgsENS_11RobustSolveENS_11AffineSolveE")
    zab = _meta(txt, "_ZN3dvo14k_gn_solve_zabENS_9SolveArgsENS_11AffineSolveENS_8GeoSolveE")
    assert zab[0] <= ab[0] and zab[1] <= ab[1], ("k_gn_solve_zab (VGPRs, scratch) %s against k_gn_solve_ab %s" % (zab, ab))
    # the families it is composed of keep their names and template parameters beside it
    assert re.search(r"\.amdhsa_kernel _ZN3dvo12k_track_gn_zILi4ELi2ELb0EEEvNS_6GnArgsENS_5GeoGnE\b", txt)
    assert re.search(r"\.amdhsa_kernel _ZN3dvo13k_track_gn_abILi4ELi2ELb0ELb0EEEvNS_6GnArgsENS_8RobustGnENS_8AffineGnE\b", txt)
