"""CPU tests of a batch's robust residual weights (include/dvo.h, dvo_batch_set_robust_weights and its companions): the entry points
are declared, exported and bound, dvo_robust_config has the same layout in C and in ctypes, a NULL handle is refused before anything
touches the GPU, the C++ facade's new methods compile, the reference arithmetic of tests/robust_ref.py is self-consistent, and the two
hot weighted kernel instances compile without scratch inside the plain kernel's register budget."""
import ctypes as C
import os
import re
import shutil
import subprocess
import tempfile
from fractions import Fraction

import numpy as np
import pytest

import dvo_amd as dvo
import robust_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "direct-visual-odometry_amd")
SIGNATURES = {
    "dvo_batch_set_robust_weights": r"dvo_batch\s*\*\s*\w+\s*,\s*const\s+dvo_robust_config\s*\*\s*\w+",
    "dvo_batch_set_robust_scales": r"dvo_batch\s*\*\s*\w+\s*,\s*const\s+float\s*\*\s*\w+\s*,\s*int\s+\w+",
    "dvo_batch_last_robust_scales": r"dvo_batch\s*\*\s*\w+\s*,\s*float\s*\*\s*\w+",
    "dvo_op_gn_step_robust": r"int\s+dev\s*,\s*const\s+dvo_config\s*\*[^;]*int\s+level\s*,\s*int\s+kind\s*,\s*float\s+param\s*,\s*float\s+s2\s*,"
                             r"\s*dvo_gn_result\s*\*\s*\w+",
}
FIELDS = [f[0] for f in dvo.RobustConfig._fields_]


@pytest.mark.parametrize("name", sorted(SIGNATURES))
def test_declared_exported_and_listed(name):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dvo.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+%s\s*\(\s*%s\s*\)\s*;" % (name, SIGNATURES[name]), txt), name
    assert hasattr(dvo.lib(), name)
    assert name in dvo.EXPORTS


def test_constants_are_declared():
    txt = open(os.path.join(ROOT, "include", "dvo.h")).read()
    for name, v in (("NONE", 0), ("HUBER", 1), ("STUDENT_T", 2), ("SCALE_ADAPTIVE", 0), ("SCALE_GIVEN", 1)):
        assert re.search(r"#define\s+DVO_ROBUST_%s\s+%d\b" % (name, v), txt), name
        assert getattr(dvo, "ROBUST_" + name) == v
    assert (rr.NONE, rr.HUBER, rr.STUDENT_T, rr.ADAPTIVE, rr.GIVEN) == (0, 1, 2, 0, 1)
    assert "weighted mean square" in re.sub(r"\s+", " ", txt.lower())   # dvo.h says what `residual` is while weights are on


def test_layout_matches_c():
    cc = shutil.which("gcc") or shutil.which("cc")
    if not cc:
        pytest.skip("no C compiler")
    with tempfile.TemporaryDirectory() as td:
        src = os.path.join(td, "layout.c")
        body = "".join('    printf("%s %%zu\\n", offsetof(dvo_robust_config, %s));\n' % (f, f) for f in FIELDS)
        open(src, "w").write('#include <stddef.h>\n#include <stdio.h>\n#include <stdint.h>\n#include "dvo.h"\nint main(void)\n{\n'
                             '    printf("sizeof %zu\\n", sizeof(dvo_robust_config));\n' + body + "    return 0;\n}\n")
        exe = os.path.join(td, "layout")
        subprocess.run([cc, "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", exe, src], check=True, capture_output=True)
        out = dict(l.split() for l in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split("\n") if l)
    assert int(out["sizeof"]) == C.sizeof(dvo.RobustConfig) == 20
    for f in FIELDS:
        assert int(out[f]) == getattr(dvo.RobustConfig, f).offset, f
    assert FIELDS == ["struct_size", "kind", "scale_mode", "param", "scale_floor"]


def test_both_batches_bind_them():
    for cls in (dvo.Batch, dvo.MonoBatch):
        for m in ("set_robust_weights", "set_robust_scales", "last_robust_scales"):
            assert callable(getattr(cls, m, None)), (cls.__name__, m)
    assert callable(dvo.optimize_robust)


def test_null_handle_and_bad_operator_arguments_are_refused():
    L = dvo.lib()
    cfg = dvo.RobustConfig(C.sizeof(dvo.RobustConfig), dvo.ROBUST_HUBER, dvo.ROBUST_SCALE_ADAPTIVE, 1.345, 1e-3)
    s = (C.c_float * 2)(1.0, 1.0)
    assert L.dvo_batch_set_robust_weights(None, C.byref(cfg)) == dvo.DVO_ERR_BAD_ARGUMENT
    assert L.dvo_batch_set_robust_weights(None, None) == dvo.DVO_ERR_BAD_ARGUMENT
    assert L.dvo_batch_set_robust_scales(None, s, 0) == dvo.DVO_ERR_BAD_ARGUMENT
    assert L.dvo_batch_set_robust_scales(None, None, 0) == dvo.DVO_ERR_BAD_ARGUMENT
    assert L.dvo_batch_last_robust_scales(None, s) == dvo.DVO_ERR_BAD_ARGUMENT
    out = dvo.GnResult()
    f = C.c_float
    # a kind outside the set, a param that is not finite and > 0, NULL maps: refused before a device is opened
    assert L.dvo_op_gn_step_robust(0, None, None, None, None, None, 4, 4, None, None, 0, 1, f(1.0), f(1.0), C.byref(out)) == dvo.DVO_ERR_BAD_ARGUMENT
    img = (C.c_float * 16)(); K = (C.c_float * 9)(); xi = (C.c_float * 6)()
    for kind, param in ((3, 1.0), (-1, 1.0), (1, 0.0), (1, -1.0), (2, float("nan")), (2, float("inf"))):
        assert L.dvo_op_gn_step_robust(0, None, img, img, img, img, 4, 4, K, xi, 0, kind, f(param), f(1.0), C.byref(out)) == dvo.DVO_ERR_BAD_ARGUMENT, \
            (kind, param)


def test_facade_robust_methods_compile(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("g++ not available")
    src = tmp_path / "snippet.cpp"
    src.write_text(r"""
#include "dvo.hpp"
#include <vector>
int use(const float* dev_scales)
{
    const dvo::Mat3 K{525.f, 0.f, 319.5f, 0.f, 525.f, 239.5f, 0.f, 0.f, 1.f};
    dvo::BatchTracker bt(4, K, 640, 480);
    bt.setRobustWeights(DVO_ROBUST_HUBER);
    bt.setRobustWeights(DVO_ROBUST_STUDENT_T, 5.0f, DVO_ROBUST_SCALE_GIVEN);
    bt.setRobustScales(dev_scales, true);
    std::vector<float> s0 = bt.lastRobustScales();
    bt.setRobustWeights(DVO_ROBUST_NONE);
    dvo::BatchMono mb(4, K, 640, 480);
    mb.setRobustWeights(DVO_ROBUST_HUBER, 1.345f, DVO_ROBUST_SCALE_ADAPTIVE, 1e-3f);
    mb.setRobustScales(nullptr);
    std::vector<float> s1 = mb.lastRobustScales();
    return (int)(s0.size() + s1.size());
}
""")
    r = subprocess.run([gxx, "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


# ------------------------------------------------------------------------------------------------ the reference's own arithmetic
def test_reference_fmaf_is_correctly_rounded():
    rng = np.random.RandomState(5)
    a = rng.standard_normal(4000).astype(np.float32); b = rng.standard_normal(4000).astype(np.float32)
    c = (rng.standard_normal(4000) * 10.0 ** rng.uniform(-8, 2, 4000)).astype(np.float32)
    # operands built to land exactly on float32 midpoints after the float64 rounding (the double-rounding cases)
    a = np.concatenate([a, np.float32([1.0 + 2.0 ** -12, 1.0 + 2.0 ** -23, 3.0])])
    b = np.concatenate([b, np.float32([1.0 + 2.0 ** -12, 1.0 - 2.0 ** -24, 2.0 ** -25])])
    c = np.concatenate([c, np.float32([2.0 ** -60, 2.0 ** -80, 1.0])])
    got = rr.fmaf(a, b, c)
    for i in range(a.size):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        v = got[i]
        lo, hi = np.nextafter(v, np.float32(-np.inf)), np.nextafter(v, np.float32(np.inf))
        err = abs(Fraction(float(v)) - exact)
        assert err <= abs(Fraction(float(lo)) - exact) and err <= abs(Fraction(float(hi)) - exact), (i, a[i], b[i], c[i], v)


def test_reference_weights():
    r = np.float32([0.0, 1e-3, -0.05, 0.2, -3.0])
    np.testing.assert_array_equal(rr.rho(rr.NONE, 1.0, 1e-2, r), np.ones(5, np.float32))
    for bad in (0.0, -1.0, np.nan, np.inf):                       # a scale that is not finite and > 0: plain
        np.testing.assert_array_equal(rr.rho(rr.HUBER, 1.345, bad, r), np.ones(5, np.float32))
        np.testing.assert_array_equal(rr.rho(rr.STUDENT_T, 5.0, bad, r), np.ones(5, np.float32))
    c = np.float32(1.345) * np.sqrt(np.float32(1e-2))
    w = rr.rho(rr.HUBER, 1.345, 1e-2, r)
    np.testing.assert_array_equal(w, np.float32([1, 1, 1, c / np.float32(0.2), c / np.float32(3.0)]))
    w = rr.rho(rr.STUDENT_T, 5.0, 1e-2, r)
    assert w[0] == np.float32(np.float32(6.0) * np.float32(1e-2)) / (np.float32(5.0) * np.float32(1e-2))   # r = 0: (nu + 1) / nu up to one rounding
    assert np.all(np.diff(w[[0, 1, 2, 3, 4]]) < 0)
    assert rr.adaptive_s2(None, 1e-6) == np.inf and rr.adaptive_s2(-1.0, 1e-6) == np.inf and rr.adaptive_s2(0.0, 1e-6) == np.inf
    assert rr.adaptive_s2(np.float32(1e-7), np.float32(1e-6)) == np.float32(1e-6)
    assert rr.adaptive_s2(np.float32(3e-4), np.float32(1e-6)) == np.float32(3e-4)


def test_reference_sums_with_unit_weights_are_the_plain_sums():
    import gn_sums
    rng = np.random.RandomState(2)
    t = dict(J=rng.standard_normal((500, 6)).astype(np.float32), r=(0.1 * rng.standard_normal(500)).astype(np.float32))
    t["rw"] = (t["r"] * np.float32(3.0)).astype(np.float32)
    plain = gn_sums.exact_sums(t)
    for kind, s2 in ((rr.NONE, 1.0), (rr.HUBER, 1e12), (rr.STUDENT_T, np.inf)):
        ex = rr.exact_sums(t, kind, 1.345, s2)
        for k in ("H", "g", "A_H", "A_g"):
            np.testing.assert_array_equal(ex[k], plain[k])
        assert ex["sum_r2"] == plain["sum_r2"] and ex["n"] == 500
    ex = rr.exact_sums(t, rr.HUBER, 1.345, 1e-4)
    assert 0 < ex["sum_r2"] < plain["sum_r2"] and (ex["rho"] < 1).any() and (ex["rho"] == 1).any()


# ------------------------------------------------------------------------------------------------ registers of the hot instances
# k_track_gn_rw / k_track_gn_rw_cam <4, 2, raster | 2-D tiles>: built for the plain kernel's 6 waves per SIMD (84 VGPRs), no scratch
RW_VGPR_BUDGET = 84


def test_hot_weighted_kernels_fit_the_register_budget():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    cont = open(os.path.join(PKG, "Makefile")).read().split("FLAGS   =", 1)[1].split("\n")
    flags = (cont[0].rstrip("\\") + " " + cont[1]).split()
    flags = [f.replace("$(ARCH)", "gfx950") for f in flags if f != "-fPIC"]
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "k.s")
        subprocess.run([hipcc] + flags + ["-S", "--cuda-device-only", "-o", out, os.path.join(PKG, "csrc", "dvo_kernels.hip")],
                       check=True, capture_output=True, timeout=900)
        txt = open(out).read()
    checked = 0
    for kernel in ("_ZN3dvo13k_track_gn_rw", "_ZN3dvo17k_track_gn_rw_cam"):
        for variant in ("ILi4ELi2ELb0EE", "ILi4ELi2ELb1EE"):   # <PPT 4, G 2, raster | 2-D tiles>
            m = re.search(r"\.amdhsa_kernel %s%s.*?\.end_amdhsa_kernel" % (kernel, variant), txt, re.S)
            assert m, "kernel variant not found: " + kernel + variant
            body = m.group(0)
            scratch = int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body).group(1))
            vgpr = int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", body).group(1))
            assert scratch == 0, "%s%s spills %d bytes of scratch per lane" % (kernel, variant, scratch)
            assert vgpr <= RW_VGPR_BUDGET, "%s%s needs %d VGPRs (budget %d = 6 waves per SIMD)" % (kernel, variant, vgpr, RW_VGPR_BUDGET)
            checked += 1
    assert checked == 4
    # the plain kernel keeps its name and its four template parameters beside the new family
    assert re.search(r"\.amdhsa_kernel _ZN3dvo10k_track_gnILi4ELi2ELb0ELb0EEEvNS_6GnArgsE\b", txt)
