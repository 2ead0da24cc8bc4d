"""CPU tests of the photometric calibration fused into the mono ingest (include/dvo.h, dvo_batch_set_photometric and its companions,
DESIGN.md §31): the five entry points are declared, exported and bound, the new dvo_pyramid_kernel kinds agree between header and
binding, the header states the contract, every refusal that needs no handle is made before anything touches the GPU, the C++
facade's new methods compile, the numpy replica (tests/photometric_ref.py) holds on hand-made bytes, the identity table is
k_ingest's scale, and the new per-frame kernels compile for gfx950 without scratch."""
import ctypes as C
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import dvo_amd as dvo
import photometric_ref as pr
from lockstep import raw_gray

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "direct-visual-odometry_amd")
F32 = np.float32
SIGNATURES = {
    "dvo_batch_set_photometric": r"dvo_batch\s*\*\s*\w+\s*,\s*int\s+n_cal\s*,\s*const\s+float\s*\*\s*inv_response\s*,\s*const\s+float\s*\*\s*vignette\s*,"
                                 r"\s*const\s+int\s*\*\s*seq_cal",
    "dvo_batch_get_photometric": r"dvo_batch\s*\*\s*\w+\s*,\s*int\s*\*\s*n_cal\s*,\s*int\s*\*\s*seq_cal",
    "dvo_vo_set_photometric": r"dvo_vo\s*\*\s*\w+\s*,\s*const\s+float\s+inv_response\s*\[\s*256\s*\]\s*,\s*const\s+float\s*\*\s*vignette",
    "dvo_debug_batch_photometric_gain": r"dvo_batch\s*\*\s*\w+\s*,\s*int\s+seq\s*,\s*float\s*\*\s*gain",
    "dvo_debug_batch_last_pyramid_kernel": r"dvo_batch\s*\*\s*\w+\s*,\s*dvo_pyramid_kernel\s*\*\s*\w+",
}


@pytest.mark.parametrize("name", sorted(SIGNATURES))
def test_declared_exported_and_listed(name):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dvo.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+%s\s*\(\s*%s\s*\)\s*;" % (name, SIGNATURES[name]), txt), name
    assert hasattr(dvo.lib(), name)
    assert name in dvo.EXPORTS


def test_kind_constants_and_contract_phrases():
    txt = open(os.path.join(ROOT, "include", "dvo.h")).read()
    for name, value in (("PHOTO_RAW4", 4), ("PHOTO_SCALAR", 5), ("PHOTO_REMAP", 6)):
        assert re.search(r"#define\s+DVO_PYRAMID_KERNEL_%s\s+%d\b" % (name, value), txt), name
        assert getattr(dvo, "PYRAMID_KERNEL_" + name) == value
    assert (dvo.PYRAMID_KERNEL_SCALAR, dvo.PYRAMID_KERNEL_RAW4, dvo.PYRAMID_KERNEL_SPLIT, dvo.PYRAMID_KERNEL_REMAP) == (0, 1, 2, 3)
    k = dvo.PyramidKernel(dvo.PYRAMID_KERNEL_PHOTO_RAW4, 2, 1)
    assert k.name() == "k_pyramid_raw4_photo<2, true>"
    assert dvo.PyramidKernel(dvo.PYRAMID_KERNEL_PHOTO_SCALAR, 0, 0).name() == "k_pyramid_photo<false, false>"
    assert dvo.PyramidKernel(dvo.PYRAMID_KERNEL_PHOTO_REMAP, 0, 1).name() == "k_pyramid_photo<true, true>"
    flat = re.sub(r"[\s*]+", " ", txt)
    for phrase in ("gray = inv_response[c][g8] (1.0f / vignette[c][p])", "one IEEE division (done once, at set time), one multiply, no contraction",
                   "gray = DVO_INVALID where vignette[c][p] is not finite or <= 0", "(float)i (float)(1.0 / 255.0)", "vignette NULL means 1",
                   "applied to the luma, not per channel", "(index -1 stays DVO_INVALID)", "static per-camera mask",
                   "n_cal = 0 clears it", "Before the first frame only", "dvo_last_error names the first bad calibration or sequence",
                   "set in either order", "Calibration needs the byte", "dvo_batch_set_affine_rows in GIVEN mode",
                   "runs exactly the launches it runs without this entry point"):
        assert phrase in flat, phrase
    kh = open(os.path.join(PKG, "csrc", "dvo_kernels.h")).read()
    assert "struct PhotoArgs" in kh and re.search(r"kPhotoMasked\s*=\s*-1\.0f", kh)
    assert "PhotoArgs" not in kh.split("struct PyramidArgs {", 1)[1].split("};", 1)[0]   # a second block, not new PyramidArgs members


def test_bindings_exist():
    for m in ("set_photometric", "get_photometric", "photometric_gain", "last_pyramid_kernel"):
        assert callable(getattr(dvo.MonoBatch, m, None)), m
    assert callable(getattr(dvo.VisualOdometry, "set_photometric", None))
    assert not hasattr(dvo.Batch, "set_photometric")     # sensor-depth batches: the follow-up


def test_refusals_that_need_no_handle():
    L = dvo.lib()
    lut = pr.identity_response()
    n = C.c_int(7)
    k = dvo.PyramidKernel()
    g = np.zeros(4, F32)
    assert L.dvo_batch_set_photometric(None, 1, dvo.fp(lut), None, None) == dvo.DVO_ERR_BAD_ARGUMENT
    assert b"null handle" in L.dvo_last_error()
    assert L.dvo_batch_set_photometric(None, 0, None, None, None) == dvo.DVO_ERR_BAD_ARGUMENT
    assert L.dvo_batch_get_photometric(None, C.byref(n), None) == dvo.DVO_ERR_BAD_ARGUMENT and n.value == 7
    assert L.dvo_vo_set_photometric(None, dvo.fp(lut), None) == dvo.DVO_ERR_BAD_ARGUMENT
    assert L.dvo_vo_set_photometric(None, None, None) == dvo.DVO_ERR_BAD_ARGUMENT
    assert L.dvo_debug_batch_photometric_gain(None, 0, dvo.fp(g)) == dvo.DVO_ERR_BAD_ARGUMENT
    assert L.dvo_debug_batch_last_pyramid_kernel(None, C.byref(k)) == dvo.DVO_ERR_BAD_ARGUMENT


def test_facade_methods_compile(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to check the facade"
    src = tmp_path / "snippet.cpp"
    src.write_text(r"""
#include "dvo.hpp"
#include <vector>
int use()
{
    const dvo::Mat3 K{525.f, 0.f, 319.5f, 0.f, 525.f, 239.5f, 0.f, 0.f, 1.f};
    std::vector<float> lut(2 * 256, 0.5f), vig(2 * 640 * 480, 1.0f);
    const int cal[4] = {0, 1, 1, 0};
    dvo::BatchMono mb(4, K, 640, 480);
    mb.setPhotometric(2, lut.data(), vig.data(), cal);
    mb.setPhotometric(1, lut.data(), nullptr);
    mb.setPhotometric(0, nullptr, nullptr);
    dvo::VisualOdometry vo(K, 640, 480);
    vo.setPhotometric(lut.data(), vig.data());
    vo.setPhotometric(nullptr, nullptr);
    return DVO_PYRAMID_KERNEL_PHOTO_RAW4 + DVO_PYRAMID_KERNEL_PHOTO_SCALAR + DVO_PYRAMID_KERNEL_PHOTO_REMAP;
}
""")
    r = subprocess.run([gxx, "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


# ------------------------------------------------------------------------------------------------ the replica's own rules
def test_identity_table_is_the_ingest_scale():
    t = pr.identity_response()
    assert t.dtype == F32 and t.shape == (256,)
    for i in range(256):
        assert t[i] == F32(i) * F32(1.0 / 255.0), i
    u8 = np.arange(256, dtype=np.uint8).reshape(16, 16)
    assert pr.correct_np(u8).tobytes() == raw_gray(u8).tobytes()                       # NULL, NULL: k_ingest's gray
    assert pr.correct_np(u8, t, np.ones((16, 16), F32)).tobytes() == raw_gray(u8).tobytes()


def test_replica_on_hand_made_bytes():
    lut = pr.gamma_response(2.2).astype(F32)
    assert lut[0] == 0 and lut[255] == 1 and (np.diff(lut) > 0).all()
    u8 = np.array([[0, 255, 128, 7]], np.uint8)
    V = np.array([[0.5, 0.25, 0.0, 0.8]], F32)
    out = pr.correct_np(u8, lut, V)
    assert out[0, 0] == 0 and out[0, 1] == F32(4.0) and out[0, 2] == -2 and out[0, 3] == lut[7] * (F32(1.0) / F32(0.8))
    assert out.dtype == F32
    # the product is ONE division and ONE multiply in float32, not lut / V
    v3 = F32(3.0)
    differs = [i for i in range(256) if lut[i] * (F32(1.0) / v3) != lut[i] / v3]
    assert differs, "the two roundings must be distinguishable for the test to mean anything"
    i = differs[0]
    assert pr.correct_np(np.array([[i]], np.uint8), lut, np.array([[3.0]], F32))[0, 0] == lut[i] * (F32(1.0) / v3)
    # masks: zero, negative, NaN, +inf; a denormal is positive and finite: its gain is +inf
    Vm = np.array([[0.0, -1.0, np.nan, np.inf, 1e-40]], F32)
    g = pr.gain_np(Vm, Vm.shape)
    assert (g[0, :4] == -1).all() and np.isposinf(g[0, 4])
    o = pr.correct_np(np.array([[9, 9, 9, 9, 9]], np.uint8), lut, Vm)
    assert (o[0, :4] == -2).all() and np.isposinf(o[0, 4])
    assert np.isnan(pr.correct_np(np.array([[0]], np.uint8), lut, np.array([[1e-40]], F32))[0, 0])   # 0 * inf
    # a 3-channel pixel: the response is looked up with k_ingest's fixed-point luma, not per channel
    rgb = np.array([[[200, 30, 90]]], np.uint8)
    y = (200 * 4899 + 30 * 9617 + 90 * 1868 + 8192) >> 14
    assert pr.luma_u8(rgb)[0, 0] == y
    assert pr.correct_np(rgb, lut, np.array([[0.5]], F32))[0, 0] == lut[y] * F32(2.0)
    assert pr.correct_np(rgb)[0, 0] == raw_gray(rgb)[0, 0]
    rgba = np.array([[[200, 30, 90, 17]]], np.uint8)
    assert pr.correct_np(rgba, lut, None)[0, 0] == lut[y]


def test_gain_table_and_simulator():
    w, h = 24, 16
    V = pr.cos4_vignette(w, h, 0.4)
    assert abs(V.min() - 0.4) < 1e-6 and abs(V.max() - 1.0) < 1e-2
    t = pr.gain_table_np(V, w, h)
    assert t.shape == (4, 6) and t[1, 2] == F32(1.0) / V[4, 8]
    assert pr.gain_table_np(None, w, h).tobytes() == np.ones((4, 6), F32).tobytes()
    K = np.array([[20, 0, 11.5], [0, 20, 7.5], [0, 0, 1]], F32)
    tz = pr.gain_table_np(V, w, h, K, np.zeros(5, F32))          # a zero D maps every kept pixel onto itself
    assert tz.tobytes() == t.tobytes()
    M = pr.masked_vignette(64, 40)
    assert (M[36:] == 0).all() and (M[:36] > 0).all()
    # expose() then correct_np() recovers the irradiance up to the u8 rounding of the simulated camera
    e = np.linspace(0.05, 0.95, w * h).reshape(h, w)
    u8 = pr.expose(e, pr.gamma_forward(2.2), V)
    back = pr.correct_np(u8, pr.gamma_response(2.2).astype(F32), V)
    # one count of the u8 is d(irradiance) = 2.2 x^(1.2) / 255 <= 2.2 / 255 before the vignette is divided out (>= 0.4)
    assert np.abs(back - e).max() <= 0.5 * 2.2 / 255 / 0.4 + 1e-6


# ------------------------------------------------------------------------------------------------ the new kernels' resources
def test_new_kernels_compile_without_scratch():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "hipcc is needed to compile the kernels"
    cont = open(os.path.join(PKG, "Makefile")).read().split("FLAGS   =", 1)[1].split("\n")
    flags = (cont[0].rstrip("\\") + " " + cont[1]).split()
    flags = [f.replace("$(ARCH)", "gfx950") for f in flags if f != "-fPIC"]
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "k.s")
        subprocess.run([hipcc] + flags + ["-S", "--cuda-device-only", "-o", out, os.path.join(PKG, "csrc", "dvo_kernels.hip")],
                       check=True, capture_output=True, timeout=900)
        txt = open(out).read()
    checked = 0
    want = ["_ZN3dvo20k_pyramid_raw4_photoILi2ELb%dELb%dEE" % (p, l) for p in (0, 1) for l in (0, 1)] + \
           ["_ZN3dvo15k_pyramid_photoILb%dELb%dEE" % (p, r) for p in (0, 1) for r in (0, 1)] + ["_ZN3dvo17k_photometric_map"]
    for kernel in want:
        m = re.search(r"\.amdhsa_kernel %s\w*.*?\.end_amdhsa_kernel" % kernel, txt, re.S)
        assert m, "kernel not found: " + kernel
        body = m.group(0)
        scratch = int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body).group(1))
        vgpr = int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", body).group(1))
        lds = int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", body).group(1))
        assert scratch == 0, "%s spills %d bytes of scratch per lane" % (kernel, scratch)
        assert vgpr <= 64, "%s needs %d VGPRs: below eight waves per SIMD" % (kernel, vgpr)
        # the response row staged in LDS (1 KB) -- none in the plain-load form of the hot kernel and in the map kernel
        plain = kernel.endswith("Lb0EE") and "raw4" in kernel or "photometric_map" in kernel
        assert lds == (0 if plain else 1024), (kernel, lds)
        checked += 1
    assert checked == 9
