"""CPU tests of the lens undistortion fused into the sensor-depth batch (include/dvo.h: dvo_batch_set_sensor_distortion,
dvo_batch_get_sensor_distortion): the entry points are declared, exported and bound, a NULL handle is refused before anything touches
the GPU, the C++ facade's new methods compile, and -- compiled for gfx950 -- the new k_pyramid_remap_depth instances need no scratch
and stay within their VGPR budget while the mono remap kernels keep their instruction streams (tests/golden/isa_sensor_undistort.json,
recorded with tools/isa_compare.py's normalisation from the parent commit)."""
import ctypes as C
import hashlib
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import dvo_amd as dvo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "direct-visual-odometry_amd")
NAMES = ("dvo_batch_set_sensor_distortion", "dvo_batch_get_sensor_distortion")
# k_pyramid_remap_depth<PPT, PLAN>: four kept pixels per thread (PPT = 4) and the scalar fallback, without and with the plan
NEW_KERNELS = {"_ZN3dvo21k_pyramid_remap_depthILi%dELb%dEEEvNS_11PyramidArgsE" % (p, q): p for p in (4, 1) for q in (0, 1)}
# VGPR budget: at most 32 (the kernels are memory bound; 32 leaves every SIMD its full 16 waves -- measured 30 at PPT = 4, 14 at PPT = 1)
VGPR_BUDGET = 32


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dvo.h")).read(), flags=re.S)


def test_entry_points_are_declared_exported_and_bound():
    txt = _header()
    assert re.search(r"\bint\s+dvo_batch_set_sensor_distortion\s*\(\s*dvo_batch\s*\*\s*\w+\s*,\s*const\s+float\s*\*\s*\w+\s*,\s*int\s+\w+\s*\)", txt)
    assert re.search(r"\bint\s+dvo_batch_get_sensor_distortion\s*\(\s*dvo_batch\s*\*\s*\w+\s*,\s*float\s*\*\s*\w+\s*,\s*int\s*\*\s*\w+\s*\)", txt)
    L = dvo.lib()
    for n in NAMES:
        assert hasattr(L, n), n
        assert n in dvo.EXPORTS, n
    nm = shutil.which("nm")
    if nm:
        out = subprocess.run([nm, "-D", "--defined-only", dvo.LIB_PATH], capture_output=True, text=True, check=True).stdout
        for n in NAMES:
            assert re.search(r"\bT %s$" % n, out, re.M), n


def test_null_handle_is_refused():
    L = dvo.lib()
    D = np.zeros(5, np.float32)
    dp = D.ctypes.data_as(C.c_void_p)
    assert L.dvo_batch_set_sensor_distortion(None, dp, 0) == 1          # DVO_ERR_BAD_ARGUMENT
    assert L.dvo_batch_set_sensor_distortion(None, dp, 1) == 1
    assert L.dvo_batch_set_sensor_distortion(None, None, 0) == 1
    en = C.c_int(7)
    assert L.dvo_batch_get_sensor_distortion(None, dp, C.byref(en)) == 1
    assert L.dvo_batch_get_sensor_distortion(None, None, None) == 1
    assert en.value == 7


def test_facade_methods_compile(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("g++ not available")
    src = tmp_path / "snippet.cpp"
    src.write_text(r"""
#include "dvo.hpp"
#include <array>
#include <vector>
int use()
{
    const dvo::Mat3 K{517.3f, 0.f, 318.6f, 0.f, 516.5f, 255.3f, 0.f, 0.f, 1.f};
    const std::array<float, 5> D{0.2624f, -0.9531f, -0.0054f, 0.0026f, 1.1633f};
    dvo::BatchTracker b(4, K, 640, 480);
    b.setDistortion(D.data());
    std::vector<float> per(4 * 5, 0.f);
    b.setDistortion(per.data(), true);
    b.setDistortion(nullptr);
    std::vector<std::array<float, 5>> got = b.distortion();
    return (int)got.size();
}
""")
    r = subprocess.run([gxx, "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_python_shapes_are_checked_before_the_library():
    bt = dvo.Batch.__new__(dvo.Batch)
    bt.n_seq = 3
    with pytest.raises(ValueError):
        bt.set_distortion(np.zeros((2, 5), np.float32))
    with pytest.raises(ValueError):
        bt.set_distortion(np.zeros(6, np.float32))


@pytest.fixture(scope="module")
def kernels_asm():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    cont = open(os.path.join(PKG, "Makefile")).read().split("FLAGS   =", 1)[1].split("\n")
    flags = (cont[0].rstrip("\\") + " " + cont[1]).split()
    flags = [f.replace("$(ARCH)", "gfx950") for f in flags if f != "-fPIC"]
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "k.s")
        subprocess.run([hipcc] + flags + ["-S", "--cuda-device-only", "-o", out, os.path.join(PKG, "csrc", "dvo_kernels.hip")],
                       check=True, capture_output=True, timeout=1800)
        return open(out).read()


def _isa_tools():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import isa_compare
    finally:
        sys.path.pop(0)
    return isa_compare


def _parse(I, txt):
    with tempfile.NamedTemporaryFile("w", suffix=".s", delete=False) as f:
        f.write(txt)
    try:
        return I.kernels(f.name)
    finally:
        os.unlink(f.name)


def test_new_kernels_use_no_scratch_within_vgpr_budget(kernels_asm):
    I = _isa_tools()
    body, meta = _parse(I, kernels_asm)
    for name, ppt in NEW_KERNELS.items():
        assert name in meta, name
        vgprs, _, scratch = meta[name]
        assert scratch == 0, "%s spills %d bytes of scratch per lane" % (name, scratch)
        assert vgprs <= VGPR_BUDGET, "%s: %d VGPRs" % (name, vgprs)
        if ppt == 4:   # the four-pixel form reads four table entries with one 16-byte load and stores the top level 16 bytes at a time
            assert re.search(r"global_load_dwordx4", body[name]), name
            assert re.search(r"global_store_dwordx4", body[name]), name


def test_mono_remap_kernels_are_instruction_identical(kernels_asm):
    I = _isa_tools()
    body, _ = _parse(I, kernels_asm)
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "isa_sensor_undistort.json")))
    assert len(want) == 2   # k_pyramid_remap, k_undistort_map
    for name, rec in want.items():
        assert name in body, name
        got = I.norm(body[name])
        assert len(got.split("\n")) == rec["instructions"], name
        assert hashlib.sha256(got.encode()).hexdigest() == rec["sha256"], "%s: instruction stream changed" % name
