"""CPU tests of the lens undistortion fused into the mono ingest (include/dvo.h: dvo_batch_set_distortion, dvo_batch_get_distortion,
dvo_vo_set_distortion): the entry points are declared, exported and bound, a NULL handle is refused before anything touches the GPU,
the C++ facade's new methods compile, and -- compiled for gfx950 -- the new kernels need no scratch while k_undistort, k_pyramid and
every k_pyramid_raw4 instance keep the instruction stream of the parent commit (tests/golden/isa_pyramid_undistort.json, recorded
with tools/isa_compare.py's normalisation before the remap arithmetic moved into dvo_math.h)."""
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
NAMES = ("dvo_batch_set_distortion", "dvo_batch_get_distortion", "dvo_vo_set_distortion")


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dvo.h")).read(), flags=re.S)


def test_entry_points_are_declared_exported_and_bound():
    txt = _header()
    assert re.search(r"\bint\s+dvo_batch_set_distortion\s*\(\s*dvo_batch\s*\*\s*\w+\s*,\s*const\s+float\s*\*\s*\w+\s*,\s*int\s+\w+\s*\)", txt)
    assert re.search(r"\bint\s+dvo_batch_get_distortion\s*\(\s*dvo_batch\s*\*\s*\w+\s*,\s*float\s*\*\s*\w+\s*,\s*int\s*\*\s*\w+\s*\)", txt)
    assert re.search(r"\bint\s+dvo_vo_set_distortion\s*\(\s*dvo_vo\s*\*\s*\w+\s*,\s*const\s+float\s+\w+\s*\[\s*5\s*\]\s*\)", txt)
    L = dvo.lib()
    for n in NAMES:
        assert hasattr(L, n), n
        assert n in dvo.EXPORTS, n


def test_null_handle_is_refused():
    L = dvo.lib()
    D = np.zeros(5, np.float32)
    dp = D.ctypes.data_as(C.c_void_p)
    assert L.dvo_batch_set_distortion(None, dp, 0) == 1            # DVO_ERR_BAD_ARGUMENT
    assert L.dvo_batch_set_distortion(None, None, 0) == 1
    en = C.c_int(7)
    assert L.dvo_batch_get_distortion(None, dp, C.byref(en)) == 1
    assert L.dvo_vo_set_distortion(None, dp) == 1
    assert L.dvo_vo_set_distortion(None, None) == 1


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
    const dvo::Mat3 K{780.f, 0.f, 378.f, 0.f, 796.f, 220.f, 0.f, 0.f, 1.f};
    const std::array<float, 5> D{-0.0462f, 0.152f, -0.00429f, 0.0117f, -0.0725f};
    dvo::VisualOdometry vo(K, 640, 480);
    vo.setDistortion(D);
    dvo::BatchMono b(4, K, 640, 480);
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
    mb = dvo.MonoBatch.__new__(dvo.MonoBatch)
    mb.n_seq = 3
    with pytest.raises(ValueError):
        mb.set_distortion(np.zeros((2, 5), np.float32))
    with pytest.raises(ValueError):
        mb.set_distortion(np.zeros(4, np.float32))
    vo = dvo.VisualOdometry.__new__(dvo.VisualOdometry)
    with pytest.raises(ValueError):
        vo.setDistortion(np.zeros(6, np.float32))


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


def test_new_kernels_use_no_scratch(kernels_asm):
    I = _isa_tools()
    _, meta = _parse(I, kernels_asm)
    for name in ("_ZN3dvo15k_pyramid_remapENS_11PyramidArgsE", "_ZN3dvo15k_undistort_mapEPKNS_12UndistortCamEiiiiiiPi"):
        assert name in meta, name
        assert meta[name][2] == 0, "%s spills %d bytes of scratch per lane" % (name, meta[name][2])


def _parse(I, txt):
    with tempfile.NamedTemporaryFile("w", suffix=".s", delete=False) as f:
        f.write(txt)
    try:
        return I.kernels(f.name)
    finally:
        os.unlink(f.name)


def test_existing_pyramid_and_undistort_kernels_are_instruction_identical(kernels_asm):
    I = _isa_tools()
    body, _ = _parse(I, kernels_asm)
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "isa_pyramid_undistort.json")))
    assert len(want) == 7   # k_undistort, k_pyramid<false/true>, k_pyramid_raw4<1/2, false/true>
    for name, rec in want.items():
        assert name in body, name
        got = I.norm(body[name])
        assert len(got.split("\n")) == rec["instructions"], name
        assert hashlib.sha256(got.encode()).hexdigest() == rec["sha256"], "%s: instruction stream changed" % name
