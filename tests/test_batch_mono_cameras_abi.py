"""CPU tests of the per-camera mono batch (include/dvo.h, dvo_batch_create_mono_cameras): the entry point is declared, exported and
bound, bad tables are refused before anything touches the GPU, the C++ facade's new BatchMono constructor compiles, and the
per-camera mapping kernels (k_depth_update_cam, k_propagate_owner_cam) need no scratch and no more VGPRs than the default ones."""
import ctypes as C
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import dvo_amd as dvo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "direct-visual-odometry_amd")
NAME = "dvo_batch_create_mono_cameras"
K640 = np.array([[525.0, 0.0, 319.5], [0.0, 525.0, 239.5], [0.0, 0.0, 1.0]], np.float32)


def _create(n, K, out=True):
    """dvo_batch_create_mono_cameras(n, K, 640, 480, 8, NULL, &out): (status, handle, dvo_last_error)"""
    L = dvo.lib()
    p = C.c_void_p()
    kp = K.ctypes.data_as(C.c_void_p) if K is not None else None
    st = L.dvo_batch_create_mono_cameras(n, kp, 640, 480, 8, None, C.byref(p) if out else None)
    return st, p, L.dvo_last_error().decode()


def test_create_mono_cameras_is_declared_exported_and_bound():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dvo.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+%s\s*\(\s*int\s+\w+\s*,\s*const\s+float\s*\*\s*\w+\s*,\s*int\s+\w+\s*,\s*int\s+\w+\s*,\s*int\s+\w+\s*,"
                     r"\s*const\s+dvo_config\s*\*\s*\w+\s*,\s*dvo_batch\s*\*\s*\*\s*\w+\s*\)" % NAME, txt)
    assert hasattr(dvo.lib(), NAME)
    assert NAME in dvo.EXPORTS


def test_null_out_and_null_K_are_refused():
    K = np.stack([K640] * 2)
    st, p, _ = _create(2, K, out=False)
    assert st == 1 and not p.value                 # DVO_ERR_BAD_ARGUMENT
    st, p, err = _create(2, None)
    assert st == 1 and not p.value
    assert NAME in err, err


@pytest.mark.parametrize("bad", ["nan", "inf", "fx0", "fy-", "fx-nan"])
def test_a_bad_table_is_refused_with_the_sequence_index(bad):
    K = np.stack([K640] * 4)
    q = {"nan": 2, "inf": 0, "fx0": 1, "fy-": 3, "fx-nan": 1}[bad]
    if bad == "nan":
        K[q, 1, 2] = np.nan
    elif bad == "inf":
        K[q, 2, 0] = np.inf
    elif bad == "fx0":
        K[q, 0, 0] = 0.0
    elif bad == "fy-":
        K[q, 1, 1] = -400.0
    else:
        K[q, 0, 0] = np.nan
    st, p, err = _create(4, K)
    assert st == 1 and not p.value, bad
    assert "sequence %d" % q in err, err


def test_python_table_shape_is_checked():
    with pytest.raises(ValueError):
        dvo.MonoBatch(3, np.stack([K640] * 2), 640, 480, per_sequence_K=True)
    with pytest.raises(dvo.DvoError, match="sequence 1"):
        K = np.stack([K640] * 3).reshape(3, 9)
        K[1, 4] = 0.0
        dvo.MonoBatch(3, K, 640, 480, per_sequence_K=True)


def test_facade_per_camera_constructor_compiles(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("g++ not available")
    src = tmp_path / "snippet.cpp"
    src.write_text(r"""
#include "dvo.hpp"
#include <vector>
int use()
{
    std::vector<dvo::Mat3> K(4, dvo::Mat3{525.f, 0.f, 319.5f, 0.f, 525.f, 239.5f, 0.f, 0.f, 1.f});
    K[1][0] = 400.f;
    dvo::BatchMono per_camera(4, K.data(), 640, 480);
    dvo::BatchMono shared(4, K[0], 640, 480, 8);
    return (int)per_camera.worldPoses().size() + (int)shared.worldPoses().size();
}
""")
    r = subprocess.run([gxx, "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def _meta(txt, name):
    m = re.search(r"\.amdhsa_kernel %s\n.*?\.end_amdhsa_kernel" % name, txt, re.S)
    assert m, "kernel not found: " + name
    body = m.group(0)
    return (int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", body).group(1)),
            int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body).group(1)))


def test_per_camera_mapping_kernels_fit_the_default_budget():
    """The per-sequence intrinsics arrive in SGPRs (scalar loads once per workgroup): no scratch, no VGPR above the defaults."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    cont = open(os.path.join(PKG, "Makefile")).read().split("FLAGS   =", 1)[1].split("\n")
    flags = (cont[0].rstrip("\\") + " " + cont[1]).split()
    flags = [f.replace("$(ARCH)", "gfx950") for f in flags if f != "-fPIC"]
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "m.s")
        subprocess.run([hipcc] + flags + ["-S", "--cuda-device-only", "-o", out, os.path.join(PKG, "csrc", "dvo_map_kernels.hip")],
                       check=True, capture_output=True, timeout=900)
        txt = open(out).read()
    for default, cam in (("_ZN3dvo14k_depth_updateENS_10UpdateArgsE", "_ZN3dvo18k_depth_update_camENS_10UpdateArgsE"),
                         ("_ZN3dvo17k_propagate_ownerENS_8PropArgsE", "_ZN3dvo21k_propagate_owner_camENS_8PropArgsE")):
        v0, s0 = _meta(txt, default)
        v1, s1 = _meta(txt, cam)
        assert s1 == 0, "%s spills %d bytes of scratch per lane" % (cam, s1)
        assert v1 <= v0, "%s needs %d VGPRs, the default %d" % (cam, v1, v0)
