"""CPU tests of keyframe tracking for sensor-depth batches (include/dvo.h, dvo_batch_set_keyframe_tracking): the entry point is declared,
exported and bound, a NULL handle is refused before anything touches the GPU, the C++ facade's new methods compile, and the new
bookkeeping kernel needs no scratch and stays within the VGPRs of the kernel it mirrors (k_mono_decide_plan) plus one allocation unit."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

import dvo_amd as dvo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "direct-visual-odometry_amd")


def test_declared_exported_and_listed():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dvo.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+dvo_batch_set_keyframe_tracking\s*\(\s*dvo_batch\s*\*\s*\w+\s*,\s*int\s+\w+\s*\)\s*;", txt)
    assert hasattr(dvo.lib(), "dvo_batch_set_keyframe_tracking")
    assert "dvo_batch_set_keyframe_tracking" in dvo.EXPORTS


def test_the_batch_binds_it():
    for m in ("set_keyframe_tracking", "world_poses", "copy_world_poses_device", "keyframe"):
        assert callable(getattr(dvo.Batch, m, None)), m
    for m in ("world_poses", "copy_world_poses_device", "keyframe"):
        assert callable(getattr(dvo.MonoBatch, m, None)), m


def test_null_handle_is_refused():
    L = dvo.lib()
    assert L.dvo_batch_set_keyframe_tracking(None, 1) == dvo.DVO_ERR_BAD_ARGUMENT
    assert L.dvo_batch_set_keyframe_tracking(None, 0) == dvo.DVO_ERR_BAD_ARGUMENT
    assert L.dvo_batch_world_poses(None, None, None, None) == dvo.DVO_ERR_BAD_ARGUMENT
    assert L.dvo_batch_copy_world_poses_device(None, None, None, None) == dvo.DVO_ERR_BAD_ARGUMENT
    assert L.dvo_batch_keyframe_get(None, 0, 0, None, None, None, None, None, None, None, None) == dvo.DVO_ERR_BAD_ARGUMENT


def test_facade_keyframe_methods_compile(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("g++ not available")
    src = tmp_path / "snippet.cpp"
    src.write_text(r"""
#include "dvo.hpp"
#include <vector>
int use(float* xi_dev, float* T_dev, int* key_dev)
{
    const dvo::Mat3 K{525.f, 0.f, 319.5f, 0.f, 525.f, 239.5f, 0.f, 0.f, 1.f};
    dvo::BatchTracker bt(4, K, 640, 480);
    bt.setKeyframeTracking();
    bt.setKeyframeTracking(false);
    bt.setKeyframeTracking(true);
    std::vector<int> key;
    std::vector<dvo::Mat4> T = bt.worldPoses(&key);
    std::vector<dvo::Mat4> T2 = bt.worldPoses();
    bt.copyWorldPosesDevice(xi_dev, T_dev, key_dev);
    bt.copyWorldPosesDevice(xi_dev);
    dvo::Keyframe k = bt.keyframe(0);
    dvo::Keyframe k1 = bt.keyframe(1, 2);
    return (int)(T.size() + T2.size() + k.gray.size() + k1.depth.size()) + k.id + k1.width;
}
""")
    r = subprocess.run([gxx, "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def _meta(txt, name):
    m = re.search(r"\.amdhsa_kernel %s\n.*?\.end_amdhsa_kernel" % name, txt, re.S)
    assert m, "kernel not found: " + name
    body = m.group(0)
    return (int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", body).group(1)),
            int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body).group(1)))


def test_kf_decide_fits_the_budget():
    """k_kf_decide: no scratch, and at most one allocation unit (8 VGPRs) above k_mono_decide_plan, whose TRACK branch it runs."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    cont = open(os.path.join(PKG, "Makefile")).read().split("FLAGS   =", 1)[1].split("\n")
    flags = (cont[0].rstrip("\\") + " " + cont[1]).split()
    flags = [f.replace("$(ARCH)", "gfx950") for f in flags if f != "-fPIC"]
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "map.s")
        subprocess.run([hipcc] + flags + ["-S", "--cuda-device-only", "-o", out, os.path.join(PKG, "csrc", "dvo_map_kernels.hip")],
                       check=True, capture_output=True, timeout=900)
        asm = open(out).read()
    budget = _meta(asm, "_ZN3dvo18k_mono_decide_planENS_12MonoPlanArgsE")[0] + 8
    v, scratch = _meta(asm, "_ZN3dvo11k_kf_decideENS_12MonoPlanArgsE")
    assert scratch == 0, ("scratch", scratch)
    assert v <= budget, (v, budget)
