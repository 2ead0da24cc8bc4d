"""CPU tests of per-sequence skip and restart on a mono batch (include/dvo.h, dvo_batch_set_mono_actions and its three companions):
the entry points are declared, exported and bound, a NULL handle is refused before anything touches the GPU, the C++ facade's new
BatchMono methods compile, and the plan kernels of a mono call need no scratch and stay within the VGPR budget of the kernels they
stand in for."""
import ctypes as C
import os
import re
import shutil
import subprocess
import tempfile

import pytest

import dvo_amd as dvo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "direct-visual-odometry_amd")
NAMES = ["dvo_batch_set_mono_actions", "dvo_batch_mono_last_status", "dvo_batch_copy_mono_status_device",
         "dvo_batch_set_mono_start_depth_device"]
SIGNATURES = {
    "dvo_batch_set_mono_actions": r"dvo_batch\s*\*\s*\w+\s*,\s*const\s+uint8_t\s*\*\s*\w+\s*,\s*int\s+\w+",
    "dvo_batch_mono_last_status": r"dvo_batch\s*\*\s*\w+\s*,\s*int\s*\*\s*\w+",
    "dvo_batch_copy_mono_status_device": r"dvo_batch\s*\*\s*\w+\s*,\s*int\s*\*\s*\w+",
    "dvo_batch_set_mono_start_depth_device": r"dvo_batch\s*\*\s*\w+\s*,\s*const\s+float\s*\*\s*\w+\s*,\s*const\s+float\s*\*\s*\w+",
}


@pytest.mark.parametrize("name", NAMES)
def test_declared_exported_and_listed(name):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dvo.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+%s\s*\(\s*%s\s*\)\s*;" % (name, SIGNATURES[name]), txt), name
    assert hasattr(dvo.lib(), name)
    assert name in dvo.EXPORTS


def test_mono_batch_binds_them():
    for m in ("set_actions", "last_status", "copy_status_device", "set_start_depth_device"):
        assert callable(getattr(dvo.MonoBatch, m, None)), m


def test_null_handle_is_refused():
    L = dvo.lib()
    st = C.c_int(0)
    buf = (C.c_uint8 * 4)()
    assert L.dvo_batch_set_mono_actions(None, buf, 0) == 1               # DVO_ERR_BAD_ARGUMENT
    assert L.dvo_batch_set_mono_actions(None, None, 0) == 1
    assert L.dvo_batch_mono_last_status(None, C.byref(st)) == 1
    assert L.dvo_batch_copy_mono_status_device(None, C.byref(st)) == 1
    assert L.dvo_batch_set_mono_start_depth_device(None, None, None) == 1


def test_facade_mono_lifecycle_methods_compile(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("g++ not available")
    src = tmp_path / "snippet.cpp"
    src.write_text(r"""
#include "dvo.hpp"
#include <vector>
int use(const float* depth_dev, const float* sigma_dev, int* status_dev, const uint8_t* actions_dev)
{
    dvo::BatchMono mb(4, dvo::Mat3{525.f, 0.f, 319.5f, 0.f, 525.f, 239.5f, 0.f, 0.f, 1.f}, 640, 480);
    std::vector<uint8_t> act = {DVO_SEQ_SKIP, DVO_SEQ_TRACK, DVO_SEQ_RESTART, DVO_SEQ_TRACK};
    mb.setActions(act.data());
    mb.setActions(actions_dev, true);
    mb.setActions(nullptr);
    mb.setStartDepthDevice(depth_dev, sigma_dev);
    mb.setStartDepthDevice(nullptr, nullptr);
    mb.copyStatusDevice(status_dev);
    std::vector<int> st = mb.lastStatus();
    return (int)st.size();
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


def _device_asm(src, td):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    cont = open(os.path.join(PKG, "Makefile")).read().split("FLAGS   =", 1)[1].split("\n")
    flags = (cont[0].rstrip("\\") + " " + cont[1]).split()
    flags = [f.replace("$(ARCH)", "gfx950") for f in flags if f != "-fPIC"]
    out = os.path.join(td, os.path.basename(src) + ".s")
    subprocess.run([hipcc] + flags + ["-S", "--cuda-device-only", "-o", out, os.path.join(PKG, "csrc", src)],
                   check=True, capture_output=True, timeout=900)
    return open(out).read()


# (plan kernel, the plain kernel it stands in for, VGPRs allowed above it).  The per-pixel kernels stay within the plain budget.  The
# two per-sequence kernels run one thread per sequence, once per call: k_mono_decide_plan holds each sequence's own frame id in a VGPR
# (k_mono_decide's is a kernel argument) and k_mono_commit_plan has three branches where k_mono_commit has two; they may use up to
# one allocation unit (8 VGPRs) more.
PAIRS = [
    ("dvo_map_kernels.hip", "_ZN3dvo28k_regularize_redecimate_planENS_10RegDecArgsENS_13MonoStartArgsE",
     "_ZN3dvo23k_regularize_redecimateENS_10RegDecArgsE", 0),
    ("dvo_kernels.hip", "_ZN3dvo20k_pyramid_remap_planENS_11PyramidArgsE", "_ZN3dvo15k_pyramid_remapENS_11PyramidArgsE", 0),
    ("dvo_map_kernels.hip", "_ZN3dvo18k_mono_decide_planENS_12MonoPlanArgsE",
     "_ZN3dvo13k_mono_decideEPNS_7MonoSeqEPKNS_8SeqStateEiifiPfS5_PiNS_7MonoRefES6_", 8),
    ("dvo_map_kernels.hip", "_ZN3dvo18k_mono_commit_planENS_12MonoPlanArgsE",
     "_ZN3dvo13k_mono_commitEPNS_7MonoSeqEPfiiiiS2_S2_Pi", 8),
]


def test_plan_kernels_fit_the_plain_budget():
    """No scratch, and no more VGPRs than the plain kernel each one replaces in a planned mono call (plus the slack above)."""
    with tempfile.TemporaryDirectory() as td:
        asm = {src: _device_asm(src, td) for src in sorted({p[0] for p in PAIRS})}
    for src, plan, plain, slack in PAIRS:
        v1, s1 = _meta(asm[src], plan)
        v0, _ = _meta(asm[src], plain)
        assert s1 == 0, (plan, "scratch", s1)
        assert v1 <= v0 + slack, (plan, v1, plain, v0)
