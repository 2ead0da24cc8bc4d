"""CPU tests of the per-sequence start pose of a batch's tracking (include/dvo.h, dvo_batch_set_pose_guess_mode and its two
companions): the entry points are declared, exported and bound, a NULL handle is refused before anything touches the GPU, the C++
facade's new methods compile, and the two seed kernels need no scratch and stay within the VGPR budget of the per-sequence kernels
they run beside (k_plan, k_mono_decide_plan) plus one allocation unit."""
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
NAMES = ["dvo_batch_set_pose_guess_mode", "dvo_batch_set_pose_guess", "dvo_batch_last_start_poses"]
SIGNATURES = {
    "dvo_batch_set_pose_guess_mode": r"dvo_batch\s*\*\s*\w+\s*,\s*int\s+\w+",
    "dvo_batch_set_pose_guess": r"dvo_batch\s*\*\s*\w+\s*,\s*const\s+float\s*\*\s*\w+\s*,\s*int\s+\w+",
    "dvo_batch_last_start_poses": r"dvo_batch\s*\*\s*\w+\s*,\s*float\s*\*\s*\w+",
}


@pytest.mark.parametrize("name", NAMES)
def test_declared_exported_and_listed(name):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dvo.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+%s\s*\(\s*%s\s*\)\s*;" % (name, SIGNATURES[name]), txt), name
    assert hasattr(dvo.lib(), name)
    assert name in dvo.EXPORTS


def test_modes_are_declared():
    txt = open(os.path.join(ROOT, "include", "dvo.h")).read()
    for name, v in (("DVO_GUESS_NONE", 0), ("DVO_GUESS_GIVEN", 1), ("DVO_GUESS_CONSTANT_VELOCITY", 2)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, v), txt), name
    assert (dvo.GUESS_NONE, dvo.GUESS_GIVEN, dvo.GUESS_CONSTANT_VELOCITY) == (0, 1, 2)


def test_both_batches_bind_them():
    for cls in (dvo.Batch, dvo.MonoBatch):
        for m in ("set_pose_guess_mode", "set_pose_guess", "last_start_poses"):
            assert callable(getattr(cls, m, None)), (cls.__name__, m)


def test_null_handle_is_refused():
    L = dvo.lib()
    rows = (C.c_float * 12)()
    assert L.dvo_batch_set_pose_guess_mode(None, 0) == 1                  # DVO_ERR_BAD_ARGUMENT
    assert L.dvo_batch_set_pose_guess_mode(None, 2) == 1
    assert L.dvo_batch_set_pose_guess_mode(None, 7) == 1
    assert L.dvo_batch_set_pose_guess(None, rows, 0) == 1
    assert L.dvo_batch_set_pose_guess(None, None, 0) == 1
    assert L.dvo_batch_last_start_poses(None, rows) == 1


def test_facade_pose_guess_methods_compile(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("g++ not available")
    src = tmp_path / "snippet.cpp"
    src.write_text(r"""
#include "dvo.hpp"
#include <vector>
int use(const float* rows_dev)
{
    const dvo::Mat3 K{525.f, 0.f, 319.5f, 0.f, 525.f, 239.5f, 0.f, 0.f, 1.f};
    dvo::BatchTracker bt(4, K, 640, 480);
    std::vector<float> rows(4 * 6, 0.0f);
    bt.setPoseGuessMode(DVO_GUESS_GIVEN);
    bt.setPoseGuess(rows.data());
    bt.setPoseGuess(rows_dev, true);
    bt.setPoseGuess(nullptr);
    std::vector<std::array<float, 6>> s0 = bt.lastStartPoses();
    dvo::BatchMono mb(4, K, 640, 480);
    mb.setPoseGuessMode(DVO_GUESS_CONSTANT_VELOCITY);
    mb.setPoseGuessMode(DVO_GUESS_GIVEN);
    mb.setPoseGuess(rows.data());
    std::vector<std::array<float, 6>> s1 = mb.lastStartPoses();
    return (int)(s0.size() + s1.size());
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


# The seed kernels and the per-sequence kernels they run beside.  Each seed does k_set_pose's work (pose_from_xi in float, se3_exp_d in
# double), so its register count is set by the double exp, not by the plan: the budget is the larger of k_plan and k_mono_decide_plan,
# plus one allocation unit (8 VGPRs).  One thread per sequence, once per push.
SEEDS = [("dvo_kernels.hip", "_ZN3dvo11k_seed_poseENS_12PoseSeedArgsE"),
         ("dvo_map_kernels.hip", "_ZN3dvo11k_mono_seedENS_12PoseSeedArgsE")]
BUDGET = [("dvo_kernels.hip", "_ZN3dvo6k_planENS_8PlanArgsE"),
          ("dvo_map_kernels.hip", "_ZN3dvo18k_mono_decide_planENS_12MonoPlanArgsE")]


def test_seed_kernels_fit_the_budget():
    """No scratch, and at most one allocation unit above the larger of k_plan and k_mono_decide_plan."""
    with tempfile.TemporaryDirectory() as td:
        asm = {src: _device_asm(src, td) for src in ("dvo_kernels.hip", "dvo_map_kernels.hip")}
    budget = max(_meta(asm[src], k)[0] for src, k in BUDGET) + 8
    for src, seed in SEEDS:
        v, scratch = _meta(asm[src], seed)
        assert scratch == 0, (seed, "scratch", scratch)
        assert v <= budget, (seed, v, budget)
