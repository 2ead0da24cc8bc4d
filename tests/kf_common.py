"""What tests/test_gpu_kf_fusion.py and tests/test_gpu_kf_carry.py share: the batch shape and constants, the renders, the action
schedules, the per-sequence cameras and the feeds (each test file keeps its own SIZE, keyframe_max_frames and action mix); and what
tests/test_kf_fusion_abi.py and tests/test_kf_carry_abi.py share: the register pins of the kernels in csrc/dvo_map_kernels.hip."""
import functools
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import dvo_amd as dvo
from dvo_amd import synth
from util import K640

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "direct-visual-odometry_amd")
SKIP, TRACK, RESTART = dvo.SEQ_SKIP, dvo.SEQ_TRACK, dvo.SEQ_RESTART
TRACKED, SKIPPED, STARTED = dvo.SEQ_TRACKED, dvo.SEQ_SKIPPED, dvo.SEQ_STARTED
LEVELS, CULLS, TOP = 3, 1, 2
STEPS = (1.0, 0.75, 0.5)
KH = np.array(K640, np.float32).copy()
KH[0] *= 0.5
KH[1] *= 0.5
MAX_DIFF, MAX_COUNT = 0.05, 16


@functools.lru_cache(maxsize=None)
def _map_kernels_asm():
    """the device assembly of csrc/dvo_map_kernels.hip under the Makefile's flags, compiled once per run"""
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
        return open(out).read()


def assert_map_kernels_fit(budgets):
    """every (mangled kernel name, VGPR budget): no scratch, no LDS, and the VGPRs within the budget"""
    asm = _map_kernels_asm()
    for name, budget in budgets:
        m = re.search(r"\.amdhsa_kernel %s\n.*?\.end_amdhsa_kernel" % name, asm, re.S)
        assert m, "kernel not found: " + name
        g = lambda k: int(re.search(r"\.amdhsa_%s (\d+)" % k, m.group(0)).group(1))
        v, scratch, lds = g("next_free_vgpr"), g("private_segment_fixed_size"), g("group_segment_fixed_size")
        assert scratch == 0 and lds == 0, (name, scratch, lds)
        assert v <= budget, (name, v, budget)


def cfg(max_frames, **kw):
    kw.setdefault("max_iterations", 6)
    kw.setdefault("keyframe_min_translation", 1.0)
    kw.setdefault("keyframe_max_frames", max_frames)
    return dvo.default_config(gn_pixels_per_thread=4, crop_enable=0, step_default=STEPS[0], step_level1=STEPS[1], step_level2=STEPS[2],
                              min_residual=0.0, min_update=2e-5, **kw)


def holes(d):
    """0, NaN, +inf, below min_depth and a 0.3 m step block in every frame: in the keyframes and in the tracked / promoting frames"""
    d = d.copy()
    d[:, 20:40, 30:60] = 0.0
    d[:, 100:110, 200:230] = np.nan
    d[:, 150:156, 40:80] = np.inf
    d[:, 60:120, 120:180] += np.float32(0.3)
    d[:, 200:204, 100:140] = 0.1
    return d


@functools.lru_cache(maxsize=None)
def frames(size, noise=0.0, with_holes=False, big=False):
    """six renders (gray, depth, sigma), computed once per option set and read-only; big: larger steps between them"""
    kw = dict(sigma_t=0.02, sigma_r_deg=1.2) if big else {}
    g, d, s, _ = synth.sequence(6, width=size[0], height_px=size[1], K=KH, seed=42, sigma_value=0.5, **kw)
    g, d, s = g.numpy(), d.numpy(), s.numpy()
    if noise:
        d = (d + np.random.RandomState(7).normal(0.0, noise, d.shape)).astype(np.float32)
    if with_holes:
        d = holes(d)
    for a in (g, d, s):
        a.setflags(write=False)
    return g, d, s


def dev(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return t


def idx(B, pushes):
    return [[(k + b) % 6 for b in range(B)] for k in range(pushes)]


def acts(B, n, seed, p):
    """p: the probabilities of SKIP, TRACK and RESTART"""
    rng = np.random.RandomState(seed)
    a = rng.choice([SKIP, TRACK, RESTART], size=(n, B), p=p).astype(np.uint8)
    a[0] = TRACK
    a[0, B - 1] = SKIP          # one sequence starts late: its keyframe does not exist after the first push
    return a


def cams(B):
    c = np.tile(KH.reshape(1, 9), (B, 1)).astype(np.float32)
    c[:, 0] *= 1.0 + 0.01 * np.arange(B); c[:, 4] *= 1.0 - 0.008 * np.arange(B)
    c[:, 2] += 0.7 * np.arange(B); c[:, 5] -= 0.4 * np.arange(B)
    return c


def push(bt, keep, maps, feed):
    gi, di, si = maps
    if feed == "host":
        bt.push_host(gi, di, si)
    elif feed in ("raw", "raw_host"):
        with np.errstate(invalid="ignore"):   # (a NaN or +inf hole is a 0 of the sensor)
            g8 = np.clip(np.rint(gi * 255), 0, 255).astype(np.uint8)
            d16 = np.clip(np.rint(np.nan_to_num(di, nan=0.0, posinf=0.0) * 5000), 0, 65535).astype(np.uint16)
        if feed == "raw_host":
            bt.push_raw_host(g8, d16)
        else:
            import torch
            tg = dev(g8); td = torch.from_numpy(d16.view(np.int16)).cuda()
            torch.cuda.synchronize()
            keep.append((tg, td))
            bt.push_raw_device(tg.data_ptr(), 1, td.data_ptr())
    else:
        t = [dev(x) for x in maps]
        keep.append(t)
        bt.push_device(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr())
