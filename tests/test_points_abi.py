"""CPU tests of the keyframe point-cloud export (include/dvo.h, dvo_batch_export_points): the entry points are
declared, exported and bound, the argument block has the layout the binding assumes, the default configuration is the documented one,
NULL arguments are refused before anything touches the GPU, the header states the contract, the C++ facade compiles, the replica
(tests/points_ref.py) keeps its anchors, and the new kernels need no scratch and stay within the VGPRs measured when they were written
(k_points_prep 46, k_points_count 28, k_points_scan 14, k_points_write / _cam 73) plus one allocation unit of 8."""
import ctypes as C
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import dvo_amd as dvo
import points_ref as pref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "direct-visual-odometry_amd")
NAMES = ("dvo_points_config_default", "dvo_batch_export_points", "dvo_batch_last_points")
F32 = np.float32
ALL, NEW = dvo.POINTS_ALL, dvo.POINTS_NEW   # (without the feature the file fails here, at import)


def _header():
    return open(os.path.join(ROOT, "include", "dvo.h")).read()


def test_declared_exported_and_listed():
    txt = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert re.search(r"#define\s+DVO_POINTS_ALL\s+0\b", txt) and re.search(r"#define\s+DVO_POINTS_NEW\s+1\b", txt)
    assert re.search(r"typedef\s+struct\s+dvo_points_config\s*\{\s*int\s+struct_size;\s*int\s+select;\s*int\s+level;\s*int\s+stride;\s*"
                     r"float\s+min_depth,\s*max_depth;\s*float\s+max_sigma;\s*float\s+min_age;\s*int\s+min_count;\s*\}\s*dvo_points_config;", txt)
    assert re.search(r"\bvoid\s+dvo_points_config_default\s*\(\s*dvo_points_config\s*\*", txt)
    assert re.search(r"\bint\s+dvo_batch_export_points\s*\(\s*dvo_batch\s*\*\s*\w+\s*,\s*const\s+dvo_points_config\s*\*\s*\w+\s*,\s*uint32_t\s+"
                     r"\w+\s*,\s*float\s*\*\s*\w+\s*,\s*uint32_t\s*\*\s*\w+\s*,\s*float\s*\*\s*\w+\s*,\s*uint32_t\s*\*\s*\w+\s*\)", txt)
    assert re.search(r"\bint\s+dvo_batch_last_points\s*\(\s*dvo_batch\s*\*\s*\w+\s*,\s*uint32_t\s*\*", txt)
    for n in NAMES:
        assert hasattr(dvo.lib(), n), n
        assert n in dvo.EXPORTS, n
    assert "dvo_*" in open(os.path.join(PKG, "csrc", "libdvo.map")).read()   # (the map exports the C ABI by its prefix)
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for n in NAMES:
        assert n in integration, n


def test_the_header_states_the_contract():
    txt = " ".join(" ".join(re.sub(r"^\s*\*\s", "", ln) for ln in _header().splitlines()).split())   # (comment lines joined)
    for phrase in ("x % stride == 0 && y % stride == 0", "d >= min_depth && d <= max_depth (false for NaN / inf)",
                   "sequences in index order, within a sequence raster order", "src[i] = y * w_l + x",
                   "xyzg[i] = (Xw, Yw, Zw, gray[level][y][x])", "offsets[n_seq] = the total", "dvo_op_se3_exp(-ref_xi)",
                   "back_project(k_l, (float)x, (float)y, d)", "transform(Wk, ...)", "nothing at or past capacity is touched",
                   "capacity = 0 with NULL xyzg / src / sigma is the counting call", "n_seq * w_l * h_l > 2^31 - 1",
                   "changes nothing in the handle's maps", "runs exactly the launches it always ran"):
        assert phrase in txt, phrase


def test_default_config_and_struct_layout():
    c = dvo.PointsConfig()
    dvo.lib().dvo_points_config_default(C.byref(c))
    assert C.sizeof(dvo.PointsConfig) == 36 and c.struct_size == 36
    assert [f[0] for f in dvo.PointsConfig._fields_] == ["struct_size", "select", "level", "stride", "min_depth", "max_depth", "max_sigma",
                                                         "min_age", "min_count"]
    assert [getattr(dvo.PointsConfig, f[0]).offset for f in dvo.PointsConfig._fields_] == list(range(0, 36, 4))
    # every started sequence, the top level (-1), stride 1, the handle's min_depth (< 0), max_depth +inf and no other gate
    assert (c.select, c.level, c.stride, c.min_count) == (ALL, -1, 1, 0)
    assert c.min_depth < 0 and c.max_depth == np.inf and c.max_sigma == np.inf and c.min_age == 0.0
    dvo.lib().dvo_points_config_default(None)
    assert (dvo.POINTS_ALL, dvo.POINTS_NEW) == (0, 1)
    k = dvo.points_config(stride=2, select=NEW)
    assert (k.stride, k.select, k.struct_size) == (2, NEW, 36)
    with pytest.raises(AttributeError):
        dvo.points_config(nope=1)


def test_both_batch_kinds_bind_it():
    for cls in (dvo.Batch, dvo.MonoBatch):
        for m in ("export_points", "last_points", "export_points_torch"):
            assert callable(getattr(cls, m, None)), (cls, m)


def test_null_arguments_are_refused():
    L = dvo.lib()
    c = dvo.points_config()
    off = (C.c_uint32 * 4)()
    assert L.dvo_batch_export_points(None, C.byref(c), 0, None, None, None, off) == dvo.DVO_ERR_BAD_ARGUMENT
    assert L.dvo_batch_export_points(None, None, 0, None, None, None, None) == dvo.DVO_ERR_BAD_ARGUMENT
    assert L.dvo_batch_last_points(None, off) == dvo.DVO_ERR_BAD_ARGUMENT
    assert L.dvo_batch_last_points(None, None) == dvo.DVO_ERR_BAD_ARGUMENT


def test_facade_compiles(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("g++ not available")
    src = tmp_path / "snippet.cpp"
    src.write_text(r"""
#include "dvo.hpp"
#include <vector>
int use(float* xyzg, uint32_t* idx, float* sigma, uint32_t* off)
{
    const dvo::Mat3 K{525.f, 0.f, 319.5f, 0.f, 525.f, 239.5f, 0.f, 0.f, 1.f};
    dvo_points_config c;
    dvo_points_config_default(&c);
    c.select = DVO_POINTS_NEW; c.stride = 2;
    dvo::BatchTracker bt(4, K, 640, 480);
    bt.setKeyframeTracking();
    bt.exportPoints(c, 1000u, xyzg, idx, off);
    std::vector<uint32_t> a = bt.lastPoints();
    dvo::BatchMono bm(4, K, 640, 480);
    bm.exportPoints(c, 0u, nullptr, nullptr, nullptr, off);
    bm.exportPoints(c, 1000u, xyzg, idx, sigma, off);
    std::vector<uint32_t> b = bm.lastPoints();
    return (int)(a.size() + b.size());
}
""")
    r = subprocess.run([gxx, "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


# ---- the replica's anchors ------------------------------------------------------------------------------------------------------
K_L = np.array([[131.25, 0, 39.875], [0, 131.25, 29.875], [0, 0, 1]], F32)
EYE = np.eye(4, dtype=F32)


def _maps(h=7, w=9, seed=0):
    rng = np.random.RandomState(seed)
    d = (1.0 + rng.rand(h, w)).astype(F32)
    g = rng.rand(h, w).astype(F32)
    return d, g


def test_replica_order_and_identity():
    d, g = _maps()
    d[2, 3] = np.nan; d[4, 5] = np.inf; d[0, 0] = 0.1; d[6, 8] = -2.0
    xyzg, src, sg = pref.export_sequence(d, g, K_L, EYE)
    want = [y * 9 + x for y in range(7) for x in range(9) if (y, x) not in ((2, 3), (4, 5), (0, 0), (6, 8))]
    assert src.tolist() == want and sg is None and xyzg.dtype == F32 and src.dtype == np.uint32
    ys, xs = np.divmod(src.astype(np.int64), 9)
    assert xyzg[:, 2].tobytes() == d[ys, xs].tobytes() and xyzg[:, 3].tobytes() == g[ys, xs].tobytes()   # identity: Zw = d
    # X = (d * (x - cx)) * (1 / fx), each operation rounded once
    ifx = F32(1) / K_L[0, 0]
    assert xyzg[:, 0].tobytes() == ((d[ys, xs] * (xs.astype(F32) - K_L[0, 2])).astype(F32) * ifx).astype(F32).tobytes()


def test_replica_gates_and_offsets():
    d, g = _maps()
    sg = np.linspace(0.01, 0.5, 63).reshape(7, 9).astype(F32)
    age = (np.arange(63).reshape(7, 9) % 5).astype(F32)
    cnt = (np.arange(63).reshape(7, 9) % 4).astype(np.uint8)
    assert pref.gates(d).sum() == 63
    assert pref.gates(d, stride=2).sum() == 4 * 5 and pref.gates(d, stride=3).sum() == 3 * 3
    assert pref.gates(d, max_depth=1.5).sum() == int((d <= F32(1.5)).sum())
    assert pref.gates(d, sigma=sg, max_sigma=0.25).sum() == int((sg <= F32(0.25)).sum())
    assert pref.gates(d, age=age, min_age=2.0).sum() == int((age >= 2).sum())
    assert pref.gates(d, counts=cnt, min_count=2).sum() == int((cnt >= 2).sum())
    nan_sigma = sg.copy(); nan_sigma[1, 1] = np.nan
    assert pref.gates(d, sigma=nan_sigma).sum() == 63 and pref.gates(d, sigma=nan_sigma, max_sigma=1e30).sum() == 62   # +inf: not read
    one = dict(depth=d, gray=g, K=K_L, Wk=EYE, sigma=sg)
    off, xyzg, src, s = pref.export([one, None, one, None], want_sigma=True, stride=2)
    assert off.tolist() == [0, 20, 20, 40, 40] and off.dtype == np.uint32
    assert xyzg.shape == (40, 4) and src[:20].tolist() == src[20:].tolist() and s.shape == (40,)
    off, xyzg, src, s = pref.export([None, None])
    assert off.tolist() == [0, 0, 0] and xyzg.shape == (0, 4) and s is None


def test_replica_transform_is_the_pose():
    d, g = _maps()
    T = np.eye(4, dtype=F32)
    T[:3, 3] = (0.5, -0.25, 2.0)
    T[:3, :3] = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], F32)
    a, _, _ = pref.export_sequence(d, g, K_L, EYE)
    b, _, _ = pref.export_sequence(d, g, K_L, T)
    np.testing.assert_array_equal(b[:, 0], (-a[:, 1] + F32(0.5)).astype(F32))
    np.testing.assert_array_equal(b[:, 1], (a[:, 0] - F32(0.25)).astype(F32))
    np.testing.assert_array_equal(b[:, 2], (a[:, 2] + F32(2.0)).astype(F32))


# ---- register pins ----------------------------------------------------------------------------------------------------------------
def _meta(txt, name):
    m = re.search(r"\.amdhsa_kernel %s\n.*?\.end_amdhsa_kernel" % name, txt, re.S)
    assert m, "kernel not found: " + name
    body = m.group(0)
    g = lambda k: int(re.search(r"\.amdhsa_%s (\d+)" % k, body).group(1))
    return g("next_free_vgpr"), g("private_segment_fixed_size"), g("group_segment_fixed_size")


def test_kernels_fit_the_budget():
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
    # (name, VGPR budget, LDS bytes: the wave counts / the scan's 1 024 run sums / the write's staged points, 1 024 x (16 + 4 + 4) + 32)
    for name, budget, lds in (("_ZN3dvo13k_points_prepENS_14PointsPrepArgsE", 46 + 8, 0),
                              ("_ZN3dvo14k_points_countENS_10PointsArgsE", 28 + 8, 16),
                              ("_ZN3dvo13k_points_scanEPKjiPjS2_", 14 + 8, 4096),
                              ("_ZN3dvo14k_points_writeENS_10PointsArgsE", 73 + 8, 24608),
                              ("_ZN3dvo18k_points_write_camENS_10PointsArgsE", 73 + 8, 24608)):
        v, scratch, got_lds = _meta(asm, name)
        assert scratch == 0, (name, scratch)
        assert got_lds == lds, (name, got_lds)
        assert v <= budget, (name, v, budget)
