"""CPU tests of the median (MAD) robust scale of a batch (include/dvo.h, dvo_batch_set_robust_median and its companions):
the entry points are declared, exported and bound, dvo_robust_log has the same layout in C and in ctypes, every refusal that needs no
handle is made before anything touches the GPU, the header states the contract, the C++ facade's new methods compile, the replica's
rules (tests/robust_median_ref.py) hold on hand-made residual vectors, a whole replica call with the scale forced to +inf is orc.track
bit for bit, and the four hot instances of the new tile kernels compile without scratch inside five waves per SIMD."""
import ctypes as C
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import dvo_amd as dvo
import orc
import robust_median_ref as mr
from dvo_amd import synth
from util import K640

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "direct-visual-odometry_amd")
SIGNATURES = {
    "dvo_batch_set_robust_median": r"dvo_batch\s*\*\s*\w+\s*,\s*const\s+dvo_robust_config\s*\*\s*\w+",
    "dvo_batch_last_robust_log": r"dvo_batch\s*\*\s*\w+\s*,\s*int\s+\w+\s*,\s*dvo_robust_log\s*\*\s*\w+",
    "dvo_batch_last_robust_histogram": r"dvo_batch\s*\*\s*\w+\s*,\s*int\s+\w+\s*,\s*uint32_t\s+\w+\s*\[\s*256\s*\]",
    "dvo_op_gn_step_robust_median": r"int\s+dev\s*,\s*const\s+dvo_config\s*\*[^;]*int\s+level\s*,\s*int\s+kind\s*,\s*float\s+param\s*,\s*float\s+s2\s*,"
                                    r"\s*dvo_gn_result\s*\*\s*\w+\s*,\s*uint32_t\s+\w+\s*\[\s*256\s*\]\s*,\s*int\s*\*\s*\w+\s*,\s*float\s*\*\s*\w+",
}
FIELDS = [f[0] for f in dvo.RobustLog._fields_]
F32 = np.float32


@pytest.mark.parametrize("name", sorted(SIGNATURES))
def test_declared_exported_and_listed(name):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dvo.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+%s\s*\(\s*%s\s*\)\s*;" % (name, SIGNATURES[name]), txt), name
    assert hasattr(dvo.lib(), name)
    assert name in dvo.EXPORTS


def test_constants_and_contract_phrases():
    txt = open(os.path.join(ROOT, "include", "dvo.h")).read()
    assert re.search(r"#define\s+DVO_ROBUST_SCALE_MEDIAN\s+2\b", txt)
    assert dvo.ROBUST_SCALE_MEDIAN == 2 == mr.MEDIAN and dvo.MEDIAN_BINS == 256 == mr.BINS and mr.K0 == 1776
    flat = re.sub(r"[\s*]+", " ", txt)
    for phrase in ("K0 = (127 - 16) << 4 = 1776", "clamp((int)(__float_as_uint(fabsf(r)) >> 19) - 1776, 0, 255)",
                   "16 bins per octave over [2^-16, 1)", "sum counts = n_valid exactly", "main loop and deferred border loop alike",
                   "independent of tile shape, launch plan, track_streams and summation order",
                   "the smallest bin with cum(m) >= (n + 1) / 2", "__uint_as_float(((m + 1776) << 19) | (1 << 18))",
                   "s = 1.4826f med", "s2 = max(s s, floor2)", "priming pair", "no pose, no track log, no quality record",
                   "no contraction"):
        assert phrase in flat, phrase
    kh = open(os.path.join(PKG, "csrc", "dvo_kernels.h")).read()
    assert re.search(r"#define\s+DVO_MEDIAN_K0\s+1776\b", kh) and re.search(r"#define\s+DVO_MEDIAN_BINS\s+256\b", kh)


def test_layout_matches_c():
    cc = shutil.which("gcc") or shutil.which("cc")
    if not cc:
        pytest.skip("no C compiler")
    with tempfile.TemporaryDirectory() as td:
        src = os.path.join(td, "layout.c")
        body = "".join('    printf("%s %%zu\\n", offsetof(dvo_robust_log, %s));\n' % (f, f) for f in FIELDS)
        open(src, "w").write('#include <stddef.h>\n#include <stdio.h>\n#include <stdint.h>\n#include "dvo.h"\nint main(void)\n{\n'
                             '    printf("sizeof %zu\\n", sizeof(dvo_robust_log));\n' + body + "    return 0;\n}\n")
        exe = os.path.join(td, "layout")
        subprocess.run([cc, "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", exe, src], check=True, capture_output=True)
        out = dict(l.split() for l in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split("\n") if l)
    assert int(out["sizeof"]) == C.sizeof(dvo.RobustLog) == dvo.ROBUST_LOG_DTYPE.itemsize
    for f in FIELDS:
        assert int(out[f]) == getattr(dvo.RobustLog, f).offset, f
    assert FIELDS == ["struct_size", "levels", "n_iter", "s2", "median_bin", "count", "prime_bin", "prime_count"]


def test_both_batches_bind_them():
    for cls in (dvo.Batch, dvo.MonoBatch):
        for m in ("set_robust_median", "last_robust_log", "last_robust_histogram"):
            assert callable(getattr(cls, m, None)), (cls.__name__, m)
    assert callable(dvo.op_gn_step_robust_median)


def test_refusals_that_need_no_handle():
    L = dvo.lib()
    cfg = dvo.RobustConfig(C.sizeof(dvo.RobustConfig), dvo.ROBUST_HUBER, dvo.ROBUST_SCALE_MEDIAN, 1.345, 1e-3)
    lg = dvo.RobustLog(); lg.struct_size = C.sizeof(dvo.RobustLog)
    cnt = (C.c_uint32 * 256)()
    assert L.dvo_batch_set_robust_median(None, C.byref(cfg)) == dvo.DVO_ERR_BAD_ARGUMENT
    assert L.dvo_batch_set_robust_median(None, None) == dvo.DVO_ERR_BAD_ARGUMENT
    assert L.dvo_batch_last_robust_log(None, 0, C.byref(lg)) == dvo.DVO_ERR_BAD_ARGUMENT
    assert L.dvo_batch_last_robust_histogram(None, 0, cnt) == dvo.DVO_ERR_BAD_ARGUMENT
    out = dvo.GnResult()
    f = C.c_float
    m = C.c_int(0); nxt = C.c_float(0)
    img = (C.c_float * 16)(); K = (C.c_float * 9)(); xi = (C.c_float * 6)()
    step = L.dvo_op_gn_step_robust_median
    # NULL outputs, NULL maps, a kind outside the set, a param that is not finite and > 0: refused before a device is opened
    assert step(0, None, img, img, img, img, 4, 4, K, xi, 0, 1, f(1.0), f(1.0), C.byref(out), None, C.byref(m), C.byref(nxt)) == dvo.DVO_ERR_BAD_ARGUMENT
    assert step(0, None, img, img, img, img, 4, 4, K, xi, 0, 1, f(1.0), f(1.0), C.byref(out), cnt, None, C.byref(nxt)) == dvo.DVO_ERR_BAD_ARGUMENT
    assert step(0, None, img, img, img, img, 4, 4, K, xi, 0, 1, f(1.0), f(1.0), C.byref(out), cnt, C.byref(m), None) == dvo.DVO_ERR_BAD_ARGUMENT
    assert step(0, None, None, None, None, None, 4, 4, None, None, 0, 1, f(1.0), f(1.0), C.byref(out), cnt, C.byref(m), C.byref(nxt)) == dvo.DVO_ERR_BAD_ARGUMENT
    for kind, param in ((3, 1.0), (-1, 1.0), (1, 0.0), (1, -1.0), (2, float("nan")), (2, float("inf"))):
        assert step(0, None, img, img, img, img, 4, 4, K, xi, 0, kind, f(param), f(1.0), C.byref(out), cnt, C.byref(m), C.byref(nxt)) \
            == dvo.DVO_ERR_BAD_ARGUMENT, (kind, param)


def test_facade_median_methods_compile(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("g++ not available")
    src = tmp_path / "snippet.cpp"
    src.write_text(r"""
#include "dvo.hpp"
#include <vector>
int use()
{
    const dvo::Mat3 K{525.f, 0.f, 319.5f, 0.f, 525.f, 239.5f, 0.f, 0.f, 1.f};
    dvo::BatchTracker bt(4, K, 640, 480);
    bt.setRobustMedian(DVO_ROBUST_HUBER);
    bt.setRobustMedian(DVO_ROBUST_STUDENT_T, 5.0f, 1e-3f);
    dvo_robust_log lg = bt.lastRobustLog(1);
    std::vector<uint32_t> h0 = bt.lastRobustHistogram(1);
    bt.setRobustWeights(DVO_ROBUST_NONE);
    dvo::BatchMono mb(4, K, 640, 480);
    mb.setRobustMedian(DVO_ROBUST_HUBER, 1.345f);
    std::vector<uint32_t> h1 = mb.lastRobustHistogram(0);
    return (int)(h0.size() + h1.size()) + lg.prime_bin + mb.lastRobustLog(0).prime_count;
}
""")
    r = subprocess.run([gxx, "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


# ------------------------------------------------------------------------------------------------ the replica's own rules
def test_bins_of_hand_made_residuals():
    z = np.zeros(37, F32)
    assert (mr.bins(z) == 0).all() and mr.select(mr.counts(z)) == (0, 37)
    assert (mr.bins(F32([-0.0, 1e-30, -2.0 ** -17, np.nextafter(F32(2.0 ** -16), F32(0))])) == 0).all()
    big = F32([1.0, -1.0, 3.5, -1e30, np.inf, -np.inf, np.nan])
    assert (mr.bins(big) == 255).all() and mr.select(mr.counts(big)) == (255, 7)
    assert mr.bins(F32([np.nextafter(F32(1.0), F32(0))]))[0] == 255 and mr.bins(F32([2.0 ** -16]))[0] == 0
    # 16 bins per octave: 2^-16 * 2^(k / 16) rounded down to the bin's edge; the sign does not matter
    for k in range(1, 256):
        e = mr.edge(k)
        assert mr.bins(F32([e, -e]))[0] == k == mr.bins(F32([-e]))[0] and mr.bins(F32([np.nextafter(e, F32(0))]))[0] == k - 1
    assert mr.edge(16) == F32(2.0 ** -15) and mr.edge(17) == F32(2.0 ** -15 * (1 + 1 / 16)) and mr.edge(255) == F32(0.5 * (1 + 15 / 16))
    assert mr.bins(F32([0.75]))[0] == 248 and mr.bins(F32([2.0 ** -16 * 1.07]))[0] == 1


def test_selection_on_one_value_per_bin_edge():
    edges = np.array([mr.edge(k) for k in range(1, 256)], F32)
    for n in (255, 254, 2, 1):            # odd and even
        r = edges[:n] * np.where(np.arange(n) % 2, F32(-1), F32(1))
        c = mr.counts(r)
        assert c.sum() == n and c[0] == 0 and (c[1:n + 1] == 1).all()
        m, nn = mr.select(c)
        # the (n + 1) // 2-th smallest value sits in bin (n + 1) // 2 (the lower median for an even n)
        assert nn == n and m == (n + 1) // 2, (n, m)
    assert mr.select(np.zeros(256, np.uint32)) == (-1, 0)
    s2, m, n = mr.next_s2(np.zeros(256, np.uint32), 1e-6)
    assert s2 == np.inf and (m, n) == (-1, 0)                      # n = 0: the next entry is plain
    c = np.zeros(256, np.uint32); c[[10, 200]] = (5, 5)
    assert mr.select(c) == (10, 10)
    c[200] = 6
    assert mr.select(c) == (200, 11)
    c[10] = 6
    assert mr.select(c) == (10, 12)


def test_bin_scale():
    for m in (0, 1, 100, 255):
        med = np.array([((m + 1776) << 19) | (1 << 18)], np.uint32).view(F32)[0]
        assert mr.edge(m) < med < (mr.edge(m + 1) if m < 255 else F32(1.0)) if m > 0 else med < mr.edge(1)
        s = F32(F32(1.4826) * med)
        assert mr.bin_s2(m, 0.0) == F32(s * s)
    assert mr.bin_s2(0, F32(1e-3) * F32(1e-3)) == F32(1e-3) * F32(1e-3)          # a floor that binds
    assert mr.bin_s2(200, F32(1e-3) * F32(1e-3)) > F32(1e-3) * F32(1e-3)         # and one that does not
    # bin 255's midpoint is 0.984375: s2 = (1.4826f * 0.984375f)^2
    assert mr.bin_s2(255, 0.0) == F32(F32(F32(1.4826) * F32(0.984375)) * F32(F32(1.4826) * F32(0.984375)))
    e = mr.edge_slack(F32([mr.edge(5), np.nextafter(mr.edge(5), F32(0)), mr.edge(7) * F32(1.001), 0.0, 2.0]))
    assert e[5] == 2 and e.sum() == 2


KH = np.array(K640, F32).copy()
KH[0] *= 0.5
KH[1] *= 0.5


def test_replica_with_an_infinite_scale_is_the_oracle_track():
    g, d, s, _ = synth.sequence(2, width=320, height_px=240, K=KH, seed=42, sigma_value=0.5)
    g, d, s = g.numpy(), d.numpy(), s.numpy()
    obj, ref = orc.OFrame(g[1], d[1], s[1], KH, 3, 1), orc.OFrame(g[0], d[0], s[0], KH, 3, 1)
    xo, lo = orc.track(obj, ref, crop=False)
    cfg = dvo.default_config()
    xr, lr = mr.median_track(obj, ref, 3, mr.HUBER, 1.345, 1e-6, False, cfg.max_iterations, cfg.min_update, cfg.min_residual,
                             force_s2=np.inf)
    assert list(lr["n_iter"]) == [int(n) for n in lo["n_iter"][:3]]
    assert xr.tobytes() == np.asarray(xo, F32).tobytes(), (xr, xo)
    for l in range(3):
        assert lr["residual"][l].tobytes() == lo["residual"][l].tobytes() and lr["xi_after"][l].tobytes() == lo["xi_after"][l].tobytes(), l
        assert np.isinf(lr["s2"][l]).all() and all(n > 500 for n in lr["count"][l])
    # and with the rule itself the scale is finite, follows the previous record and moves the pose
    xm, lm = mr.median_track(obj, ref, 3, mr.HUBER, 1.345, 1e-6, False, cfg.max_iterations, cfg.min_update, cfg.min_residual)
    assert lm["prime"][1] == lm["count"][0][0] and lm["prime"][0] == lm["median_bin"][0][0]     # the same pose, the same pixels
    assert lm["s2"][0][0] == mr.bin_s2(lm["prime"][0], 1e-6) and np.isfinite(np.concatenate(lm["s2"])).all()
    assert xm.tobytes() != xr.tobytes()


# ------------------------------------------------------------------------------------------------ registers of the hot instances
# k_track_gn_md / k_track_gn_md_cam <4, 2, raster | 2-D tiles>: built for five waves per SIMD (DVO_GN_MD_WAVES = 5: 512 / 5 in
# granules of 8 = 96 VGPRs; the LDS add does not fit the 80 of k_track_gn_rw's six waves), no scratch
MD_VGPR_CEILING = 96


def test_hot_median_kernels_fit_five_waves_without_scratch():
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
    for kernel in ("_ZN3dvo13k_track_gn_md", "_ZN3dvo17k_track_gn_md_cam"):
        for variant in ("ILi4ELi2ELb0EE", "ILi4ELi2ELb1EE"):   # <PPT 4, G 2, raster | 2-D tiles>
            m = re.search(r"\.amdhsa_kernel %s%s.*?\.end_amdhsa_kernel" % (kernel, variant), txt, re.S)
            assert m, "kernel variant not found: " + kernel + variant
            body = m.group(0)
            scratch = int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body).group(1))
            vgpr = int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", body).group(1))
            lds = int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", body).group(1))
            assert scratch == 0, "%s%s spills %d bytes of scratch per lane" % (kernel, variant, scratch)
            assert vgpr <= MD_VGPR_CEILING, "%s%s needs %d VGPRs (ceiling %d = 5 waves per SIMD)" % (kernel, variant, vgpr, MD_VGPR_CEILING)
            assert lds <= 160 * 1024 // 5, (kernel, variant, lds)   # five workgroups of four waves per CU
            checked += 1
    assert checked == 4
    assert re.search(r"#define\s+DVO_GN_MD_WAVES\s+5\b", open(os.path.join(PKG, "csrc", "dvo_kernels.hip")).read())
    # the weighted family keeps its names beside the new one
    assert re.search(r"\.amdhsa_kernel _ZN3dvo13k_track_gn_rwILi4ELi2ELb0EEEvNS_6GnArgsENS_8RobustGnE\b", txt)
