"""CPU tests of the binomial-filtered gray pyramid of a sensor-depth batch (include/dvo.h: dvo_batch_set_pyramid_filter,
dvo_batch_pyramid_filter, dvo_op_pyramid_frames_filtered): the entry points are declared, exported, bound and in the C++ facade; NULL
and out-of-set arguments and the operator's refusals that need no device are returned; the numpy replica of the contract
(tests/pyramid_filter_ref.py) equals an exact float64 convolution with renormalisation on dyadic input, keeps the plain build's valid
sets at every level and never makes a NaN; its tracking call on plain frames is orc.track; the outcome numbers of DESIGN.md §39 are
recomputed; and every instance of the two new kernels compiles for gfx950 without scratch."""
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
import pyramid_filter_ref as fref
import pyramid_ref as pref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "direct-visual-odometry_amd")
F32 = np.float32
BAD = dvo.DVO_ERR_BAD_ARGUMENT
SIGNATURES = {
    "dvo_batch_set_pyramid_filter": r"dvo_batch\s*\*\s*\w+\s*,\s*int\s+\w+",
    "dvo_batch_pyramid_filter": r"dvo_batch\s*\*\s*\w+\s*,\s*int\s*\*\s*\w+",
    "dvo_op_pyramid_frames_filtered": r"int\s+dev\s*,\s*const\s+dvo_config\s*\*\s*\w+\s*,\s*const\s+dvo_pyramid_frames_args\s*\*\s*\w+\s*,\s*int\s+filter\s*,"
                                      r"\s*float\s*\*\s*const\s+gray_out\[\]\s*,\s*float\s*\*\s*const\s+depth_out\[\]\s*,\s*float\s*\*\s*const\s+sigma_out\[\]\s*,"
                                      r"\s*float\s*\*\s*const\s+wgt_out\[\]\s*,\s*dvo_pyramid_kernel\s*\*\s*\w+",
}


@pytest.mark.parametrize("name", sorted(SIGNATURES))
def test_declared_exported_and_listed(name):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dvo.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+%s\s*\(\s*%s\s*\)\s*;" % (name, SIGNATURES[name]), txt), name
    assert hasattr(dvo.lib(), name) and name in dvo.EXPORTS
    assert "dvo_*" in open(os.path.join(PKG, "csrc", "libdvo.map")).read()   # (the map exports the C ABI by its prefix)


def test_constants_contract_and_bindings():
    txt = open(os.path.join(ROOT, "include", "dvo.h")).read()
    for name, v in (("DVO_PYRAMID_FILTER_NONE", 0), ("DVO_PYRAMID_FILTER_BINOMIAL3", 1), ("DVO_PYRAMID_KERNEL_FILTER", 7)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, v), txt), name
        assert getattr(dvo, name[4:]) == v
    assert (fref.NONE, fref.BINOMIAL3) == (0, 1)
    flat = re.sub(r"\s+", " ", re.sub(r"\n \*", " ", txt))
    for phrase in ("NaN or <= DVO_INVALID", "k = (2 - |i|)(2 - |j|)", "S = fmaf((float)k, g, S)", "S / (float)W, one IEEE division",
                   "H of the STORED level l", "copies its reference's gray forward level by level",
                   "Out of scope: mono batches, the dvo_vo handles, the combination with lens undistortion"):
        assert phrase in flat, phrase
    assert callable(dvo.op_pyramid_frames_filtered) and callable(dvo.Batch.set_pyramid_filter) and callable(dvo.Batch.pyramid_filter)
    # the kernel record names the instance: plan = PLAN | WIDE << 1 | RAW << 2
    k = dvo.PyramidKernel(dvo.PYRAMID_KERNEL_FILTER, 2, 1 | 4)
    assert k.name() == "k_pyramid_filter_top<2, true, true, false>"
    assert dvo.PyramidKernel(dvo.PYRAMID_KERNEL_FILTER, 1, 2).name() == "k_pyramid_filter_top<1, false, false, true>"
    assert C.sizeof(dvo.PyramidKernel) == 12


def test_null_and_out_of_set_arguments_are_refused():
    L = dvo.lib()
    f = C.c_int(-7)
    for v in (0, 1, 2, -1):
        assert L.dvo_batch_set_pyramid_filter(None, v) == BAD
    assert L.dvo_batch_pyramid_filter(None, C.byref(f)) == BAD and L.dvo_batch_pyramid_filter(None, None) == BAD and f.value == -7


def test_operator_refusals_that_need_no_device():
    L = dvo.lib()
    L.dvo_last_error.restype = C.c_char_p
    img = np.zeros((1, 72, 88), F32)
    raw = np.zeros((1, 72, 88), np.uint8)

    def call(filt, a):
        return L.dvo_op_pyramid_frames_filtered(0, None, C.byref(a) if a is not None else None, filt, None, None, None, None, None)

    def args(**kw):
        a = dvo.PyramidFramesArgs()
        a.struct_size = C.sizeof(dvo.PyramidFramesArgs)
        a.n_seq, a.w, a.h, a.levels, a.culls = 1, 88, 72, 4, 1
        a.gray = img.ctypes.data
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    for filt in (dvo.PYRAMID_FILTER_NONE, dvo.PYRAMID_FILTER_BINOMIAL3):
        assert call(filt, None) == BAD                                     # the plain operator's refusals come first
        assert call(filt, args(struct_size=4)) == BAD and call(filt, args(n_seq=0)) == BAD and call(filt, args(flags=8)) == BAD
        assert call(filt, args(rgb=raw.ctypes.data)) == BAD               # both gray and rgb
    for filt in (2, -1, 7):
        assert call(filt, args()) == BAD
    B3 = dvo.PYRAMID_FILTER_BINOMIAL3
    assert call(B3, args(flags=dvo.PYRAMID_ROWS_DECIMATED)) == BAD and call(B3, args(flags=dvo.PYRAMID_SPLIT)) == BAD
    assert call(B3, args(flags=dvo.PYRAMID_SPLIT | dvo.PYRAMID_FORCE_WEIGHT_MAPS)) == BAD
    assert call(B3, args(w=640, h=480, levels=2, culls=3)) == BAD and b"culls" in L.dvo_last_error()


def test_facade_methods_compile(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("g++ not available")
    src = tmp_path / "snippet.cpp"
    src.write_text(r"""
#include "dvo.hpp"
int use()
{
    const dvo::Mat3 K{525.f, 0.f, 319.5f, 0.f, 525.f, 239.5f, 0.f, 0.f, 1.f};
    dvo::BatchTracker bt(4, K, 640, 480);
    bt.setPyramidFilter();
    bt.setPyramidFilter(DVO_PYRAMID_FILTER_NONE);
    return bt.pyramidFilter() + DVO_PYRAMID_FILTER_BINOMIAL3 + DVO_PYRAMID_KERNEL_FILTER;
}
""")
    r = subprocess.run([gxx, "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


# ------------------------------------------------------------------------------------------------ the replica's own arithmetic
def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


@pytest.mark.parametrize("h,w", [(37, 45), (72, 88), (6, 7)])
def test_replica_on_dyadic_input_is_the_exact_convolution(h, w):
    """gray as multiples of 2^-8 in [0, 1], with holes: one halving equals the float64 convolution with renormalisation rounded once,
    bit for bit; so does a second halving wherever the first divided by 16 (its results are multiples of 2^-12, still exact)"""
    rng = np.random.RandomState(3)
    g = (rng.randint(0, 257, (3, h, w)) / 256.0).astype(F32)
    g[rng.rand(3, h, w) < 0.06] = pref.INVALID
    g[1, 2:5, 1:4] = pref.INVALID
    a, e = fref.halve(g), fref.halve_exact(g)
    assert np.array_equal(_bits(a), _bits(e)) and fref.valid(a).any() and (a == pref.INVALID).any()
    # weights: an interior pixel with every tap valid is the plain binomial
    full = np.full((1, 5, 5), 0.25, F32); full[0, 2, 2] = 1.0
    assert fref.halve(full)[0, 1, 1] == F32((0.25 * 12 + 4.0) / 16) and fref.halve(full)[0, 0, 0] == F32(0.25)
    clean = (rng.randint(0, 257, (1, h, w)) / 256.0).astype(F32)
    a2, e2 = fref.halve(fref.halve(clean)), fref.halve_exact(fref.halve_exact(clean))
    assert np.array_equal(_bits(a2[:, 1:, 1:]), _bits(e2[:, 1:, 1:]))


def test_replica_fmaf_is_the_correctly_rounded_fmaf():
    """k is 1, 2 or 4, so the replica's fused step is one float32 addition: the same bits as the correctly rounded fmaf of
    tests/robust_ref.py, on values of every scale, +inf and subnormals"""
    import robust_ref as rr
    rng = np.random.RandomState(0)
    g = np.concatenate([rng.rand(50000), rng.rand(2000) * 1e30, [np.inf, 1e-40, 1e-45]]).astype(F32)
    s = np.concatenate([rng.rand(50000) * 9, -rng.rand(2000) * 1e30, [1.0, 1e-41, -3e-45]]).astype(F32)
    for k in (1, 2, 4):
        assert np.array_equal(_bits(fref.fmaf_k(k, g, s)), _bits(rr.fmaf(F32(k), g, s))), k


def _holes(n, h, w, seed):
    rng = np.random.RandomState(seed)
    g = rng.rand(n, h, w).astype(F32)
    for v in (np.nan, -7.0, pref.INVALID, -np.inf, np.inf):
        g[rng.rand(n, h, w) < 0.04] = v
    g[:, 0, 0] = np.nan; g[:, h - 1, w - 1] = -np.inf; g[:, 0, w - 1] = np.inf
    g[:, 8:13, 5:11] = pref.INVALID
    return g


@pytest.mark.parametrize("w,h,levels,culls", [(88, 72, 4, 1), (90, 73, 4, 1), (178, 147, 4, 2), (37, 29, 3, 0)])
def test_replica_keeps_the_plain_valid_sets_and_makes_no_nan(w, h, levels, culls):
    g = _holes(2, h, w, 5)
    filt = fref.build(w, h, levels, culls, g)
    plain = pref.build(w, h, levels, culls, g)
    for l in range(levels):
        assert filt["gray"][l].shape == plain["gray"][l].shape
        assert np.array_equal(fref.valid(filt["gray"][l]), fref.valid(plain["gray"][l])), l
        if culls > 0 or l < levels - 1:
            assert not np.isnan(filt["gray"][l]).any(), l
            assert ((filt["gray"][l] == pref.INVALID) | fref.valid(filt["gray"][l])).all()   # invalid is stored as DVO_INVALID
    assert np.isinf(filt["gray"][levels - 1]).any()                                           # +inf is a valid tap
    if culls == 0:
        assert np.array_equal(_bits(filt["gray"][levels - 1]), _bits(g))                      # the input unchanged
    # a planned set: a SKIP sequence has the reference's gray at every level, the others the new build's
    new = fref.build(w, h, levels, culls, g[::-1].copy())
    out = fref.planned(filt, new, (pref.SEQ_SKIP, pref.SEQ_TRACK), levels)
    for l in range(levels):
        assert np.array_equal(_bits(out["gray"][l][0]), _bits(filt["gray"][l][0])) and np.array_equal(_bits(out["gray"][l][1]), _bits(new["gray"][l][1]))


def test_tracking_replica_on_plain_frames_is_the_oracle():
    from dvo_amd import synth
    K = synth.K_640.copy(); K[:2] *= 0.5
    g, d, s, _ = synth.sequence(2, 320, 240, K, 42, sigma_value=0.5)
    g, d, s = g.numpy(), d.numpy(), s.numpy()
    ref, obj = fref.Frame(g[0], d[0], s[0], K, 3, 1, filtered=False), fref.Frame(g[1], d[1], s[1], K, 3, 1, filtered=False)
    cfg = dvo.default_config()
    xr, lr = fref.filtered_track(obj, ref, 3, cfg.max_iterations, cfg.min_update, cfg.min_residual, crop=True)
    xo, lo = orc.track(obj.o, ref.o, crop=True)
    assert xr.tobytes() == np.asarray(xo, F32).tobytes() and list(lr["n_iter"]) == [int(n) for n in lo["n_iter"][:3]]


def test_outcome_numbers_of_the_replica():
    """DESIGN.md §39's table, recomputed: gray noise 0.04 on synth's 320x240 pairs, motion 0.005 / 0.3 deg, seeds 42-49.  The constants
    the GPU test is held to are the replica's own."""
    o = fref.OUTCOME
    orc.set_tracker_params(step3=o["steps"], min_residual=o["min_residual"], min_update=o["min_update"])
    try:
        plain, filt = fref.outcome_replica()
    finally:
        orc.set_tracker_params()
    print("\nreplica: plain %s\n         filtered %s\n         summed %.5f against %.5f, ratio %.4f" % (plain.tolist(), filt.tolist(), filt.sum(), plain.sum(), filt.sum() / plain.sum()))
    np.testing.assert_allclose(plain, fref.REPLICA_PLAIN, rtol=1e-3)
    np.testing.assert_allclose(filt, fref.REPLICA_FILTERED, rtol=1e-3)
    assert abs(filt.sum() / plain.sum() - fref.REPLICA_RATIO) < 5e-4
    assert (filt < plain).sum() >= 6 and (plain >= 1.25 * filt).sum() >= 6      # the scene rule of the issue: at least six of eight


# ------------------------------------------------------------------------------------------------ the kernels' registers
def test_filter_kernels_compile_without_scratch():
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
    found = {}
    for m in re.finditer(r"\.amdhsa_kernel (_ZN3dvo2[01]k_pyramid_filter_(?:top|down)\w+)(.*?)\.end_amdhsa_kernel", txt, re.S):
        g = lambda k: int(re.search(r"\.amdhsa_%s (\d+)" % k, m.group(2)).group(1))
        found[m.group(1)] = (g("next_free_vgpr"), g("private_segment_fixed_size"), g("group_segment_fixed_size"))
    b = lambda v: "Lb%dE" % v
    want = {"_ZN3dvo20k_pyramid_filter_topILi%dE%s%s%sEEvNS_11PyramidArgsE" % (c, b(r), b(p), b(v))
            for c in (0, 1, 2) for r in (0, 1) for p in (0, 1) for v in ((0,) if c == 0 else (0, 1))}
    want |= {"_ZN3dvo21k_pyramid_filter_downILb%dEEEvNS_11PyramidArgsEif" % p for p in (0, 1)}
    assert set(found) == want and len(want) == 22
    for name, (vgpr, scratch, lds) in found.items():
        assert scratch == 0, "%s spills %d bytes of scratch per lane" % (name, scratch)
        assert vgpr <= 128, "%s needs %d VGPRs" % (name, vgpr)              # (four waves per SIMD at the least)
        assert lds <= 32 * 1024, "%s holds %d bytes of LDS" % (name, lds)   # (five workgroups per CU at the least)
    # no buffer at source or intermediate resolution: culls 0 stages nothing, culls 1 the source tile, culls 2 also the 65 x 17 tile
    assert all(found[n][2] == 0 for n in found if "ILi0E" in n or "down" in n)
    assert all(found[n][2] > 0 for n in found if "ILi1E" in n or "ILi2E" in n)
