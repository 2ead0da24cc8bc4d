"""CPU tests of a batch's affine brightness compensation (include/dvo.h, dvo_batch_set_affine_brightness and its companions): the
entry points are declared, exported and bound, dvo_affine_config and dvo_affine_log have the same layout in C, ctypes and numpy, a NULL
handle is refused before anything touches the GPU, the C++ facade's new methods compile, the reference of tests/affine_ref.py is
self-consistent (with (1, 0) throughout it is orc.track bit for bit), and the hot compensated kernel instances compile without scratch
inside their wave budget, the solve twin no worse than k_gn_solve_rw."""
import ctypes as C
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import affine_ref as ar
import dvo_amd as dvo
import orc
import robust_ref as rr
from dvo_amd import synth
from util import K640

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "direct-visual-odometry_amd")
_OP_HEAD = r"int\s+dev\s*,\s*const\s+dvo_config\s*\*[^;]*int\s+level\s*,\s*int\s+kind\s*,\s*float\s+param\s*,\s*float\s+s2\s*,"
SIGNATURES = {
    "dvo_batch_set_affine_brightness": r"dvo_batch\s*\*\s*\w+\s*,\s*const\s+dvo_affine_config\s*\*\s*\w+",
    "dvo_batch_set_affine_rows": r"dvo_batch\s*\*\s*\w+\s*,\s*const\s+float\s*\*\s*\w+\s*,\s*int\s+\w+",
    "dvo_batch_last_affine": r"dvo_batch\s*\*\s*\w+\s*,\s*float\s*\*\s*\w+",
    "dvo_batch_last_affine_log": r"dvo_batch\s*\*\s*\w+\s*,\s*int\s+\w+\s*,\s*dvo_affine_log\s*\*\s*\w+",
    "dvo_op_gn_step_affine": _OP_HEAD + r"\s*float\s+a\s*,\s*float\s+b\s*,\s*dvo_gn_result\s*\*\s*\w+\s*,\s*double\s+\w+\[5\]\s*,\s*float\s+\w+\[2\]",
}
CFG_FIELDS = [f[0] for f in dvo.AffineConfig._fields_]
LOG_FIELDS = [f[0] for f in dvo.AffineLog._fields_]


@pytest.mark.parametrize("name", sorted(SIGNATURES))
def test_declared_exported_and_listed(name):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dvo.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+%s\s*\(\s*%s\s*\)\s*;" % (name, SIGNATURES[name]), txt), name
    assert hasattr(dvo.lib(), name)
    assert name in dvo.EXPORTS


def test_constants_and_contract_are_declared():
    txt = open(os.path.join(ROOT, "include", "dvo.h")).read()
    for name, v in (("OFF", 0), ("ESTIMATE", 1), ("GIVEN", 2)):
        assert re.search(r"#define\s+DVO_AFFINE_%s\s+%d\b" % (name, v), txt), name
        assert getattr(dvo, "AFFINE_" + name) == v
    assert (ar.OFF, ar.ESTIMATE, ar.GIVEN) == (0, 1, 2)
    flat = re.sub(r"\s+", " ", txt)
    for phrase in ("c = fmaf(a, I1, b)", "M12 = fmaf(p, I2, M12)", "det = N * M11 - M1 * M1", "det > min_contrast * N * M11",
                   "SSD search still assumes brightness constancy", "not a joint 8-parameter Gauss-Newton"):
        assert phrase in flat, phrase


def test_layouts_match_c():
    cc = shutil.which("gcc") or shutil.which("cc")
    if not cc:
        pytest.skip("no C compiler")
    with tempfile.TemporaryDirectory() as td:
        src = os.path.join(td, "layout.c")
        body = "".join('    printf("cfg.%s %%zu\\n", offsetof(dvo_affine_config, %s));\n' % (f, f) for f in CFG_FIELDS)
        body += "".join('    printf("log.%s %%zu\\n", offsetof(dvo_affine_log, %s));\n' % (f, f) for f in LOG_FIELDS)
        open(src, "w").write('#include <stddef.h>\n#include <stdio.h>\n#include <stdint.h>\n#include "dvo.h"\nint main(void)\n{\n'
                             '    printf("sizeof_cfg %zu\\n", sizeof(dvo_affine_config));\n'
                             '    printf("sizeof_log %zu\\n", sizeof(dvo_affine_log));\n' + body + "    return 0;\n}\n")
        exe = os.path.join(td, "layout")
        subprocess.run([cc, "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", exe, src], check=True, capture_output=True)
        out = dict(l.split() for l in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split("\n") if l)
    assert int(out["sizeof_cfg"]) == C.sizeof(dvo.AffineConfig) == 24
    assert int(out["sizeof_log"]) == C.sizeof(dvo.AffineLog) == dvo.AFFINE_LOG_DTYPE.itemsize == 4 * (2 + 8 + 2 * 8 * 32 + 2)
    for f in CFG_FIELDS:
        assert int(out["cfg." + f]) == getattr(dvo.AffineConfig, f).offset, f
    for f in LOG_FIELDS:
        assert int(out["log." + f]) == getattr(dvo.AffineLog, f).offset == dvo.AFFINE_LOG_DTYPE.fields[f][1], f
    assert CFG_FIELDS == ["struct_size", "mode", "min_pixels", "min_contrast", "gain_min", "gain_max"]
    assert LOG_FIELDS == ["struct_size", "levels", "n_iter", "a", "b", "prime_a", "prime_b"]


def test_both_batches_bind_them():
    for cls in (dvo.Batch, dvo.MonoBatch):
        for m in ("set_affine_brightness", "set_affine_rows", "last_affine", "last_affine_log"):
            assert callable(getattr(cls, m, None)), (cls.__name__, m)
    assert callable(dvo.op_gn_step_affine)
    import inspect
    d = {k: v.default for k, v in inspect.signature(dvo.Batch.set_affine_brightness).parameters.items() if k != "self"}
    assert d == dict(mode=dvo.AFFINE_OFF, min_pixels=64, min_contrast=1e-3, gain_min=0.25, gain_max=4.0)
    assert ar.GUARDS == {k: v for k, v in d.items() if k != "mode"}


def test_null_handle_and_bad_operator_arguments_are_refused():
    L = dvo.lib()
    cfg = dvo.AffineConfig(C.sizeof(dvo.AffineConfig), dvo.AFFINE_ESTIMATE, 64, 1e-3, 0.25, 4.0)
    s = (C.c_float * 4)(1.0, 0.0, 1.0, 0.0)
    lg = dvo.AffineLog(); lg.struct_size = C.sizeof(dvo.AffineLog)
    assert L.dvo_batch_set_affine_brightness(None, C.byref(cfg)) == dvo.DVO_ERR_BAD_ARGUMENT
    assert L.dvo_batch_set_affine_brightness(None, None) == dvo.DVO_ERR_BAD_ARGUMENT
    assert L.dvo_batch_set_affine_rows(None, s, 0) == dvo.DVO_ERR_BAD_ARGUMENT
    assert L.dvo_batch_set_affine_rows(None, None, 0) == dvo.DVO_ERR_BAD_ARGUMENT
    assert L.dvo_batch_last_affine(None, s) == dvo.DVO_ERR_BAD_ARGUMENT
    assert L.dvo_batch_last_affine_log(None, 0, C.byref(lg)) == dvo.DVO_ERR_BAD_ARGUMENT
    out = dvo.GnResult()
    f = C.c_float
    mom = (C.c_double * 5)(); nxt = (C.c_float * 2)()
    img = (C.c_float * 16)(); K = (C.c_float * 9)(); xi = (C.c_float * 6)()
    # NULL maps, NULL outputs, a kind outside the set, a param that is not finite and > 0: refused before a device is opened
    assert L.dvo_op_gn_step_affine(0, None, None, None, None, None, 4, 4, None, None, 0, 0, f(1.0), f(1.0), f(1.0), f(0.0), C.byref(out), mom, nxt) \
        == dvo.DVO_ERR_BAD_ARGUMENT
    assert L.dvo_op_gn_step_affine(0, None, img, img, img, img, 4, 4, K, xi, 0, 0, f(1.0), f(1.0), f(1.0), f(0.0), C.byref(out), None, nxt) \
        == dvo.DVO_ERR_BAD_ARGUMENT
    assert L.dvo_op_gn_step_affine(0, None, img, img, img, img, 4, 4, K, xi, 0, 0, f(1.0), f(1.0), f(1.0), f(0.0), C.byref(out), mom, None) \
        == dvo.DVO_ERR_BAD_ARGUMENT
    for kind, param in ((3, 1.0), (-1, 1.0), (1, 0.0), (1, -1.0), (2, float("nan")), (2, float("inf"))):
        assert L.dvo_op_gn_step_affine(0, None, img, img, img, img, 4, 4, K, xi, 0, kind, f(param), f(1.0), f(1.0), f(0.0), C.byref(out), mom, nxt) \
            == dvo.DVO_ERR_BAD_ARGUMENT, (kind, param)


def test_facade_affine_methods_compile(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("g++ not available")
    src = tmp_path / "snippet.cpp"
    src.write_text(r"""
#include "dvo.hpp"
#include <vector>
int use(const float* dev_rows)
{
    const dvo::Mat3 K{525.f, 0.f, 319.5f, 0.f, 525.f, 239.5f, 0.f, 0.f, 1.f};
    dvo::BatchTracker bt(4, K, 640, 480);
    bt.setAffineBrightness(DVO_AFFINE_ESTIMATE);
    bt.setAffineBrightness(DVO_AFFINE_GIVEN, 64, 1e-3f, 0.5f, 2.0f);
    bt.setAffineRows(dev_rows, true);
    std::vector<float> a0 = bt.lastAffine();
    dvo_affine_log l0 = bt.lastAffineLog(1);
    bt.setAffineBrightness(DVO_AFFINE_OFF);
    dvo::BatchMono mb(4, K, 640, 480);
    mb.setAffineBrightness(DVO_AFFINE_ESTIMATE, 128);
    mb.setAffineRows(nullptr);
    std::vector<float> a1 = mb.lastAffine();
    dvo_affine_log l1 = mb.lastAffineLog(0);
    return (int)(a0.size() + a1.size()) + l0.levels + l1.levels;
}
""")
    r = subprocess.run([gxx, "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


# ------------------------------------------------------------------------------------------------ the reference's own arithmetic
LEVELS, CULLS = 3, 1
KH = np.array(K640, np.float32).copy()
KH[0] *= 0.5
KH[1] *= 0.5


@pytest.fixture(scope="module")
def two_frames():
    g, d, s, _ = synth.sequence(2, width=320, height_px=240, K=KH, seed=42, sigma_value=0.5)
    g, d, s = g.numpy(), d.numpy(), s.numpy()
    return orc.OFrame(g[1], d[1], s[1], KH, LEVELS, CULLS), orc.OFrame(g[0], d[0], s[0], KH, LEVELS, CULLS)


def test_reference_identity_is_the_oracle(two_frames):
    """(1, 0): the restated terms are the oracle's r and rw bit for bit (asserted inside pixels()), and the replica of a whole call
    with (1, 0) throughout is orc.track bit for bit"""
    obj, ref = two_frames
    wp = ar.weight_params()
    for l in range(LEVELS):
        px = ar.pixels(obj.gray(l), ref.gray(l), ref.depth(l), ref.sigma(l), ref.K(l), np.zeros(6, np.float32), l, False, wp)
        t = ar.terms(px, 1.0, 0.0)
        assert px["n_valid"] > 500 and t["r"].tobytes() == px["plain"]["r"].tobytes() and t["rw"].tobytes() == px["plain"]["rw"].tobytes()
    xo, lo = orc.track(obj, ref, crop=False)
    cfg = dvo.default_config()
    xr, lr = ar.affine_track(obj, ref, LEVELS, ar.GIVEN, False, cfg.max_iterations, cfg.min_update, cfg.min_residual, wp=wp)
    assert list(lr["n_iter"]) == [int(n) for n in lo["n_iter"][:LEVELS]]
    assert xr.tobytes() == np.asarray(xo, np.float32).tobytes(), (xr, xo)


def test_reference_closed_form_recovers_a_gain_and_offset(two_frames):
    """I2 = a* I1 + b* exactly in the moments: the closed form returns (a*, b*), and every guard keeps the previous entry"""
    obj, ref = two_frames
    px = ar.pixels(obj.gray(1), ref.gray(1), ref.depth(1), ref.sigma(1), ref.K(1), np.zeros(6, np.float32), 1, False, ar.weight_params())
    fake = dict(px)
    fake["I2"] = (np.float32(1.25) * px["I1"] + np.float32(-0.04)).astype(np.float32)
    ex = ar.exact(fake, 1.0, 0.0)
    (a, b), ok = ar.closed_form(ex["n"], ex["M"], ex["n"], ar.GUARDS, (1.0, 0.0))
    assert ok and abs(float(a) - 1.25) < 1e-5 and abs(float(b) + 0.04) < 1e-5
    prev = (np.float32(0.9), np.float32(0.01))
    for g in (dict(ar.GUARDS, gain_max=1.2), dict(ar.GUARDS, min_pixels=ex["n"] + 1), dict(ar.GUARDS, min_contrast=0.999)):
        assert ar.closed_form(ex["n"], ex["M"], ex["n"], g, prev) == (prev, False)
    flat = dict(px)
    flat["I1"] = np.full_like(px["I1"], 0.5)
    exf = ar.exact(flat, 1.0, 0.0)
    assert ar.closed_form(exf["n"], exf["M"], exf["n"], ar.GUARDS, prev) == (prev, False)       # det = 0
    assert ar.closed_form(0, np.zeros(5), 0, ar.GUARDS, prev) == (prev, False)                # no pixels
    lo, hi, verdicts = ar.next_entry_bounds(ex, 17, False, ar.GUARDS, (1.0, 0.0))
    assert verdicts == {True} and lo[0] < a < hi[0] and lo[1] < b < hi[1]
    # with weights: rho = 1 everywhere (a huge scale) gives the same moments, M0 = n
    exr = ar.exact(fake, 1.0, 0.0, rr.HUBER, 1.345, 1e12)
    np.testing.assert_array_equal(exr["M"][1:], ex["M"][1:])
    assert exr["M"][0] == ex["n"]


# ------------------------------------------------------------------------------------------------ registers of the hot instances
# k_track_gn_ab / k_track_gn_ab_cam <4, 2, raster | 2-D tiles, plain | robust>: built for DVO_GN_AB_WAVES = 5 waves per SIMD -- 512 / 5
# rounded down to the allocation granule of 8 = 96 VGPRs -- without scratch; at 6 (80) they spill
AB_WAVES = 5
AB_VGPR_BUDGET = (512 // AB_WAVES) // 8 * 8


def _meta(txt, name):
    m = re.search(r"\.amdhsa_kernel %s.*?\.end_amdhsa_kernel" % re.escape(name), txt, re.S)
    assert m, "kernel not found: " + name
    body = m.group(0)
    return (int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", body).group(1)), int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body).group(1)))


def test_hot_compensated_kernels_fit_the_register_budget():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    src = open(os.path.join(PKG, "csrc", "dvo_kernels.hip")).read()
    assert re.search(r"#define DVO_GN_AB_WAVES %d\b" % AB_WAVES, src)
    cont = open(os.path.join(PKG, "Makefile")).read().split("FLAGS   =", 1)[1].split("\n")
    flags = (cont[0].rstrip("\\") + " " + cont[1]).split()
    flags = [f.replace("$(ARCH)", "gfx950") for f in flags if f != "-fPIC"]
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "k.s")
        subprocess.run([hipcc] + flags + ["-S", "--cuda-device-only", "-o", out, os.path.join(PKG, "csrc", "dvo_kernels.hip")],
                       check=True, capture_output=True, timeout=900)
        txt = open(out).read()
    checked = 0
    args = "EEvNS_6GnArgsENS_8RobustGnENS_8AffineGnE"
    for kernel in ("_ZN3dvo13k_track_gn_ab", "_ZN3dvo17k_track_gn_ab_cam"):
        for variant in ("ILi4ELi2ELb0ELb0E", "ILi4ELi2ELb1ELb0E", "ILi4ELi2ELb0ELb1E", "ILi4ELi2ELb1ELb1E"):   # <PPT 4, G 2, T2D, ROB>
            vgpr, scratch = _meta(txt, kernel + variant + args)
            assert scratch == 0, "%s%s spills %d bytes of scratch per lane" % (kernel, variant, scratch)
            assert vgpr <= AB_VGPR_BUDGET, "%s%s needs %d VGPRs (budget %d = %d waves per SIMD)" % (kernel, variant, vgpr, AB_VGPR_BUDGET, AB_WAVES)
            checked += 1
    assert checked == 8
    rw = _meta(txt, "_ZN3dvo13k_gn_solve_rwENS_9SolveArgsENS_11RobustSolveE")
    ab = _meta(txt, "_ZN3dvo13k_gn_solve_abENS_9SolveArgsENS_11RobustSolveENS_11AffineSolveE")
    assert ab[0] <= rw[0] and ab[1] <= rw[1], ("k_gn_solve_ab (VGPRs, scratch) %s against k_gn_solve_rw %s" % (ab, rw))
    # the plain and the weighted kernels keep their names and template parameters beside the new family
    assert re.search(r"\.amdhsa_kernel _ZN3dvo10k_track_gnILi4ELi2ELb0ELb0EEEvNS_6GnArgsE\b", txt)
    assert re.search(r"\.amdhsa_kernel _ZN3dvo13k_track_gn_rwILi4ELi2ELb0EEEvNS_6GnArgsENS_8RobustGnE\b", txt)
