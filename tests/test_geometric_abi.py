"""CPU tests of a sensor-depth batch's geometric (depth) term (include/dvo.h, dvo_batch_set_geometric and its companions): the entry
points are declared, exported and bound, the three structs have the same layout in C, ctypes and numpy, the default config is the
documented one, every refusal that needs no device is returned, the C++ facade's new methods compile, the reference of
tests/geometric_ref.py is self-consistent (its restated warp, sampler and Jacobian reproduce the oracle's photometric rows bit for
bit, and with weight 0 on the reference's depth a whole call is orc.track bit for bit), and the hot kernel instances compile without
scratch inside their wave budget, the solve twin no worse than k_gn_solve."""
import ctypes as C
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import dvo_amd as dvo
import geometric_ref as gr
import orc
from dvo_amd import synth
from util import K640

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "direct-visual-odometry_amd")
SIGNATURES = {
    "dvo_batch_set_geometric": (r"int", r"dvo_batch\s*\*\s*\w+\s*,\s*const\s+dvo_geometric_config\s*\*\s*\w+"),
    "dvo_batch_last_geometric": (r"int", r"dvo_batch\s*\*\s*\w+\s*,\s*dvo_geometric_record\s*\*\s*\w+"),
    "dvo_batch_last_geometric_log": (r"int", r"dvo_batch\s*\*\s*\w+\s*,\s*int\s+\w+\s*,\s*dvo_geometric_log\s*\*\s*\w+"),
    "dvo_geometric_config_default": (r"void", r"dvo_geometric_config\s*\*\s*\w+"),
    "dvo_op_gn_step_geometric": (r"int", r"int\s+dev\s*,\s*const\s+dvo_config\s*\*[^;]*const\s+float\s*\*\s*obj_depth[^;]*const\s+float\s*\*\s*ref_depth[^;]*"
                                         r"int\s+level\s*,\s*float\s+weight\s*,\s*float\s+max_diff\s*,\s*dvo_gn_result\s*\*\s*\w+\s*,\s*double\s+\w+\[2\]"),
}
STRUCTS = {"dvo_geometric_config": dvo.GeometricConfig, "dvo_geometric_record": dvo.GeometricRecord, "dvo_geometric_log": dvo.GeometricLog}


@pytest.mark.parametrize("name", sorted(SIGNATURES))
def test_declared_exported_and_listed(name):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dvo.h")).read(), flags=re.S)
    ret, args = SIGNATURES[name]
    assert re.search(r"\b%s\s+%s\s*\(\s*%s\s*\)\s*;" % (ret, name, args), txt), name
    assert hasattr(dvo.lib(), name)
    assert name in dvo.EXPORTS
    assert "dvo_*" in open(os.path.join(PKG, "csrc", "libdvo.map")).read()   # (the map exports the C ABI by its prefix)


def test_constants_and_contract_are_declared():
    txt = open(os.path.join(ROOT, "include", "dvo.h")).read()
    for name, v in (("OFF", 0), ("ON", 1)):
        assert re.search(r"#define\s+DVO_GEOMETRIC_%s\s+%d\b" % (name, v), txt), name
        assert getattr(dvo, "GEOMETRIC_" + name) == v
    assert (gr.OFF, gr.ON) == (0, 1)
    flat = re.sub(r"\s+", " ", re.sub(r"\n \*", " ", txt))
    for phrase in ("rz = Zs - Zw", "Jz[2] = Jp[2] - 1, Jz[3] = Jp[3] - Y, Jz[4] = Jp[4] + X", "lam = weight * (iz * iz)", "rgw = rg * wgt",
                   "S29 = fmaf(rg, rg, S29)", "fabsf(rz) <= max_diff", "finite and >= min_depth", "dvo_vo handles have no geometric term"):
        assert phrase in flat, phrase


def test_layouts_match_c():
    cc = shutil.which("gcc") or shutil.which("cc")
    if not cc:
        pytest.skip("no C compiler")
    with tempfile.TemporaryDirectory() as td:
        src = os.path.join(td, "layout.c")
        body = ""
        for cname, cls in STRUCTS.items():
            body += '    printf("%s.sizeof %%zu\\n", sizeof(%s));\n' % (cname, cname)
            body += "".join('    printf("%s.%s %%zu\\n", offsetof(%s, %s));\n' % (cname, f[0], cname, f[0]) for f in cls._fields_)
        open(src, "w").write('#include <stddef.h>\n#include <stdio.h>\n#include <stdint.h>\n#include "dvo.h"\nint main(void)\n{\n' + body + "    return 0;\n}\n")
        exe = os.path.join(td, "layout")
        subprocess.run([cc, "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", exe, src], check=True, capture_output=True)
        out = dict(l.split() for l in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split("\n") if l)
    for cname, cls in STRUCTS.items():
        assert int(out[cname + ".sizeof"]) == C.sizeof(cls), cname
        for f in cls._fields_:
            assert int(out["%s.%s" % (cname, f[0])]) == getattr(cls, f[0]).offset, (cname, f[0])
    assert C.sizeof(dvo.GeometricConfig) == 16 and C.sizeof(dvo.GeometricRecord) == 8 == dvo.GEOMETRIC_RECORD_DTYPE.itemsize
    assert C.sizeof(dvo.GeometricLog) == dvo.GEOMETRIC_LOG_DTYPE.itemsize == 4 * (2 + 8 + 2 * 8 * 32)
    for f in dvo.GeometricLog._fields_:
        assert getattr(dvo.GeometricLog, f[0]).offset == dvo.GEOMETRIC_LOG_DTYPE.fields[f[0]][1], f[0]
    assert [f[0] for f in dvo.GeometricConfig._fields_] == ["struct_size", "mode", "weight", "max_diff"]
    assert [f[0] for f in dvo.GeometricRecord._fields_] == ["n_geo", "mean_sq"]
    assert [f[0] for f in dvo.GeometricLog._fields_] == ["struct_size", "levels", "n_iter", "n_geo", "sum_sq"]


def test_default_config_and_bindings():
    c = dvo.geometric_default_config()
    assert (c.struct_size, c.mode) == (C.sizeof(dvo.GeometricConfig), dvo.GEOMETRIC_ON)
    assert np.float32(c.weight) == np.float32(10.0) and np.float32(c.max_diff) == np.float32(0.1)
    dvo.lib().dvo_geometric_config_default(None)   # (a NULL pointer is ignored)
    for m in ("set_geometric", "last_geometric", "last_geometric_log"):
        assert callable(getattr(dvo.Batch, m, None)), m
        assert not hasattr(dvo.MonoBatch, m), m    # sensor-depth batches only
    assert callable(dvo.op_gn_step_geometric)
    import inspect
    d = {k: v.default for k, v in inspect.signature(dvo.Batch.set_geometric).parameters.items() if k != "self"}
    assert d == dict(mode=dvo.GEOMETRIC_ON, weight=10.0, max_diff=0.1)


def test_null_handle_and_bad_operator_arguments_are_refused():
    L = dvo.lib()
    cfg = dvo.geometric_default_config()
    rec = (dvo.GeometricRecord * 2)()
    lg = dvo.GeometricLog(); lg.struct_size = C.sizeof(dvo.GeometricLog)
    assert L.dvo_batch_set_geometric(None, C.byref(cfg)) == dvo.DVO_ERR_BAD_ARGUMENT
    assert L.dvo_batch_set_geometric(None, None) == dvo.DVO_ERR_BAD_ARGUMENT
    assert L.dvo_batch_last_geometric(None, rec) == dvo.DVO_ERR_BAD_ARGUMENT
    assert L.dvo_batch_last_geometric_log(None, 0, C.byref(lg)) == dvo.DVO_ERR_BAD_ARGUMENT
    out = dvo.GnResult()
    f = C.c_float
    sums = (C.c_double * 2)()
    img = (C.c_float * 16)(); K = (C.c_float * 9)(); xi = (C.c_float * 6)()
    # NULL maps, NULL outputs, a weight or max_diff outside its range: refused before a device is opened
    call = lambda *a: L.dvo_op_gn_step_geometric(0, None, *a)
    assert call(None, None, None, None, None, 4, 4, None, None, 0, f(1.0), f(0.1), C.byref(out), sums) == dvo.DVO_ERR_BAD_ARGUMENT
    assert call(img, img, img, img, None, 4, 4, K, xi, 0, f(1.0), f(0.1), C.byref(out), sums) == dvo.DVO_ERR_BAD_ARGUMENT
    assert call(img, img, img, img, img, 4, 4, K, xi, 0, f(1.0), f(0.1), C.byref(out), None) == dvo.DVO_ERR_BAD_ARGUMENT
    for weight, max_diff in ((-1.0, 0.1), (float("nan"), 0.1), (float("inf"), 0.1), (1.0, 0.0), (1.0, -0.1), (1.0, float("nan")), (1.0, float("inf"))):
        assert call(img, img, img, img, img, 4, 4, K, xi, 0, f(weight), f(max_diff), C.byref(out), sums) == dvo.DVO_ERR_BAD_ARGUMENT, (weight, max_diff)


def test_facade_geometric_methods_compile(tmp_path):
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
    bt.setGeometric();
    bt.setGeometric(DVO_GEOMETRIC_ON, 30.0f, 0.05f);
    std::vector<dvo_geometric_record> r = bt.lastGeometric();
    dvo_geometric_log l = bt.lastGeometricLog(1);
    bt.setGeometric(DVO_GEOMETRIC_OFF);
    return (int)r.size() + r[0].n_geo + l.levels + l.n_geo[0][0];
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


def test_reference_restates_the_oracle(two_frames):
    """the restated warp, sampler and Jacobian give the oracle's photometric J, r and rw bit for bit on every fast-path pixel, at a
    pose away from zero as well; and a whole call with weight 0 on the reference's depth is orc.track bit for bit"""
    obj, ref = two_frames
    wp = gr.weight_params()
    for xi in (np.zeros(6, np.float32), np.float32([0.01, -0.008, 0.012, 0.004, -0.006, 0.009])):
        for l in range(LEVELS):
            px = gr.frame_pixels(obj, ref, False, wp)(l, xi)
            n = gr.self_check(px, obj.gray(l))
            assert px["n_valid"] > 500 and n > 0.8 * px["n_valid"], (l, n, px["n_valid"])
    xo, lo = orc.track(obj, ref, crop=False)
    cfg = dvo.default_config()
    xr, lr = gr.geometric_track(obj, ref, LEVELS, 0.0, 0.1, False, cfg.max_iterations, cfg.min_update, cfg.min_residual, wp=wp, own_depth=False)
    assert list(lr["n_iter"]) == [int(n) for n in lo["n_iter"][:LEVELS]]
    assert xr.tobytes() == np.asarray(xo, np.float32).tobytes(), (xr, xo)
    for l in range(LEVELS):
        assert lr["residual"][l].tobytes() == lo["residual"][l].tobytes() and lr["xi_after"][l].tobytes() == lo["xi_after"][l].tobytes(), l


def test_reference_gates_and_zero_weight(two_frames):
    """weight 0 leaves the exact sums the photometric ones; the gates take rows away and never add a non-finite term; a reference
    depth equal to the warped depth (a plane seen without motion) has a zero residual"""
    import gn_sums
    obj, ref = two_frames
    wp = gr.weight_params()
    xi = np.zeros(6, np.float32)
    l = 2
    px = gr.pixels(obj.gray(l), obj.depth(l), obj.sigma(l), ref.gray(l), ref.depth(l), ref.K(l), xi, l, False, wp)
    plain = gn_sums.exact_sums(px["terms"])
    ex0 = gr.exact(px, 0.0, 0.1)
    assert ex0["n_geo"] > 0.8 * ex0["n"] and ex0["S29"] == 0.0
    np.testing.assert_array_equal(ex0["H"], plain["H"]); np.testing.assert_array_equal(ex0["g"], plain["g"])
    ex = gr.exact(px, 10.0, 0.1)
    assert ex["n_geo"] == ex0["n_geo"] and ex["S29"] > 0 and (ex["H"][[0, 6, 11]] > plain["H"][[0, 6, 11]]).all()
    assert gr.exact(px, 10.0, 1e-7)["n_geo"] < ex["n_geo"]          # max_diff takes rows away
    bad = ref.depth(l).copy()
    bad[20:40, 30:60] = 0.0; bad[50:60, 30:60] = np.nan; bad[70:80, 30:60] = np.inf; bad[90:100, 30:60] += 1.0
    pxb = gr.pixels(obj.gray(l), obj.depth(l), obj.sigma(l), ref.gray(l), bad, ref.K(l), xi, l, False, wp)
    exb = gr.exact(pxb, 10.0, 0.1)
    assert exb["n"] == ex["n"] and exb["n_geo"] < ex["n_geo"] - 1000
    assert np.isfinite(exb["H"]).all() and np.isfinite(exb["g"]).all() and np.isfinite(exb["S29"])
    flat = np.full_like(ref.depth(l), 1.5)
    pxf = gr.pixels(obj.gray(l), flat, obj.sigma(l), ref.gray(l), flat, ref.K(l), xi, l, False, wp)
    assert pxf["fast"].sum() > 1000 and not pxf["rz"][pxf["fast"]].any()
    assert gr.depths(4) == (21, 17, 13) and gr.depths(1) == (12, 11, 10)


# ------------------------------------------------------------------------------------------------ registers of the hot instances
# k_track_gn_z / k_track_gn_z_cam <4, 1 | 2, raster | 2-D tiles>: built for DVO_GN_Z_WAVES = 3 waves per SIMD -- 512 / 3 rounded down
# to the allocation granule of 8 = 168 VGPRs -- without scratch; at 4 (128) they spill
Z_WAVES = 3
Z_VGPR_BUDGET = (512 // Z_WAVES) // 8 * 8


def _meta(txt, name):
    m = re.search(r"\.amdhsa_kernel %s.*?\.end_amdhsa_kernel" % re.escape(name), txt, re.S)
    assert m, "kernel not found: " + name
    body = m.group(0)
    return (int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", body).group(1)), int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body).group(1)))


def test_hot_geometric_kernels_fit_the_register_budget():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    src = open(os.path.join(PKG, "csrc", "dvo_kernels.hip")).read()
    assert re.search(r"#define DVO_GN_Z_WAVES %d\b" % Z_WAVES, src)
    cont = open(os.path.join(PKG, "Makefile")).read().split("FLAGS   =", 1)[1].split("\n")
    flags = (cont[0].rstrip("\\") + " " + cont[1]).split()
    flags = [f.replace("$(ARCH)", "gfx950") for f in flags if f != "-fPIC"]
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "k.s")
        subprocess.run([hipcc] + flags + ["-S", "--cuda-device-only", "-o", out, os.path.join(PKG, "csrc", "dvo_kernels.hip")],
                       check=True, capture_output=True, timeout=900)
        txt = open(out).read()
    checked = 0
    args = "EEEvNS_6GnArgsENS_5GeoGnE"
    for kernel in ("_ZN3dvo12k_track_gn_z", "_ZN3dvo16k_track_gn_z_cam"):
        for variant in ("ILi4ELi1ELb0", "ILi4ELi1ELb1", "ILi4ELi2ELb0", "ILi4ELi2ELb1"):   # <PPT 4, G 1 | 2, T2D>
            vgpr, scratch = _meta(txt, kernel + variant + args)
            assert scratch == 0, "%s%s spills %d bytes of scratch per lane" % (kernel, variant, scratch)
            assert vgpr <= Z_VGPR_BUDGET, "%s%s needs %d VGPRs (budget %d = %d waves per SIMD)" % (kernel, variant, vgpr, Z_VGPR_BUDGET, Z_WAVES)
            checked += 1
    assert checked == 8
    plain = _meta(txt, "_ZN3dvo10k_gn_solveENS_9SolveArgsE")
    z = _meta(txt, "_ZN3dvo12k_gn_solve_zENS_9SolveArgsENS_8GeoSolveE")
    assert z[0] <= plain[0] and z[1] <= plain[1], ("k_gn_solve_z (VGPRs, scratch) %s against k_gn_solve %s" % (z, plain))
    # the other families keep their names and template parameters beside the new one
    assert re.search(r"\.amdhsa_kernel _ZN3dvo10k_track_gnILi4ELi2ELb0ELb0EEEvNS_6GnArgsE\b", txt)
    assert re.search(r"\.amdhsa_kernel _ZN3dvo13k_track_gn_rwILi4ELi2ELb0EEEvNS_6GnArgsENS_8RobustGnE\b", txt)
    assert re.search(r"\.amdhsa_kernel _ZN3dvo13k_track_gn_abILi4ELi2ELb0ELb0EEEvNS_6GnArgsENS_8RobustGnENS_8AffineGnE\b", txt)
