"""CPU tests of step control (include/dvo.h, dvo_batch_set_step_control and dvo_op_lm_step): the entry points are
declared, exported, bound and in the C++ facade, every refusal that needs no handle is returned, the header states the contract, the
replica of tests/lm_ref.py meets its anchor bit for bit -- lambda0 = 0 without rejects is robust_ref.irls_track(kind NONE) on the level
both start from the same pose, one step behind at the level's end -- and its accepted residuals never increase on a workload that
rejects, and the new kernels compile for gfx950 with k_gn_solve_lm's scratch no larger than k_gn_solve_rw's."""
import ctypes as C
import inspect
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import dvo_amd as dvo
import lm_ref as lr
import orc
import robust_ref as rr
from dvo_amd import synth
from util import K640

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "direct-visual-odometry_amd")
SIGNATURES = {
    "dvo_lm_config_default": (r"void", r"dvo_lm_config\s*\*\s*\w+"),
    "dvo_batch_set_step_control": (r"int", r"dvo_batch\s*\*\s*\w+\s*,\s*const\s+dvo_lm_config\s*\*\s*\w+"),
    "dvo_batch_last_step_control": (r"int", r"dvo_batch\s*\*\s*\w+\s*,\s*dvo_lm_record\s*\*\s*\w+"),
    "dvo_batch_last_step_control_log": (r"int", r"dvo_batch\s*\*\s*\w+\s*,\s*int\s+seq\s*,\s*dvo_lm_log\s*\*\s*\w+"),
    "dvo_op_lm_step": (r"int", r"int\s+dev\s*,\s*int\s+n\s*,\s*const\s+double\s*\*\s*sums\s*,\s*const\s+float\s*\*\s*xi_eval\s*,\s*const\s+dvo_lm_entry\s*\*\s*entry_in\s*,"
                               r"\s*const\s+dvo_lm_config\s*\*\s*cfg\s*,\s*int\s+level_first\s*,\s*int\s+it_prev\s*,\s*int\s+max_iterations\s*,\s*int\s+fixed_iterations\s*,"
                               r"\s*float\s+min_update\s*,\s*float\s+min_residual\s*,\s*dvo_lm_entry\s*\*\s*entry_out\s*,\s*float\s*\*\s*update\s*,\s*float\s*\*\s*xi_next\s*,"
                               r"\s*int\s*\*\s*decision\s*,\s*int\s*\*\s*active"),
}


@pytest.mark.parametrize("name", sorted(SIGNATURES))
def test_declared_exported_and_listed(name):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dvo.h")).read(), flags=re.S)
    ret, args = SIGNATURES[name]
    assert re.search(r"\b%s\s+%s\s*\(\s*%s\s*\)\s*;" % (ret, name, args), txt), name
    assert hasattr(dvo.lib(), name)
    assert name in dvo.EXPORTS
    assert "dvo_*" in open(os.path.join(PKG, "csrc", "libdvo.map")).read()   # (the map exports the C ABI by its prefix)


def test_header_states_the_contract():
    txt = open(os.path.join(ROOT, "include", "dvo.h")).read()
    flat = re.sub(r"\s+", " ", re.sub(r"\n \*", " ", txt))
    for phrase in ("n_valid > 0 && (float)n_valid >= min_valid_fraction * (float)n_acc && residual <= residual_acc",
                   "a NaN residual rejects, a tie accepts", "lambda = lambda * lambda_down",
                   "lambda = fminf(fmaxf(lambda, lambda_floor) * lambda_up, lambda_max)", "times 1.0 + (double)lambda",
                   "With n_acc == 0 the update is zero", "a non-finite update", "a sequence that stops holds the accepted pose",
                   "A level therefore always ends on an evaluated, accepted pose", "the accepted residuals never increase",
                   "xi_after is the pose the sequence holds after the iteration", "receives the accepted sums of the finest level",
                   "only the pose the level ends on is one step behind", "k_track_gn + k_gn_solve_lm",
                   "runs exactly the launches it always ran", "all zeros for a sequence that did not track",
                   "Step control together with those terms, and dvo_vo handles, are out of scope"):
        assert phrase in flat, phrase
    for name, value in (("DVO_LM_OFF", 0), ("DVO_LM_ON", 1), ("DVO_LM_FIRST", 1), ("DVO_LM_ACCEPT", 2), ("DVO_LM_REJECT", 3)):
        assert re.search(r"#define %s\s+%d\b" % (name, value), txt), name
    assert (dvo.LM_OFF, dvo.LM_ON, dvo.LM_FIRST, dvo.LM_ACCEPT, dvo.LM_REJECT) == (0, 1, 1, 2, 3)
    assert (lr.FIRST, lr.ACCEPT, lr.REJECT) == (dvo.LM_FIRST, dvo.LM_ACCEPT, dvo.LM_REJECT)


def test_bindings_and_defaults():
    for cls in (dvo.Batch, dvo.MonoBatch):
        for m in ("set_step_control", "last_step_control", "last_step_control_log", "op_lm_step"):
            assert callable(getattr(cls, m, None)), (cls, m)
    assert callable(dvo.op_lm_step)
    d = {k: v.default for k, v in inspect.signature(dvo.Batch.set_step_control).parameters.items() if k != "self"}
    assert d == dict(mode=dvo.LM_ON, **lr.DEFAULTS)
    c = dvo.lm_default_config()
    assert c.struct_size == C.sizeof(dvo.LmConfig) == 32 and c.mode == dvo.LM_ON
    for k, v in lr.DEFAULTS.items():
        assert np.float32(getattr(c, k)) == np.float32(v), k
    dvo.lib().dvo_lm_config_default(None)   # (a NULL config is ignored)
    assert C.sizeof(dvo.LmEntry) == 408 and C.sizeof(dvo.LmRecord) == 20 and dvo.LM_ENTRY_DTYPE.itemsize == 408
    assert C.sizeof(dvo.LmLog) == 8 + 4 * dvo.MAX_LEVELS + 8 * dvo.MAX_LEVELS * dvo.MAX_ITERATIONS


BAD_CONFIGS = [dict(lambda0=-1.0), dict(lambda0=float("nan")), dict(lambda0=float("inf")), dict(lambda_up=1.0), dict(lambda_up=0.5),
               dict(lambda_up=float("nan")), dict(lambda_up=float("inf")), dict(lambda_down=0.0), dict(lambda_down=1.5),
               dict(lambda_down=-0.5), dict(lambda_down=float("nan")), dict(lambda_floor=0.0), dict(lambda_floor=-1e-4),
               dict(lambda_floor=float("nan")), dict(lambda_floor=float("inf")), dict(lambda_max=1e-5), dict(lambda_max=float("nan")),
               dict(lambda_max=float("inf")), dict(lambda_max=-1.0), dict(min_valid_fraction=-0.1), dict(min_valid_fraction=1.1),
               dict(min_valid_fraction=float("nan")), dict(struct_size=28), dict(mode=2), dict(mode=dvo.LM_OFF)]


def test_null_and_bad_arguments_are_refused():
    L = dvo.lib()
    c = dvo.lm_default_config()
    rec = (dvo.LmRecord * 2)()
    lg = dvo.LmLog()
    lg.struct_size = C.sizeof(dvo.LmLog)
    assert L.dvo_batch_set_step_control(None, C.byref(c)) == dvo.DVO_ERR_BAD_ARGUMENT
    assert L.dvo_batch_set_step_control(None, None) == dvo.DVO_ERR_BAD_ARGUMENT
    assert L.dvo_batch_last_step_control(None, rec) == dvo.DVO_ERR_BAD_ARGUMENT
    assert L.dvo_batch_last_step_control_log(None, 0, C.byref(lg)) == dvo.DVO_ERR_BAD_ARGUMENT
    # the operator: NULL pointers, n < 1 and every config the setter refuses, before a device is opened
    sums = (C.c_double * 29)(); xi = (C.c_float * 6)(); ent = dvo.LmEntry(); out = dvo.LmEntry()
    upd = (C.c_float * 6)(); nxt = (C.c_float * 6)(); dec = C.c_int(); act = C.c_int()
    f = C.c_float

    def call(n, cfg, ptrs):
        s, x, e, o, u, t, d, a = ptrs
        return L.dvo_op_lm_step(0, n, s, x, e, cfg, 1, 0, 15, 0, f(2e-5), f(0.0), o, u, t, d, a)
    ptrs = [sums, xi, C.byref(ent), C.byref(out), upd, nxt, C.byref(dec), C.byref(act)]
    for k in range(len(ptrs)):
        p = list(ptrs); p[k] = None
        assert call(1, C.byref(c), p) == dvo.DVO_ERR_BAD_ARGUMENT, k
    assert call(1, None, ptrs) == dvo.DVO_ERR_BAD_ARGUMENT
    assert call(0, C.byref(c), ptrs) == dvo.DVO_ERR_BAD_ARGUMENT and call(-3, C.byref(c), ptrs) == dvo.DVO_ERR_BAD_ARGUMENT
    for bad in BAD_CONFIGS:
        b = dvo.lm_default_config()
        for k, v in bad.items():
            setattr(b, k, v)
        assert call(1, C.byref(b), ptrs) == dvo.DVO_ERR_BAD_ARGUMENT, bad
        assert L.dvo_last_error().decode().startswith("dvo_op_lm_step: "), bad
    # a valid configuration passes the checks and fails loudly at the device (no CPU fallback) -- or runs, where there is one
    assert call(1, C.byref(c), ptrs) in (dvo.DVO_OK, dvo.DVO_ERR_NO_DEVICE, dvo.DVO_ERR_HIP)


def test_facade_methods_compile(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("g++ not available")
    src = tmp_path / "snippet.cpp"
    src.write_text(r"""
#include "dvo.hpp"
#include <vector>
static_assert(sizeof(dvo_lm_entry) == 408 && sizeof(dvo_lm_record) == 20 && sizeof(dvo_lm_config) == 32, "layout of the step-control structs");
int use()
{
    const dvo::Mat3 K{525.f, 0.f, 319.5f, 0.f, 525.f, 239.5f, 0.f, 0.f, 1.f};
    dvo::BatchTracker bt(4, K, 640, 480);
    bt.setStepControl();
    bt.setStepControl(DVO_LM_ON, 0.0f, 8.0f, 0.5f, 1e-4f, 1e6f, 0.5f);
    std::vector<dvo_lm_record> r = bt.lastStepControl();
    dvo_lm_log lg = bt.lastStepControlLog(0);
    bt.setStepControl(DVO_LM_OFF);
    dvo::BatchMono bm(2, K, 640, 480);
    bm.setStepControl();
    std::vector<dvo_lm_record> rm = bm.lastStepControl();
    dvo_lm_log lm = bm.lastStepControlLog(1);
    return (int)r.size() + (int)rm.size() + lg.levels + lm.decision[0][0] + r[0].n_rejected;
}
""")
    r = subprocess.run([gxx, "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


# ------------------------------------------------------------------------------------------------ the decision rule in float32
def test_decision_rule():
    P = lr.params()
    f = np.float32
    assert lr.decide(True, 0, f(-1), 100, f(1e-3), f(1), P) == (lr.FIRST, f(1))                       # unconditional, lambda unchanged
    assert lr.decide(False, 100, f(1e-3), 100, f(1e-3), f(1), P) == (lr.ACCEPT, f(0.5))               # a tie accepts
    assert lr.decide(False, 100, np.nextafter(f(1e-3), f(1)), 100, f(1e-3), f(1), P) == (lr.REJECT, f(4))
    assert lr.decide(False, 49, f(1e-4), 100, f(1e-3), f(1), P) == (lr.REJECT, f(4))                  # below the fraction
    assert lr.decide(False, 50, f(1e-4), 100, f(1e-3), f(1), P) == (lr.ACCEPT, f(0.5))
    assert lr.decide(False, 0, f(-1), 100, f(1e-3), f(1), P)[0] == lr.REJECT                          # no pixels
    assert lr.decide(False, 100, f(np.nan), 100, f(1e-3), f(1), P)[0] == lr.REJECT                    # NaN rejects
    assert lr.decide(False, 100, f(1), 100, f(1e-3), f(0), P) == (lr.REJECT, f(1e-4) * f(4))          # raised from the floor
    assert lr.decide(False, 100, f(1), 100, f(1e-3), f(5e5), P) == (lr.REJECT, f(1e6))                # clamped
    assert lr.decide(False, 10, f(1e-4), 0, f(-1), f(1), P)[0] == lr.REJECT                           # nothing accepted yet: -1 is no bound
    H = np.arange(21, dtype=np.float64) + 1
    D = lr.damped(H, f(0.25))
    assert all(D[i] == H[i] * 1.25 for i in lr.DIAG) and all(D[i] == H[i] for i in range(21) if i not in lr.DIAG)
    assert lr.DIAG == tuple(i * 6 - i * (i - 1) // 2 for i in range(6))


# ------------------------------------------------------------------------------------------------ the replica: anchor and monotone
LEVELS, CULLS = 3, 1
KH = np.array(K640, np.float32).copy()
KH[0] *= 0.5
KH[1] *= 0.5
STEPS = (1.0, 0.75, 0.5)


def _pair(sigma, **kw):
    g, d, s, _ = synth.sequence(2, width=320, height_px=240, K=KH, seed=42, sigma_value=sigma, **kw)
    g, d, s = g.numpy(), d.numpy(), s.numpy()
    return orc.OFrame(g[1], d[1], s[1], KH, LEVELS, CULLS), orc.OFrame(g[0], d[0], s[0], KH, LEVELS, CULLS)


def test_lambda_zero_is_the_plain_iteration_one_step_behind():
    orc.set_tracker_params(step3=STEPS, min_residual=0.0, min_update=2e-5)
    try:
        obj, ref = _pair(0.5)
        xp, lp = rr.irls_track(obj, ref, LEVELS, rr.NONE, 1.0, 0.0, False, 6, 2e-5, 0.0)
        xl, ll = lr.lm_track(lr.term_sums(obj, ref), LEVELS, lr.params(lambda0=0.0, lambda_floor=1e-30), 6, 2e-5, 0.0)
    finally:
        orc.set_tracker_params()
    n = int(ll["n_iter"][0])
    assert n == lp["n_iter"][0] and n >= 3
    assert list(ll["decision"][0]) == [lr.FIRST] + [lr.ACCEPT] * (n - 1) and not ll["lambda_"][0].any()   # inputs that never reject
    assert ll["residual"][0].tobytes() == lp["residual"][0].tobytes()                  # every evaluated pose, every logged sum
    assert ll["xi_after"][0][:n - 1].tobytes() == lp["xi_after"][0][:n - 1].tobytes()
    assert ll["xi_after"][0][n - 1].tobytes() == lp["xi_after"][0][n - 2].tobytes()    # the level ends one step behind
    for l in range(LEVELS):                                                            # and every level ends on its accepted pose
        assert list(ll["decision"][l][1:]).count(lr.REJECT) == 0


def test_accepted_residuals_never_increase_where_steps_are_rejected():
    """the reference's own constants on sigma 0.1: the plain iteration is over-relaxed there"""
    orc.set_tracker_params(min_residual=0.0, min_update=2e-5)
    try:
        obj, ref = _pair(0.1)
        xl, ll = lr.lm_track(lr.oracle_sums(obj, ref), LEVELS, lr.params(), 15, 2e-5, 0.0)
    finally:
        orc.set_tracker_params()
    rejects = sum(int((d == lr.REJECT).sum()) for d in ll["decision"])
    assert rejects >= 3 and ll["evaluations"] == sum(ll["n_iter"])
    for l in range(LEVELS):
        acc = ll["accepted"][l]
        assert all(a >= b for a, b in zip(acc, acc[1:])), (l, acc)
        d, res = ll["decision"][l], ll["residual"][l]
        for it in range(1, len(d)):   # a rejected evaluation is worse than the entry, an accepted one is the new entry
            assert (res[it] > acc[it - 1]) == (d[it] == lr.REJECT) or ll["n_valid"][l][it] == 0, (l, it)
            assert acc[it] == (acc[it - 1] if d[it] == lr.REJECT else res[it]), (l, it)
        # lambda follows the decisions
        lam = ll["lambda_"][l]
        for it in range(1, len(d)):
            assert (lam[it] > lam[it - 1]) == (d[it] == lr.REJECT), (l, it)
    assert xl.tobytes() == ll["xi_after"][LEVELS - 1][-1].tobytes()


# ------------------------------------------------------------------------------------------------ registers of the new kernels
def _meta(txt, name):
    m = re.search(r"\.amdhsa_kernel %s.*?\.end_amdhsa_kernel" % re.escape(name), txt, re.S)
    assert m, "kernel not found: " + name
    body = m.group(0)
    return (int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", body).group(1)), int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body).group(1)))


def test_new_kernels_compile_and_the_solve_keeps_its_scratch():
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
    lm = _meta(txt, "_ZN3dvo13k_gn_solve_lmENS_9SolveArgsENS_7LmSolveE")
    rw = _meta(txt, "_ZN3dvo13k_gn_solve_rwENS_9SolveArgsENS_11RobustSolveE")
    assert lm[1] <= rw[1], "k_gn_solve_lm (VGPRs, scratch) %s against k_gn_solve_rw %s" % (lm, rw)
    assert lm[0] <= 512, "k_gn_solve_lm needs %d VGPRs: more than a wave has" % lm[0]   # (280 as built: one workgroup per CU)
    begin = _meta(txt, "_ZN3dvo10k_lm_beginENS_11LmBeginArgsE")
    assert begin[1] == 0
    _meta(txt, "_ZN3dvo9k_lm_stepENS_9SolveArgsENS_7LmSolveEPKdPKfii")
    # the plain kernels it runs beside keep their names
    assert re.search(r"\.amdhsa_kernel _ZN3dvo10k_gn_solveENS_9SolveArgsE\b", txt)
    assert re.search(r"\.amdhsa_kernel _ZN3dvo10k_track_gnILi4ELi2ELb0ELb0EEEvNS_6GnArgsE\b", txt)
