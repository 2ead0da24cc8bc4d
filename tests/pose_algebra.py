"""The pose-algebra fixture, its bounds ("The solve and the SE(3) chain against a multi-precision reference") and the
host shim over csrc/dvo_math.h.  numpy only: the references were frozen by tests/golden/make_pose_algebra.py.

run(op, rows) is anything that evaluates dvo_op_pose_algebra's op on float64 rows: the device (dvo_amd.pose_algebra), the header
compiled for the host, the header's device flavour compiled for the host, or a mutated copy.  check_all(run) returns the largest
error / bound ratio per op and the list of violations; the constants are counted roundings, not fits (see DESIGN.md for each)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "direct-visual-odometry_amd", "csrc")
NPZ = os.path.join(ROOT, "tests", "golden", "pose_algebra.npz")
ROWS = {0: (6, 12), 1: (12, 6), 2: (12, 6), 3: (12, 31), 4: (27, 7), 5: (21, 42)}
U = 2.0 ** -53
T6F = np.float32(1e-6)
LD = np.longdouble

# counted constants
C_R, C_R_TH = 34.0, 5.0          # rotation entries of exp: (C_R + C_R_TH theta) u
C_T, C_T_INV = 223.0, 6.0        # translation of exp: (C_T + C_T_INV / theta) u |v|inf
C_W = 15.0                       # omega of log: C_W u theta
C_V = 700.0                      # translation of log: C_V u |t|inf
C_LDL = 310.0                    # LDL^T solve: C_LDL kappa u |x|inf
C_EIG = 600.0                    # Jacobi: residual, orthogonality and eigenvalues at C_EIG u |H|
C_PINV = 2.0 * C_EIG             # pseudo-inverse: C_PINV kappa u (|x|inf + |g|inf / lambda_min kept)

_fixture = None


def fixture():
    global _fixture
    if _fixture is None:
        with np.load(NPZ) as z:
            _fixture = {k: z[k] for k in z.files}
    return _fixture


def inputs(op):
    f = fixture()
    if op == 0:
        return f["exp_in"]
    if op == 1:
        return f["log_in"]
    if op == 2:
        return f["pair_in"]
    if op == 3:
        return np.concatenate([f["pair_in"], f["rej_in"]])
    if op == 4:
        return f["solve_in"]
    return f["solve_in"][:, :21]


def err(got, hi, lo):
    return np.abs((got.astype(LD) - hi.astype(LD)) - lo.astype(LD)).astype(np.float64)


def ulpd(x):
    """one unit in the last place of the double x (of its binade)"""
    return np.spacing(np.abs(x))


def half_ulp32(ref):
    with np.errstate(over="ignore"):
        return 0.5 * np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64) * (1.0 + 2.0 ** -20)


def f32_gt(q):
    return q.astype(np.float32) > T6F


# ---------------------------------------------------------------- bounds, one row of bounds per case
def _exp_terms(xi):
    """(dR general, dt) of se3_exp_d for float64 twists xi (n, 6): scalars per case"""
    th = np.linalg.norm(xi[:, 3:], axis=1)
    V = np.abs(xi[:, :3]).max(axis=1)
    dR = np.where(th < 2.0 ** -52, 0.0, (C_R + C_R_TH * th) * U)
    with np.errstate(divide="ignore"):
        dt = np.where(f32_gt(th), (C_T + C_T_INV / np.maximum(th, 1e-300)) * U * V, 0.0)
    return th, dR, dt


def bound_exp(xi, ref):
    n = len(xi)
    th, dR, dt = _exp_terms(xi)
    b = np.empty((n, 12))
    b[:, :9] = dR[:, None]
    b[:, 9:] = dt[:, None]
    # a rotation about a coordinate axis: sqrt(fl(x^2)) = |x| exactly, two of rx, ry, rz are zeros, so most entries are one sine or
    # cosine (below one unit in the last place, the claim of libm and of sincos_dev alike) times at most one rounded factor
    w = xi[:, 3:]
    for i in np.nonzero((np.count_nonzero(w, axis=1) == 1) & (th >= 2.0 ** -52))[0]:
        j = int(np.nonzero(w[i])[0][0])
        p, q = [k for k in range(3) if k != j]
        r = ref[i, :9].reshape(3, 3)
        bb = np.zeros((3, 3))
        bb[j, j] = 15 * U
        bb[p, p] = ulpd(r[p, p]); bb[q, q] = ulpd(r[q, q])
        bb[p, q] = ulpd(r[p, q]) + 3 * U * abs(r[p, q]); bb[q, p] = ulpd(r[q, p]) + 3 * U * abs(r[q, p])
        b[i, :9] = bb.ravel()
    return b


def bound_log(rows, ref, aux):
    theta = aux[:, 0]
    T = np.abs(rows[:, 9:]).max(axis=1)
    b = np.empty((len(rows), 6))
    has_w = np.abs(ref[:, 3:]).max(axis=1) > 0
    b[:, 3:] = np.where(has_w, C_W * U * theta, 0.0)[:, None]
    b[:, :3] = np.where(f32_gt(aux[:, 2]), C_V * U * T, 0.0)[:, None]
    return b


def double_term_pair(rows, ref, aux):
    """the double part of ops 2 and 3: exp, exp, product, log, each stage's own roundings and what it passes on"""
    theta, s, wl, tmax, ta, tb = aux.T
    _, dRa, dta = _exp_terms(rows[:, :6])
    _, dRb, dtb = _exp_terms(rows[:, 6:])
    dR = 3 * (dRa + dRb) + 3 * U
    dt = 3 * dRa * tb + 3 * dtb + dta + 4 * U * (3 * tb + ta)
    has_w = np.abs(ref[:, 3:]).max(axis=1) > 0
    with np.errstate(divide="ignore", invalid="ignore"):
        k = np.where(has_w, theta / np.maximum(s, 1e-300), 0.0)
    dw = np.where(has_w, C_W * U * theta + 6.1 * k * dR, 0.0)
    dv = np.where(f32_gt(wl), C_V * U * tmax + 8.2 * dt + 4.0 * dw * tmax, dt)
    b = np.empty((len(rows), 6))
    b[:, :3] = dv[:, None]
    b[:, 3:] = dw[:, None]
    return b


def bound_pair(rows, ref, aux):
    return half_ulp32(ref) + double_term_pair(rows, ref, aux)


def bound_solve(rows, ref, aux):
    pinv, lmax, kmin, nkept = aux[:, 0], aux[:, 1], aux[:, 2], aux[:, 3]
    xmax = np.abs(ref).max(axis=1)
    gmax = np.abs(rows[:, 21:]).max(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        kappa = np.where(nkept > 0, lmax / kmin, 0.0)
        d = np.where(pinv > 0, C_PINV * kappa * U * (xmax + gmax / kmin), C_LDL * kappa * U * xmax)
    d = np.where(nkept > 0, d, 0.0)
    b = half_ulp32(ref) + d[:, None]
    b[nkept == 0] = 0.0                      # max diag <= 0 or nothing kept: x = 0, exactly
    return b


def full6(H21):
    A = np.zeros((6, 6), LD)
    k = 0
    for i in range(6):
        for j in range(i, 6):
            A[i, j] = A[j, i] = H21[k]
            k += 1
    return A


# ---------------------------------------------------------------- the check
class Report:
    def __init__(self):
        self.ratio = {}
        self.bad = []

    def take(self, op, e, b, what):
        e = np.asarray(e, np.float64); b = np.asarray(b, np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(b > 0, e / b, np.where(e == 0, 0.0, np.inf))
        r = np.where(np.isnan(e), np.inf, r)
        self.ratio[op] = max(self.ratio.get(op, 0.0), float(r.max()) if r.size else 0.0)
        for i in np.argwhere(r > 1.0)[:4]:
            self.bad.append("op %d %s case %d entry %s: error %.3e, bound %.3e" % (op, what, i[0], i[1:].tolist(), e[tuple(i)], b[tuple(i)]))

    def fail(self, msg):
        self.bad.append(msg)

    def lines(self):
        return ["op %d: largest error / bound = %.4f" % (op, r) for op, r in sorted(self.ratio.items())]


def bits_equal(a, b):
    a = np.ascontiguousarray(a, np.float64); b = np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and bool(((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))).all())


def check_all(run, ops=(0, 1, 2, 3, 4, 5), flags=True):
    """every op on the whole fixture; flags=False leaves out op 4's pinv flag (the host shim restates it, the header has no such function)"""
    f = fixture()
    rep = Report()
    out = {op: run(op, inputs(op)) for op in ops}
    if 0 in ops:
        ref = f["exp_hi"]
        rep.take(0, err(out[0], ref, f["exp_lo"]), bound_exp(f["exp_in"], ref), "exp")
    if 1 in ops:
        rep.take(1, err(out[1], f["log_hi"], f["log_lo"]), bound_log(f["log_in"], f["log_hi"], f["log_aux"]), "log")
    npair = len(f["pair_in"])
    pb = bound_pair(f["pair_in"], f["pair_hi"], f["pair_aux"])
    if 2 in ops:
        rep.take(2, err(out[2], f["pair_hi"], f["pair_lo"]), pb, "concatenate")
    if 3 in ops:
        o = out[3]
        if not (o[:npair, 0] == 1.0).all():
            rep.fail("op 3 refused a finite update: cases %s" % np.nonzero(o[:npair, 0] != 1.0)[0][:8].tolist())
        rep.take(3, err(o[:npair, 1:7], f["pair_hi"], f["pair_lo"]), pb, "update")
        # the state that goes with xi': exp(xi') in double and float(exp(-xi')), bit for bit what op 0 gives for xi' and -xi'
        fin = np.nonzero(o[:, 0] == 1.0)[0]
        xin = o[fin, 1:7]
        if np.isfinite(xin).all():
            ep, em = run(0, xin), run(0, -xin)
            if not bits_equal(o[fin, 7:19], ep):
                rep.fail("op 3: Tc' is not op 0 of xi' (%d cases)" % int((o[fin, 7:19] != ep).any(axis=1).sum()))
            if not bits_equal(o[fin, 19:31], em.astype(np.float32).astype(np.float64)):
                rep.fail("op 3: pose is not float32(op 0 of -xi') (%d cases)" % int((o[fin, 19:31] != em.astype(np.float32)).any(axis=1).sum()))
        else:
            rep.fail("op 3 accepted a non-finite pose")
        if 2 in ops and not bits_equal(o[:npair, 1:7], out[2]):
            rep.fail("op 3: xi' is not op 2 of (xi, upd)")
        # refused updates: flag 0 where the fixture says the result has a NaN; a refused update leaves xi, Tc and pose as they were
        rej = o[npair:]
        rin = f["rej_in"]
        must = f["rej_must"]
        if not (rej[must == 1, 0] == 0.0).all():
            rep.fail("op 3 accepted an update whose result is NaN")
        keep = np.nonzero(rej[:, 0] == 0.0)[0]
        if len(keep):
            x0 = rin[keep, :6]
            same = bits_equal(rej[keep, 1:7], x0) and bits_equal(rej[keep, 7:19], run(0, x0)) and \
                bits_equal(rej[keep, 19:31], run(0, -x0).astype(np.float32).astype(np.float64))
            if not same:
                rep.fail("op 3: a refused update changed xi, Tc or pose")
        acc = np.nonzero(rej[:, 0] == 1.0)[0]
        if len(acc) and np.isnan(rej[acc, 1:7]).any():
            rep.fail("op 3 accepted a NaN pose")
    if 4 in ops:
        tag = f["solve_tag"]
        ok = tag == 0
        o = out[4]
        rep.take(4, err(o[ok, :6], f["solve_hi"][ok], f["solve_lo"][ok]), bound_solve(f["solve_in"][ok], f["solve_hi"][ok], f["solve_aux"][ok]), "solve")
        H = f["solve_in"][:, :21]
        for i in np.nonzero(ok)[0]:                      # an exactly zero row and column: x is exactly 0 there
            A = full6(H[i])
            for r_ in range(6):
                if not A[r_].any() and A.any() and o[i, r_] != 0.0:
                    rep.fail("op 4 case %d: x[%d] = %g along an exactly zero row" % (i, r_, o[i, r_]))
        if flags and not (o[ok, 6] == f["solve_aux"][ok, 0]).all():
            rep.fail("op 4: pinv flag differs from the reference's branch in cases %s" % np.nonzero(ok)[0][o[ok, 6] != f["solve_aux"][ok, 0]].tolist())
        if np.isfinite(o[tag == 1, :6]).all(axis=1).any():
            rep.fail("op 4: a system with a NaN sum gave a finite x")
    if 5 in ops:
        tag = f["solve_tag"]
        o = out[5]
        e_res, e_orth, e_lam, bnd = [], [], [], []
        for i in np.nonzero(tag == 0)[0]:
            A = full6(f["solve_in"][i, :21])
            d = o[i, :6].astype(LD); V = o[i, 6:].reshape(6, 6).astype(LD)
            hn = float(np.sqrt((A * A).sum()))
            e_res.append(float(np.abs(A @ V - V * d[None, :]).max()))
            e_orth.append(float(np.abs(V.T @ V - np.eye(6, dtype=LD)).max()) * hn)
            e_lam.append(float(np.abs(np.sort(d) - f["solve_aux"][i, 4:10].astype(LD)).max()))
            bnd.append(C_EIG * U * hn)
        rep.take(5, np.array([e_res, e_orth, e_lam]).T, np.array([bnd, bnd, bnd]).T, "eig (residual, orthogonality, eigenvalues)")
    return rep, out


# ---------------------------------------------------------------- the header on the host
SHIM = r"""
#include "dvo_math.h"
using namespace dvo;
// solve6's choice of solve6_pinv, as csrc/dvo_kernels.hip restates it for the device (solve6_takes_pinv)
static bool takes_pinv(const double H[21])
{
    double maxd = 0;
    for (int i = 0; i < 6; i++) maxd = H[tri(i, i)] > maxd ? H[tri(i, i)] : maxd;
    if (!(maxd > 0.0)) return false;
    double L[6][6], d[6];
    bool ok = true;
    for (int j = 0; j < 6; j++) {
        double dj = H[tri(j, j)];
        for (int k = 0; k < j; k++) dj -= L[j][k] * L[j][k] * d[k];
        ok = ok && (dj > 1e-12 * maxd);
        d[j] = dj;
        const double inv = 1.0 / dj;
        for (int i = j + 1; i < 6; i++) {
            double v = H[tri(j, i)];
            for (int k = 0; k < j; k++) v -= L[i][k] * L[j][k] * d[k];
            L[i][j] = v * inv;
        }
    }
    return !ok;
}
extern "C" void pose_algebra(int op, int n, const double* in, double* out)
{
    static const int NI[6] = {6, 12, 12, 12, 27, 21}, NO[6] = {12, 6, 6, 31, 7, 42};
    for (int i = 0; i < n; i++) {
        const double* p = in + (long long)i * NI[op];
        double* o = out + (long long)i * NO[op];
        if (op == 0) {
            double xi[6], R[9], t[3];
            for (int k = 0; k < 6; k++) xi[k] = p[k];
            se3_exp_d(xi, R, t);
            for (int k = 0; k < 9; k++) o[k] = R[k];
            for (int k = 0; k < 3; k++) o[9 + k] = t[k];
        } else if (op == 1) {
            double R[9], t[3], xi[6];
            for (int k = 0; k < 9; k++) R[k] = p[k];
            for (int k = 0; k < 3; k++) t[k] = p[9 + k];
            se3_log_d(R, t, xi);
            for (int k = 0; k < 6; k++) o[k] = xi[k];
        } else if (op == 2) {
            float a[6], b[6], c[6];
            for (int k = 0; k < 6; k++) { a[k] = (float)p[k]; b[k] = (float)p[6 + k]; }
            se3_concatenate_f(a, b, c);
            for (int k = 0; k < 6; k++) o[k] = c[k];
        } else if (op == 3) {
            float xi[6], upd[6];
            double xd[6], Tc[12];
            Pose pose;
            for (int k = 0; k < 6; k++) { xi[k] = (float)p[k]; upd[k] = (float)p[6 + k]; xd[k] = xi[k]; }
            pose_from_xi(xi, -1.0f, pose);
            se3_exp_d(xd, Tc, Tc + 9);
            o[0] = se3_update_pose(Tc, upd, xi, pose) ? 1.0 : 0.0;
            for (int k = 0; k < 6; k++) o[1 + k] = xi[k];
            for (int k = 0; k < 12; k++) o[7 + k] = Tc[k];
            for (int k = 0; k < 9; k++) o[19 + k] = pose.R[k];
            for (int k = 0; k < 3; k++) o[28 + k] = pose.t[k];
        } else if (op == 4) {
            double H[21], g[6];
            float x[6];
            for (int k = 0; k < 21; k++) H[k] = p[k];
            for (int k = 0; k < 6; k++) g[k] = p[21 + k];
            solve6(H, g, x);
            for (int k = 0; k < 6; k++) o[k] = x[k];
            o[6] = takes_pinv(H) ? 1.0 : 0.0;
        } else {
            double A[36], V[36];
            for (int r = 0, k = 0; r < 6; r++)
                for (int c = r; c < 6; c++, k++) { A[6 * r + c] = p[k]; A[6 * c + r] = p[k]; }
            jacobi_eig6(A, V);
            for (int k = 0; k < 6; k++) o[k] = A[7 * k];
            for (int k = 0; k < 36; k++) o[6 + k] = V[k];
        }
    }
}
"""

SE3_BEGIN = "// ---------------------------------------------------------------- SE(3) in double"
SE3_END = "// ---------------------------------------------------------------- 6x6 solve"


def sub_exact(text, old, new, count):
    """replace old by new, asserting that old occurs exactly count times"""
    n = len(re.findall(re.escape(old), text))
    assert n == count, "%r occurs %d times, expected %d" % (old, n, count)
    return text.replace(old, new)


def header_text():
    return open(os.path.join(CSRC, "dvo_math.h")).read()


def device_flavour(text):
    """the header with the SE(3) section's device code opened for a host compiler: sincos_dev, katan_d and atan2_dev then run on
    the host with true fma().  Only the text between the two banners is edited."""
    i, j = text.index(SE3_BEGIN), text.index(SE3_END)
    assert 0 < i < j
    sec = text[i:j]
    sec = sub_exact(sec, "#if defined(__HIPCC__)", "#if 1", 1)
    sec = sub_exact(sec, "#if defined(__HIP_DEVICE_COMPILE__)", "#if 1", 4)
    sec = sub_exact(sec, "__device__ __forceinline__", "inline", 5)
    return text[:i] + sec + text[j:]


def build_shim(workdir, text=None):
    """compile the shim over csrc/dvo_math.h (or over text, a modified copy of it) with the library's float flags; returns run(op, rows)"""
    os.makedirs(str(workdir), exist_ok=True)
    inc = CSRC
    if text is not None:
        inc = str(workdir)
        with open(os.path.join(inc, "dvo_math.h"), "w") as fh:
            fh.write(text)
    src, so = os.path.join(str(workdir), "shim.cpp"), os.path.join(str(workdir), "libposeshim.so")
    with open(src, "w") as fh:
        fh.write(SHIM)
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-shared", "-fPIC", "-I", inc, "-o", so, src])
    L = C.CDLL(so)
    L.pose_algebra.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.pose_algebra.restype = None

    def run(op, rows):
        ni, no = ROWS[op]
        rows = np.ascontiguousarray(rows, np.float64).reshape(-1, ni)
        out = np.zeros((len(rows), no), np.float64)
        L.pose_algebra(op, len(rows), rows.ctypes.data, out.ctypes.data)
        return out
    return run
