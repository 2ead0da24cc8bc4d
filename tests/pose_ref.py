"""Multi-precision reference (mpmath, 60 digits) of the pose chain AS csrc/dvo_math.h DEFINES IT: se3 exp / log / concatenate with
their small-angle rules, and the 6x6 solve with its pivot rule and pseudo-inverse cut.  Not an idealised matrix logarithm: an exact
half turn logs to omega = 0 here, as in the code.

The rules read rounded quantities (float32(theta) > 1e-6f, a pivot against 1e-12 * max diag, ...), so a case is only usable when
its branch is the same for the exact value and for any double evaluation of it.  Every decision below asserts that (Undecided): the
deciding quantity is 1e-3 relative away from the threshold, or within 2^-40 relative of a float32 value (then a double evaluation,
a few 2^-53 off, rounds to that same float32); for the solve a factor 4 from the pivot rule and from the cut.  That is a condition
on the inputs of tests/pose_cases.py, not a tolerance on results.

Only tests/golden/make_pose_algebra.py and the regeneration test import this module; the GPU run reads the frozen fixture."""
import mpmath as mp
import numpy as np

mp.mp.dps = 60
T6 = mp.mpf(float(np.float32(1e-6)))       # 1e-6f
TINY = mp.mpf(2) ** -52                     # 2.220446049250313e-16
MARGIN = mp.mpf(10) ** -3
PIVOT_RULE = mp.mpf(10) ** -12
CUT = 2 * mp.mpf(2) ** -23                  # 2 FLT_EPSILON


class Undecided(AssertionError):
    pass


def M(x):
    return mp.mpf(float(x))


def vec(a):
    return [M(x) for x in np.asarray(a, np.float64).ravel()]


def f32_gt(q, what):
    """float32(q) > 1e-6f for q >= 0, the same for q and for every double within a few 2^-53 of it"""
    if q == 0 or abs(q / T6 - 1) >= MARGIN:
        return q > T6
    f = M(np.float32(float(q)))
    if abs(q - f) > abs(q) * mp.mpf(2) ** -40:
        raise Undecided("%s = %s is neither clear of 1e-6f nor a float32 value" % (what, mp.nstr(q, 20)))
    return f > T6


def below_tiny(q, what):
    if q != 0 and abs(q / TINY - 1) < MARGIN:
        raise Undecided("%s = %s is at 2^-52" % (what, mp.nstr(q, 20)))
    return q < TINY


def cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def norm(a):
    return mp.sqrt(sum(x * x for x in a))


def exp(xi):
    """xi[6] (mpf) -> R[9], t[3]"""
    v, w = xi[:3], xi[3:]
    th = norm(w)
    if below_tiny(th, "exp theta"):
        R = [mp.mpf(1), 0, 0, 0, mp.mpf(1), 0, 0, 0, mp.mpf(1)]
        R = [mp.mpf(x) for x in R]
    else:
        c, s = mp.cos(th), mp.sin(th)
        c1 = 1 - c
        rx, ry, rz = (x / th for x in w)
        R = [c + c1 * rx * rx, c1 * rx * ry - s * rz, c1 * rx * rz + s * ry,
             c1 * rx * ry + s * rz, c + c1 * ry * ry, c1 * ry * rz - s * rx,
             c1 * rx * rz - s * ry, c1 * ry * rz + s * rx, c + c1 * rz * rz]
    if f32_gt(th, "exp theta"):
        A, B = (1 - mp.cos(th)) / th ** 2, (th - mp.sin(th)) / th ** 3
        wv = cross(w, v)
        wwv = cross(w, wv)
        t = [v[i] + A * wv[i] + B * wwv[i] for i in range(3)]
    else:
        t = list(v)
    return R, t


def log(R, t, aux=None):
    """R[9], t[3] -> xi[6]; aux (a dict) receives theta, s = |antisymmetric part| and |omega|"""
    a = [(R[7] - R[5]) / 2, (R[2] - R[6]) / 2, (R[3] - R[1]) / 2]
    s = norm(a)
    cth = (R[0] + R[4] + R[8] - 1) / 2
    th = mp.atan2(s, cth) if (s != 0 or cth != 0) else mp.mpf(0)
    w = [mp.mpf(0)] * 3
    if s > 0 and f32_gt(th, "log theta"):
        w = [x * th / s for x in a]
    wl = norm(w)
    v = list(t)
    if f32_gt(wl, "log |omega|"):
        half = wl / 2
        coef = (1 - wl * mp.cos(half) / (2 * mp.sin(half))) / wl ** 2
        wt = cross(w, t)
        wwt = cross(w, wt)
        v = [t[i] - wt[i] / 2 + coef * wwt[i] for i in range(3)]
    if aux is not None:
        aux.update(theta=th, s=s, wl=wl)
    return v + w


def compose(Ra, ta, Rb, tb):
    R = [Ra[3 * r] * Rb[c] + Ra[3 * r + 1] * Rb[3 + c] + Ra[3 * r + 2] * Rb[6 + c] for r in range(3) for c in range(3)]
    t = [Ra[3 * r] * tb[0] + Ra[3 * r + 1] * tb[1] + Ra[3 * r + 2] * tb[2] + ta[r] for r in range(3)]
    return R, t


def concatenate(a, b, aux=None):
    """log(exp(a) exp(b)) before its one rounding to float; aux receives the product's theta, s and |t|inf"""
    Ra, ta = exp(a)
    Rb, tb = exp(b)
    R, t = compose(Ra, ta, Rb, tb)
    x = log(R, t, aux)
    if aux is not None:
        aux.update(tmax=max(abs(y) for y in t), tb=max(abs(y) for y in tb), ta=max(abs(y) for y in ta))
    return x


def full6(H21):
    A = mp.zeros(6, 6)
    k = 0
    for i in range(6):
        for j in range(i, 6):
            A[i, j] = H21[k]
            A[j, i] = H21[k]
            k += 1
    return A


def eig6(H21):
    """ascending eigenvalues and the eigenvectors (columns) of the symmetric matrix"""
    E, Q = mp.eigsy(full6(H21))
    order = sorted(range(6), key=lambda i: E[i])
    return [E[i] for i in order], [[Q[r, i] for r in range(6)] for i in order]


def solve(H21, g, aux=None):
    """x[6] and whether the rule sends the system to the pseudo-inverse; aux receives the eigenvalues and the retained ones"""
    A = full6(H21)
    maxd = max([A[i, i] for i in range(6)] + [mp.mpf(0)])
    lam, vecs = eig6(H21)
    if aux is not None:
        aux.update(lam=lam, kept=[], maxd=maxd)
    if not maxd > 0:
        return [mp.mpf(0)] * 6, False
    # exact LDL^T pivots, in the code's order; the factorisation stops at the first pivot the rule refuses
    L = mp.eye(6)
    d = [mp.mpf(0)] * 6
    ok = True
    for j in range(6):
        dj = A[j, j] - sum(L[j, k] ** 2 * d[k] for k in range(j))
        lim = PIVOT_RULE * maxd
        if dj != 0 and lim / 4 < abs(dj) < lim * 4:
            raise Undecided("pivot %d = %s within a factor 4 of the rule %s" % (j, mp.nstr(dj, 8), mp.nstr(lim, 8)))
        d[j] = dj
        if not dj > lim:
            ok = False
            break
        for i in range(j + 1, 6):
            L[i, j] = (A[j, i] - sum(L[i, k] * L[j, k] * d[k] for k in range(j))) / dj
    if ok:
        x = mp.lu_solve(A, mp.matrix(g))
        if aux is not None:
            aux["kept"] = list(lam)
        return [x[i] for i in range(6)], False
    sv = [mp.sqrt(l) if l > 0 else mp.mpf(0) for l in lam]
    thr = CUT * sum(sv)
    x = [mp.mpf(0)] * 6
    kept = []
    for l, s, q in zip(lam, sv, vecs):
        if s != 0 and thr / 4 < s < thr * 4:
            raise Undecided("sqrt(lambda) = %s within a factor 4 of the cut %s" % (mp.nstr(s, 8), mp.nstr(thr, 8)))
        if not s > thr:
            continue
        kept.append(l)
        proj = sum(q[k] * g[k] for k in range(6)) / l
        x = [x[k] + q[k] * proj for k in range(6)]
    if aux is not None:
        aux["kept"] = kept
    return x, True


def hi_lo(values):
    """mpf list -> (hi, lo) float64 arrays with hi + lo the value to about 2^-106"""
    hi = np.array([float(x) for x in values], np.float64)
    lo = np.array([float(x - M(h)) if np.isfinite(h) else 0.0 for x, h in zip(values, hi)], np.float64)
    return hi, lo
