"""The fixed cases of the pose-algebra tests (dvo_op_pose_algebra) and their multi-precision references.

build() returns every array tests/golden/pose_algebra.npz holds: per op the inputs (float64 rows as the op takes them), the reference
as a (hi, lo) float64 pair and the per-case quantities the bounds of tests/pose_algebra.py read.  Nothing is drawn at test time: the
"random" axes are a seeded generator's first values.  Needs mpmath (tests/pose_ref.py); the tests read the frozen file."""
import numpy as np

PI = float(np.pi)
F32 = np.float32
T6F = F32(1e-6)


def _axes():
    r = np.random.RandomState(20260101).standard_normal((3, 3))
    ax = [np.array(a, np.float64) for a in ((1, 0, 0), (0, 1, 0), (0, 0, -1), (1, 1, 1))] + list(r)
    return [a / np.linalg.norm(a) if np.count_nonzero(a) > 1 else a for a in ax]


def thetas():
    t = [0.0, 1e-17, 1e-9, float(np.nextafter(T6F, F32(0))), float(T6F), float(np.nextafter(T6F, F32(1))), 2e-6, 1e-5, 1e-3, 0.1,
         PI / 4 * (1 - 1e-9), PI / 4 * (1 + 1e-9)]
    for k in (1, 2, 3, 4, 7, 100, 63661):
        for d in (0.0, 0.9e-5, -0.9e-5, 1.1e-5, -1.1e-5, 1e-3, -1e-3):
            t.append(k * (PI / 2) + d)
    for k in (1, 2, 3):      # the other end of the polynomial range in every quadrant: |r| just inside pi/4
        t += [k * (PI / 2) + PI / 4 * (1 - 1e-9), k * (PI / 2) - PI / 4 * (1 - 1e-9)]
    t += [PI - 1e-3, PI - 1e-5, PI - 1e-7, PI + 1e-4, 6.0, 2 * PI - 1e-4, 7.0, 20.0, 1e5 * (1 - 1e-6), 1e5 * (1 + 1e-6), 3e6]
    return t


T_SCALES = (0.0, 1e-3, 1.0, 30.0, 1e4)
T_DIR = np.array([0.6, -0.7, 0.39])


def exp_inputs():
    rows = []
    for th in thetas():
        for ia, ax in enumerate(_axes()):
            for sc in T_SCALES:
                if ia >= 4 and sc in (1e-3, 30.0):      # the random axes take three of the five translation scales
                    continue
                rows.append(np.concatenate([T_DIR * sc, ax * th]))   # (on a coordinate axis |omega| is theta exactly)
    return np.array(rows, np.float64)


def _dir6(i):
    d = np.random.RandomState(77 + i).standard_normal(6)
    d[:3] *= 0.7 / np.linalg.norm(d[:3])
    d[3:] *= 0.8 / np.linalg.norm(d[3:])
    return d


def pair_inputs():
    """(a, b) float32 twists of ops 2 and 3, as float64 rows of 12"""
    rows = []
    for i in range(3):
        da, db = _dir6(i), _dir6(10 + i)
        for na in (1e-7, 1e-4, 1e-2, 0.3, 1.5, 3.0):
            for nb in (0.0, 1e-7, 1e-4, 1e-2, 0.5):
                rows.append(np.concatenate([da * na, db * nb]))
            rows.append(np.concatenate([da * na, -(da * na).astype(F32).astype(np.float64)]))     # b = -a
        for pose in (1e-3, 1e-2, 0.1, 0.3):               # the tracker's sizes
            for upd in (1e-5, 1e-4, 1e-3, 1e-2):
                rows.append(np.concatenate([da * pose, db * upd]))
    z = np.zeros(3)
    for ax in _axes()[:5]:                                 # products just below pi and beyond it (the logarithm wraps)
        for tot in (PI - 1e-2, PI - 1e-3, PI + 1e-3, PI + 0.5, 2 * PI - 1e-2):
            rows.append(np.concatenate([T_DIR, ax * 2.0, 0.1 * T_DIR, ax * (tot - 2.0)]))
    rows.append(np.concatenate([z, [0, 0, 3.0], z, [0.2, 0, 0.1]]))
    return np.array(rows, np.float64).astype(F32).astype(np.float64)


def rejected_inputs():
    """op 3 only: updates with a NaN, an infinity or 1e30 in them, on a pose of the tracker's size"""
    xi = (_dir6(0) * 0.1).astype(F32).astype(np.float64)
    rows, must = [], []
    for slot, val, rej in ((0, np.nan, 1), (4, np.nan, 1), (5, np.inf, 1), (1, np.inf, 0), (2, 1e30, 0), (3, 1e30, 0)):
        upd = (_dir6(10) * 1e-3).astype(F32).astype(np.float64)
        upd[slot] = val
        rows.append(np.concatenate([xi, upd]))
        must.append(rej)
    allinf = np.full(6, np.inf)
    rows.append(np.concatenate([xi, allinf])); must.append(1)
    return np.array(rows, np.float64), np.array(must, np.int32)


def _sym21(A):
    A = 0.5 * (A + A.T)
    return np.array([A[i, j] for i in range(6) for j in range(i, 6)], np.float64)


def _Q(seed, n=6):
    q, _ = np.linalg.qr(np.random.RandomState(seed).standard_normal((n, n)))
    return q


def solve_inputs():
    """H[21] g[6] rows and a tag per row: 0 bounded, 1 a NaN sum (no bound)"""
    rows, tags = [], []
    x0 = np.array([0.3, -1.1, 0.7, 0.05, -0.4, 0.9])
    gen = np.array([1.0, -2.0, 0.5, 3.0, -1.0, 0.25])

    def add(H, g, tag=0):
        H21 = _sym21(np.asarray(H, np.float64))
        rows.append(np.concatenate([H21, np.asarray(g, np.float64)])); tags.append(tag)

    def full(H):
        H = np.asarray(H, np.float64)
        return 0.5 * (H + H.T)

    for ic, cond in enumerate((1e1, 1e3, 1e5, 1e7, 1e9, 1e11)):          # symmetric positive definite
        for scale in (1e-20, 1.0, 1e12):
            for seed in (1, 2):
                Q = _Q(100 * seed + ic)
                lam = scale * cond ** (-np.arange(6) / 5.0)
                H = full((Q * lam) @ Q.T)
                add(H, H @ x0)
                add(H, gen * scale)
    ints = np.random.RandomState(5).randint(-3, 4, size=(5, 6)).astype(np.float64)
    for rank in range(1, 6):                                             # J^T J from small integers: exactly singular in double
        J = ints[:rank]
        H = J.T @ J
        for zero in (None, rank % 6):
            Hz = H.copy()
            if zero is not None:
                Hz[zero, :] = 0; Hz[:, zero] = 0
            add(Hz, Hz @ x0)          # g in the range of H
            add(Hz, gen)              # and out of it
    for rho, m in ((1e-11, 1.0), (1e-13, 1.0)):                          # the last pivot at rho times the largest diagonal entry
        L = np.eye(6)
        L[5, :5] = 1.0
        L[3, 1] = 0.5; L[2, 0] = -0.25
        D = np.ones(6)
        H0 = (L * D) @ L.T
        D[5] = rho * H0.diagonal().max()
        H = (L * D) @ L.T
        add(H, H @ x0)
        add(H, gen)
    # the last pivot at 1e-11 of the largest diagonal entry WITH the small eigenvalue below the pseudo-inverse's cut: the rule keeps this
    # system on the LDL^T path, which solves along the small eigenvector too; a rule at 1e-10 would hand it over and lose that part
    eps, q5 = 0.6e-13, np.sqrt(0.006)
    v = np.concatenate([np.full(5, np.sqrt((1 - q5 * q5) / 5)), [q5]])
    H = np.eye(6) - (1 - eps) * np.outer(v, v)
    add(H, H @ v)
    add(H, gen)
    for ratio in (1e-6, 1e-8):                                         # one sqrt(lambda) at ratio of the sum, beside an exact zero row
        Q5 = _Q(9, 5)
        big = int(np.abs(Q5[:, 4]).argmax())              # the small eigenvalue's vector mostly along the last pivot's row
        Q5[[big, 4]] = Q5[[4, big]]
        lam = np.ones(5); lam[4] = (ratio * 4.0) ** 2
        H = np.zeros((6, 6)); H[:5, :5] = full((Q5 * lam) @ Q5.T)
        g = np.zeros(6); g[:5] = H[:5, :5] @ x0[:5]
        add(H, g)
        add(H, gen)
    add(np.zeros((6, 6)), gen)                                           # H = 0
    add(-np.eye(6) - 0.1, gen)                                           # every diagonal entry negative
    Hn = full((_Q(3) * np.array([2.0, 1.0, 0.5, 0.25, 1.5, -1.0])) @ _Q(3).T)   # one negative eigenvalue
    add(Hn, gen)
    Hs = full((_Q(4) * np.array([2.0, 1.0, 0.5, 0.25, 1.5, 3.0])) @ _Q(4).T)
    gn = gen.copy(); gn[2] = np.nan
    add(Hs, gn, 1)                                                       # a NaN sum in g
    Hq = Hs.copy(); Hq[1, 3] = np.nan; Hq[3, 1] = np.nan
    add(Hq, gen, 1)                                                      # and one in H
    return np.array(rows, np.float64), np.array(tags, np.int32)


def log_inputs(exp_in, exp_hi):
    """R[9] t[3] rows: float-rounded exp results, double-rounded rotations at the arctangent's break points, the axes' exact turns"""
    import mpmath as mp
    import pose_ref as pr
    rows = []
    for x, r in zip(exp_in, exp_hi):
        sc = np.abs(x[:3]).max()
        if sc in (0.0, 1.0, 1e4) and np.linalg.norm(x[3:]) < 25.0:
            rows.append(r.astype(F32).astype(np.float64))
    t = T_DIR * 2.0
    for ax in _axes()[:5]:
        angles = []
        for b in (0.4375, 0.6875, 1.1875, 2.4375):
            for e in (-1e-9, 1e-9):
                angles += [float(mp.atan(mp.mpf(b))) + e * b, PI - float(mp.atan(mp.mpf(b))) + e * b]
        if np.count_nonzero(ax) == 1:
            angles += [float(np.nextafter(T6F, F32(0))), float(T6F), float(np.nextafter(T6F, F32(1)))]
        for th in angles:
            R, _ = pr.exp(pr.vec(np.concatenate([np.zeros(3), ax * th])))
            rows.append(np.concatenate([[float(v) for v in R], t]))
    rows.append(np.concatenate([np.eye(3).ravel(), t]))
    for R in ([[0, -1, 0], [1, 0, 0], [0, 0, 1]], [[1, 0, 0], [0, 0, -1], [0, 1, 0]], [[0, 0, 1], [0, 1, 0], [-1, 0, 0]],     # quarter turns
              [[-1, 0, 0], [0, -1, 0], [0, 0, 1]], [[1, 0, 0], [0, -1, 0], [0, 0, -1]], [[-1, 0, 0], [0, 1, 0], [0, 0, -1]]):  # half turns
        for tt in (np.zeros(3), t):
            rows.append(np.concatenate([np.array(R, np.float64).ravel(), tt]))
    return np.array(rows, np.float64)


def reference(op, row):
    """(reference values as mpf list, aux float list) of one case; raises pose_ref.Undecided for an ambiguous branch"""
    import pose_ref as pr
    x = pr.vec(row)
    aux = {}
    if op == 0:
        R, t = pr.exp(x)
        return R + t, []
    if op == 1:
        xi = pr.log(x[:9], x[9:], aux)
        return xi, [float(aux["theta"]), float(aux["s"]), float(aux["wl"])]
    if op == 2:
        xi = pr.concatenate(x[:6], x[6:], aux)
        return xi, [float(aux[k]) for k in ("theta", "s", "wl", "tmax", "ta", "tb")]
    if op == 4:
        sol, pinv = pr.solve(x[:21], x[21:], aux)
        lam, kept = aux["lam"], aux["kept"]
        lmax = max(abs(l) for l in lam)
        kmin = min(kept) if kept else lmax
        return sol, [1.0 if pinv else 0.0, float(lmax), float(kmin), float(len(kept))] + [float(l) for l in lam]
    raise ValueError(op)


def build(log=print):
    import pose_ref as pr
    out = {}
    exp_in = exp_inputs()
    refs = [reference(0, r)[0] for r in exp_in]          # (all of them: the log inputs derive from these)
    hl = [pr.hi_lo(v) for v in refs]
    out["exp_in"] = exp_in
    out["exp_hi"] = np.array([h for h, _ in hl]); out["exp_lo"] = np.array([l for _, l in hl])
    cand = log_inputs(exp_in, out["exp_hi"])
    keep, hi, lo, aux, dropped = [], [], [], [], 0
    for i, r in enumerate(cand):
        try:
            v, a = reference(1, r)
        except pr.Undecided:
            dropped += 1        # a float-rounded matrix whose angle fell next to 1e-6f: such a case decides nothing, it is left out
            continue
        h, l = pr.hi_lo(v)
        keep.append(r); hi.append(h); lo.append(l); aux.append(a)
    log("log: %d cases, %d candidates left out as undecided" % (len(keep), dropped))
    out["log_in"] = np.array(keep); out["log_hi"] = np.array(hi); out["log_lo"] = np.array(lo); out["log_aux"] = np.array(aux)
    pin = pair_inputs()
    res = [reference(2, r) for r in pin]                 # (Undecided propagates: these cases are chosen, not derived)
    hl = [pr.hi_lo(v) for v, _ in res]
    out["pair_in"] = pin
    out["pair_hi"] = np.array([h for h, _ in hl]); out["pair_lo"] = np.array([l for _, l in hl])
    out["pair_aux"] = np.array([a for _, a in res])
    out["rej_in"], out["rej_must"] = rejected_inputs()
    sin, tags = solve_inputs()
    hi, lo, aux = [], [], []
    for r, tag in zip(sin, tags):
        if tag:
            hi.append(np.zeros(6)); lo.append(np.zeros(6)); aux.append(np.zeros(10))
            continue
        v, a = reference(4, r)
        h, l = pr.hi_lo(v)
        hi.append(h); lo.append(l); aux.append(a)
    out["solve_in"] = sin; out["solve_tag"] = tags
    out["solve_hi"] = np.array(hi); out["solve_lo"] = np.array(lo); out["solve_aux"] = np.array(aux)
    return out
