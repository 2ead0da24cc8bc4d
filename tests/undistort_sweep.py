"""The camera sweep of the lens-undistortion tests (tests/test_undistort_source_host.py on the CPU, tests/test_gpu_undistort_exact.py
through dvo_op_undistort): (name, K, D, w, h) cases that reach the edges of undistort_source (csrc/dvo_math.h), and the census
that proves they do.  Every case is checked index for index against tests/real_data.py:undistort_index_np."""
import numpy as np

from real_data import D_LOGICOOL, K_LOGICOOL, undistort_coords_np, undistort_index_np

D_TUM = np.array([0.2624, -0.9531, -0.0054, 0.0026, 1.1633], np.float32)   # TUM fr1 RGB camera
D_ZERO = np.zeros(5, np.float32)


def K_of(fx, fy, cx, cy):
    return np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], np.float32)


def D_of(**c):
    order = ("k1", "k2", "p1", "p2", "k3")
    return np.array([c.get(n, 0.0) for n in order], np.float32)


def _single_coefficients():
    """each coefficient alone at +-{1e-3, 0.3, 3}"""
    out = []
    for n in ("k1", "k2", "p1", "p2", "k3"):
        for m in (1e-3, 0.3, 3.0):
            for s in (1, -1):
                out.append(("%s=%g" % (n, s * m), D_of(**{n: s * m})))
    return out


def _cases():
    cases = []
    add = lambda name, K, D, w, h: cases.append((name, np.asarray(K, np.float32), np.asarray(D, np.float32), int(w), int(h)))

    # exact .5 ties: with f = 1, c = 0 and one tangential coefficient of 1/8 the coordinates are multiples of 1/8
    add("tie_p2_40x30", K_of(1, 1, 0, 0), D_of(p2=0.125), 40, 30)
    add("tie_p1_40x30", K_of(1, 1, 0, 0), D_of(p1=0.125), 40, 30)
    add("tie_p1p2_64x48", K_of(1, 1, 0, 0), D_of(p1=0.125, p2=-0.125), 64, 48)
    add("tie_k1_f2_33x17", K_of(2, 2, 0, 0), D_of(k1=0.5), 33, 17)
    add("tie_cx_half_9x7", K_of(1, 1, -0.5, 0.5), D_of(p2=0.125, p1=0.125), 9, 7)
    # the reference's cameras at their own and at other sizes
    add("logicool_640x480", K_LOGICOOL, D_LOGICOOL, 640, 480)
    add("logicool_q_160x120", K_of(195, 199, 94.5, 55), D_LOGICOOL, 160, 120)
    add("tum_640x480", K_of(517.3, 516.5, 318.6, 255.3), D_TUM, 640, 480)
    add("tum_646x486", K_of(517.3, 516.5, 318.6, 255.3), D_TUM, 646, 486)
    add("tum_1920x1080", K_of(1551.9, 1549.5, 955.8, 538.4), D_TUM, 1920, 1080)
    add("logicool_1920x1080", K_of(2340, 2388, 1134, 660), D_LOGICOOL, 1920, 1080)
    add("zero_1920x1080", K_of(1500, 1400, 959.5, 539.5), D_ZERO, 1920, 1080)
    # degenerate sizes
    add("1x1_zero", K_of(1, 1, 0, 0), D_ZERO, 1, 1)
    add("1x1_tum", K_of(2, 2, 0.5, 0.5), D_TUM, 1, 1)
    add("1x9_k1", K_of(1, 2, 0, 4), D_of(k1=-0.3), 1, 9)
    add("9x1_k1", K_of(2, 1, 4, 0), D_of(k1=0.3), 9, 1)
    add("2x2_p1", K_of(1, 1, 0.5, 0.5), D_of(p1=3.0), 2, 2)
    # folding: k1 = -2 bends the image back over itself
    add("fold_k1-2_96x64", K_of(40, 36, 47.5, 31.5), D_of(k1=-2.0), 96, 64)
    add("fold_k1-2_257x129", K_of(120, 110, 128, 64), D_of(k1=-2.0), 257, 129)
    # huge and non-finite coefficients (D4): the coordinates leave float range or are NaN
    add("huge_k1_1e6_50x40", K_of(10, 12, 25, 20), D_of(k1=1e6), 50, 40)
    add("huge_k3_1e30_50x40", K_of(2, 1, 25, 20), D_of(k3=1e30), 50, 40)
    add("huge_p1_1e30_31x23", K_of(1, 1, 15, 11), D_of(p1=-1e30), 31, 23)
    add("huge_all_1e6_37x29", K_of(5, 7, 18, 14), np.full(5, 1e6, np.float32), 37, 29)
    add("nan_k2_17x13", K_of(8, 8, 8, 6), D_of(k2=float("nan")), 17, 13)
    add("nan_p2_17x13", K_of(8, 8, 8, 6), D_of(p2=float("nan"), k1=0.1), 17, 13)
    add("inf_k1_17x13", K_of(8, 8, 8, 6), D_of(k1=float("inf")), 17, 13)

    # a seeded sweep: sizes up to 1920 x 1080; centred, off-centre and outside principal points; fx != fy; tiny focal lengths;
    # D = 0, D_LOGICOOL, TUM fr1 and each coefficient alone at +-{1e-3, 0.3, 3}
    rng = np.random.RandomState(20261016)
    sizes = [(1, 1), (3, 2), (7, 5), (16, 16), (33, 17), (40, 30), (64, 48), (127, 95), (160, 120), (257, 129), (320, 240),
             (511, 383), (640, 480), (646, 486), (1280, 720), (1920, 1080)]
    Ds = [("zero", D_ZERO), ("logicool", D_LOGICOOL), ("tum", D_TUM)] + _single_coefficients()
    for i, (dname, D) in enumerate(Ds):
        for j in range(2):
            w, h = sizes[rng.randint(len(sizes) - 2) if (i + j) % 9 else rng.randint(len(sizes))]
            pp = ("centred", "off", "outside")[(i + j) % 3]
            if pp == "centred":
                cx, cy = (w - 1) / 2.0, (h - 1) / 2.0
            elif pp == "off":
                cx, cy = rng.uniform(0, w), rng.uniform(0, h)
            else:
                cx, cy = w * rng.choice([-0.6, -0.1, 1.1, 1.7]), h * rng.uniform(-0.5, 1.5)
            fsel = (i * 2 + j) % 4
            if fsel == 0:
                fx, fy = (1.0, 1.0) if rng.rand() < 0.5 else (2.0, 1.0)
            elif fsel == 1:
                fx, fy = (2.0, 2.0) if rng.rand() < 0.5 else (1.0, 2.0)
            else:
                f = rng.uniform(0.5, 1.5) * max(w, h)
                fx, fy = f, f * rng.uniform(0.8, 1.25)
            add("sweep%02d_%s_%s_%dx%d" % (len(cases), dname, pp, w, h), K_of(fx, fy, cx, cy), D, w, h)
    return cases


CASES = _cases()
IDS = [c[0] for c in CASES]


def census(K, D, w, h):
    """The edges a case reaches, counted on the reference side: exact .5 ties of in-image pixels (x, y); coordinates in [-0.5, 0)
    that round to 0 and stay inside (x or y); coordinates in [w - 0.5, w + 0.5] (x) or [h - 0.5, h + 0.5] (y); D4 pixels (a
    coordinate not finite or |m| >= 2**30); folds (destinations whose source another destination also takes)."""
    mx, my = undistort_coords_np(K, D, w, h)
    idx = undistort_index_np(K, D, w, h)
    inside = idx >= 0
    with np.errstate(invalid="ignore"):
        fx, fy = mx - np.floor(mx), my - np.floor(my)
        d4 = ~(np.isfinite(mx) & np.isfinite(my) & (np.abs(mx) < 2 ** 30) & (np.abs(my) < 2 ** 30))
        c = dict(tie_x=int((inside & (fx == 0.5)).sum()), tie_y=int((inside & (fy == 0.5)).sum()),
                 neg_half=int((inside & (((mx >= -0.5) & (mx < 0)) | ((my >= -0.5) & (my < 0)))).sum()),
                 far_edge=int((((mx >= w - 0.5) & (mx <= w + 0.5)) | ((my >= h - 0.5) & (my <= h + 0.5))).sum()),
                 d4=int(d4.sum()))
    src = idx[inside]
    c["fold"] = int(src.size - np.unique(src).size)
    return c
