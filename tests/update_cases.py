"""Constructed inputs of Mapper::update for the branches k_depth_update adds to the oracle's algorithm (csrc/dvo_map_kernels.hip:
the float / double / sqrt cascade of the loop test, the sample reuse, the interior fast path, the workgroup's counting sort by the
head's step count, the two depthEstimate forms) and for the exits natural scenes do not reach (non-finite geometry, ages outside the
history, the 102-step cap, the image border).

Every case is a scene at MAP level (the operators take top-level maps; an orc.OFrame with one level and no culling holds the same
arrays): a textured plane seen by a keyframe at the identity and by a translated frame, with per-pixel prior depth, sigma and age
choosing the class.  The base geometry is dyadic -- K = [64 0 32; 0 64 24], the map-level K of a 256 x 192 frame with
K = [256 0 128; 0 256 96], translation 1/4 -- so a prior (depth, sigma) with power-of-two depth +- sigma gives segment ends and a
segment length that are exact in float: (1.5, 0.5) is a segment of exactly 8 px.

Each case has two forms.  'uniform': every pixel of the mapping window carries the class's prior (for the border classes: every
pixel of the border row), so every wave takes the kernel's wave-uniform branches the same way however the counting sort orders the
pixels.  'mixed': about one window pixel in eight carries it, the others ordinary priors of several search lengths, so waves are
mixed and the sort has buckets to separate.

case(name, form) -> dict; oracle_frames(c) -> (keyframes, obj) as orc.OFrame; run_oracle(c) -> the oracle's maps and the census;
NAMES: {name: (forms, classes)} with `classes` the census classes (orc.CENSUS) the case is built to reach.
"""
import numpy as np

import orc

W, H = 64, 48
K64 = np.array([[64, 0, 32], [0, 64, 24], [0, 0, 1]], np.float32)
K80 = np.array([[80, 0, 40], [0, 80, 30], [0, 0, 1]], np.float32)
K_SKEW = np.array([[64, 0.25, 32], [0, 64, 24], [0, 0, 1]], np.float32)      # depthEstimate's full-K form (k_sparse == 0)
K_ANISO = np.array([[72, 0, 30.5], [0, 56, 25.25], [0, 0, 1]], np.float32)
NAN, INF = np.float32(np.nan), np.float32(np.inf)
ULP_HALF = np.float32(2.0 ** -24)   # one ulp of 0.5
# ordinary priors (depth, sigma): segments of 3.6, 6.0, 8.5, 11.0 and 13.6 px at the base geometry, none of them near an integer
ORDINARY = ((2.0, 0.35), (1.4, 0.3), (1.5, 0.52), (1.7, 0.6), (1.6, 0.7))


def texture(x, y):
    """the plane's gray at map coordinates (any float arrays), in [0.05, 0.95]"""
    x = np.asarray(x, np.float64); y = np.asarray(y, np.float64)
    return (0.5 + 0.2 * np.sin(0.9 * x + 0.3 * y) + 0.15 * np.sin(0.37 * x - 0.8 * y + 1.0) + 0.1 * np.sin(0.21 * x + 1.7 * y)).astype(np.float32)


def class_mask(w, h, form):
    """the pixels that carry the class's prior"""
    yy, xx = np.mgrid[0:h, 0:w]
    if form == "uniform":
        return np.ones((h, w), bool)
    assert form == "mixed", form
    return (xx * 7 + yy * 13) % 8 == 0


def _scene(form, prior, w=W, h=H, K=K64, t=(0.25, 0.0, 0.0), z0=1.3, rel=None, n_old=0, old_xi=None, age=0.0, only=None, contrast=1.0):
    """The plane at depth z0 in front of the reference keyframe (identity pose), the tracked frame at twist t.  prior = (depth, sigma)
    of the class pixels (scalars or maps); n_old older keyframes (poses old_xi, the same gray) precede the reference; `age` of the
    class pixels; `only`: restricts the class pixels further (a boolean map); `contrast` scales the texture about 0.5."""
    t6 = np.zeros(6, np.float32); t6[:len(t)] = t
    yy, xx = np.mgrid[0:h, 0:w]
    cls = class_mask(w, h, form)
    if only is not None:
        cls &= only
    pick = (xx * 3 + yy * 5) % len(ORDINARY)
    depth = np.choose(pick, [np.float32(o[0]) for o in ORDINARY]).astype(np.float32)
    sigma = np.choose(pick, [np.float32(o[1]) for o in ORDINARY]).astype(np.float32)
    depth = np.where(cls, np.float32(prior[0]) if np.isscalar(prior[0]) else prior[0], depth).astype(np.float32)
    sigma = np.where(cls, np.float32(prior[1]) if np.isscalar(prior[1]) else prior[1], sigma).astype(np.float32)
    ages = np.where(cls, np.float32(age), np.float32(0)).astype(np.float32)
    gray = (0.5 + (texture(xx, yy) - 0.5) * np.float32(contrast)).astype(np.float32)
    # the frame sees the plane point of keyframe pixel p at p + f t / z0 (no rotation, t_z = 0)
    obj = (0.5 + (texture(xx - K[0, 0] * t6[0] / z0, yy - K[1, 1] * t6[1] / z0) - 0.5) * np.float32(contrast)).astype(np.float32)
    olds = [np.zeros(6, np.float32)] * n_old if old_xi is None else [np.asarray(o, np.float32) for o in old_xi]
    return dict(w=w, h=h, K=np.asarray(K, np.float32), kf_gray=[gray.copy() for _ in range(n_old + 1)],
                kf_xi=olds + [np.zeros(6, np.float32)], obj_gray=obj, obj_xi=t6.copy(), obj_rel=t6.copy() if rel is None else np.asarray(rel, np.float32),
                obj_id=4, depth=depth, sigma=sigma, age=ages, cls=cls, seed=7)


def _blobs(c):
    """INVALID blobs in every keyframe's gray, crossing the segments"""
    yy, xx = np.mgrid[0:c["h"], 0:c["w"]]
    blob = ((xx - 20) ** 2 + (yy - 20) ** 2 < 9) | ((xx - 41) ** 2 + (yy - 33) ** 2 < 16) | ((xx % 17 == 5) & (yy % 11 == 3))
    for g in c["kf_gray"]:
        g[blob] = orc.INVALID
    return c


def _long_mix(form):
    """segments of 99.5 .. 103 px and far beyond: both sides of (int)length + 2 = 103 and of count++ > 100"""
    yy, xx = np.mgrid[0:H, 0:W]
    lens = np.array([99.5, 100.0, 100.5, 101.0, 101.5, 102.0, 102.5, 103.0, 110.0, 126.0])[(xx + 3 * yy) % 10]
    dmax = 16.0 / (128.0 - lens)
    return _scene(form, (((dmax + 0.125) / 2).astype(np.float32), ((dmax - 0.125) / 2).astype(np.float32)))


def _first_at_origin(form):
    """The kernel reuses the previous step's centre sample as a step's first sample where pt - dir equals the previous centre, and a
    pixel's first step takes all three samples through the `first` term of need_n alone when its pt - dir is (0, 0), the initial
    value of the previous centre.  The keyframe lies 5 behind the frame and (1.5, 1.125) beside it, so that pixel (32, 24) with depth +
    sigma = 2 and pixel (16, 12) with depth + sigma = 4 start their segments at exactly (0, 0) and run along (0.8, 0.6) into the
    image.  A ramp of the gray along that line makes the first step the best match of pixel (32, 24): its result depends on the
    sample at (0, 0)."""
    c = _scene(form, (1.5, 0.5), t=(-1.5, -1.125, 5.0), rel=np.zeros(6, np.float32))
    c["depth"][24, 32] = 1.5; c["sigma"][24, 32] = 0.5
    c["depth"][12, 16] = 3.0; c["sigma"][12, 16] = 1.0
    yy, xx = np.mgrid[0:5, 0:5]
    for g in c["kf_gray"]:
        g[0:5, 0:5] = (0.6 + 0.2 * (0.8 * xx + 0.6 * yy)).astype(np.float32)
    c["obj_gray"][24, 32] = 0.8; c["obj_gray"][12, 16] = 0.8
    return c


def case(name, form):
    f = form
    far = np.array([0.5, 0, 0, 0, 0, 0], np.float32)
    if name == "exact_x":        # length 8 exactly, along x: the last loop test has q^2 == L^2
        return _scene(f, (1.5, 0.5))
    if name == "exact_y":
        return _scene(f, (1.5, 0.5), t=(0.0, 0.25, 0.0))
    if name == "exact_diag":     # the 3-4-5 triangle: segment (6, 8), length 10 exactly, a direction that is no float
        return _scene(f, (1.5, 0.5), t=(0.1875, 0.25, 0.0))
    if name == "dband_go_diag":  # a direction next to 3-4-5 (twist bits 0x3d997fff, 0x3dccdffe), length about 4 px: after four steps the
        # accumulated q^2 lies below L^2 by less than a relative 1e-12, the literal sqrt decides and says go -- a fifth step.  The plane
        # lies where that fifth step matches (depth 0.85) and the texture is strong enough for sigmaEstimate to pass the gate there:
        # the results of some 400 pixels depend on that step
        tx, ty = np.array([0x3d997fff, 0x3dccdffe], np.uint32).view(np.float32)
        return _scene(f, (1.5, 0.5), t=(tx, ty, 0.0), z0=0.85, contrast=3.0)
    if name == "int_plus":       # dmin = 1 - 2^-21, dmax = 2 + 2^-21: 8 px plus a few float ulps -- a ninth step
        return _scene(f, (1.5, np.float32(0.5) + 8 * ULP_HALF))
    if name == "int_minus":      # 8 px minus a few float ulps
        return _scene(f, (1.5, np.float32(0.5) - 8 * ULP_HALF))
    if name == "zero_motion":    # the class pixels were born in a keyframe at the frame's own pose: length 0
        if f == "uniform":
            return _scene(f, (1.5, 0.5), t=(0.0, 0.0, 0.0))
        return _scene(f, (1.5, 0.5), n_old=1, old_xi=[[0.25, 0, 0, 0, 0, 0]], age=1.0)
    if name == "sigma_nan":
        return _scene(f, (1.5, NAN))
    if name == "sigma_inf":
        return _scene(f, (1.5, INF))
    if name == "depth_nan":
        return _scene(f, (NAN, 0.5))
    if name == "depth_pinf":
        return _scene(f, (INF, 0.5))
    if name == "depth_ninf":
        return _scene(f, (-INF, 0.5))
    if name == "depth_zero":
        return _scene(f, (0.0, 0.5))
    if name == "depth_negative":
        return _scene(f, (-1.5, 0.5))
    if name == "obj_twist_nan":  # (a property of the whole frame: one form)
        c = _scene(f, (1.5, 0.5))
        c["obj_xi"][4] = NAN; c["obj_rel"][4] = NAN
        return c
    if name == "obj_twist_inf":
        c = _scene(f, (1.5, 0.5))
        c["obj_xi"][0] = INF; c["obj_rel"][0] = INF
        return c
    if name == "kf_twist_nan":   # a non-finite entry in the OLDER keyframe's twist only; the class pixels were born there
        return _scene(f, (1.5, 0.5), n_old=1, old_xi=[[0.0, NAN, 0, 0, 0, 0]], age=1.0)
    if name == "cap":            # 112 px: the 102-step cap, head bucket 103
        return _scene(f, (np.float32(0.5625), np.float32(0.4375)))
    if name == "near_cap":
        return _long_mix(f)
    if name == "age_beyond":     # born before the oldest of the two keyframes
        return _scene(f, (1.5, 0.5), n_old=1, old_xi=[far], age=5.0)
    if name == "age_negative":
        return _scene(f, (1.5, 0.5), n_old=1, old_xi=[far], age=-1.0)
    if name == "age_old":        # (ordinary: born in the older of two keyframes, another baseline)
        return _scene(f, (1.5, 0.5), n_old=1, old_xi=[[-0.125, 0.0625, 0, 0, 0, 0]], age=1.0)
    if name == "nd_ge6":         # prior 12 +- 4: one step from the shift of depth 16 lands on the shift of depth 8
        return _scene(f, (12.0, 4.0), z0=8.0)
    if name == "border_bottom":  # a search along x that drifts from y + 0.5 to y + 1: in the last row the best match rounds to y = h
        only = np.zeros((H, W), bool); only[H - 1] = True
        c = _scene("uniform", (1.5, 0.5), t=(0.25, -0.015625, 0.0), rel=np.zeros(6, np.float32), only=only)
        if f == "mixed":
            c["depth"][H - 1, ::2] = 2.0; c["sigma"][H - 1, ::2] = 0.35
        return c
    if name == "border_top":     # the plane's point of row 12 lies at y = -0.3 of the keyframe: a best match outside the image
        only = np.zeros((H, W), bool); only[12] = True
        c = _scene("uniform", (1.5, 0.375), t=(0.25, 0.25, 0.0), rel=np.zeros(6, np.float32), only=only)
        if f == "mixed":
            c["depth"][12, ::2] = 2.0; c["sigma"][12, ::2] = 0.35
        return c
    if name == "k_sparse":       # the same scene under a sparse and a full K (depthEstimate's two forms)
        return _scene(f, (1.35, 0.3))
    if name == "k_skew":
        return _scene(f, (1.35, 0.3), K=K_SKEW)
    if name == "k_aniso":
        return _scene(f, (1.35, 0.3), K=K_ANISO)
    if name == "first_at_origin":
        return _first_at_origin(f)
    if name == "invalid_blobs":
        return _blobs(_scene(f, (1.5, 0.52), n_old=1, old_xi=[[-0.125, 0.0625, 0, 0, 0, 0]], age=1.0))
    if name == "clip_80x60":     # the mapping window (x in [16, 144], y in [12, 108]) clipped by the map's right and bottom edges at a
        # size of 4800 pixels, no multiple of the workgroup's 256; translation 0.2 at fx = 80: the same exact 8 px segment
        return _scene(f, (1.5, 0.5), w=80, h=60, K=K80, t=(0.2, 0.0, 0.0))
    raise KeyError(name)


BOTH = ("uniform", "mixed")
# name: (forms, the census classes the case must reach)
NAMES = {
    "exact_x": (BOTH, ("test_sqrt", "dband_stop", "step_not_inner")),
    "exact_y": (BOTH, ("test_sqrt", "dband_stop")),
    "exact_diag": (BOTH, ("fband_stop",)),
    "dband_go_diag": (BOTH, ("test_sqrt", "dband_go", "rejected")),
    "int_plus": (BOTH, ("test_double", "fband_go")),
    "int_minus": (BOTH, ("test_double", "fband_stop")),
    "zero_motion": (BOTH, ("length_not_pos",)),
    "sigma_nan": (BOTH, ("length_not_pos", "test_sqrt")),
    "sigma_inf": (BOTH, ("length_not_pos", "test_sqrt")),
    "depth_nan": (BOTH, ("warp_fails",)),
    "depth_pinf": (BOTH, ("warp_fails",)),
    "depth_ninf": (BOTH, ("warp_fails",)),
    "depth_zero": (BOTH, ("warp_fails",)),
    "depth_negative": (BOTH, ("head_103", "cap", "gate_nan")),
    # (a frame's twist belongs to the whole frame: no pixel beside it can be ordinary, so these two have the uniform form only)
    "obj_twist_nan": (("uniform",), ("warp_fails",)),
    "obj_twist_inf": (("uniform",), ("warp_fails",)),
    "kf_twist_nan": (BOTH, ("length_not_pos",)),
    "cap": (BOTH, ("cap", "head_103", "test_float")),
    "near_cap": (BOTH, ("cap", "head_103")),
    "age_beyond": (BOTH, ("age_beyond",)),
    "age_negative": (BOTH, ("age_negative",)),
    "age_old": (BOTH, ("accepted",)),
    "nd_ge6": (BOTH, ("gate_nd_ge6",)),
    "border_bottom": (BOTH, ("d5_clamp", "grad_invalid")),
    "border_top": (BOTH, ("best_outside", "need_n")),
    "k_sparse": (BOTH, ("accepted", "rejected")),
    "k_skew": (BOTH, ("accepted",)),
    "k_aniso": (BOTH, ("accepted",)),
    "invalid_blobs": (BOTH, ("ssd_reject", "grad_invalid")),
    "clip_80x60": (BOTH, ("test_sqrt",)),
    "first_at_origin": (BOTH, ("first_origin",)),
}
# classes that cannot count 32 pixels in any scene: {class: the count its cases must reach} (tests/test_update_cases_oracle.py says why)
FEW = {"first_origin": 2}
ALL = [(n, f) for n, (forms, _) in NAMES.items() for f in forms]


def oracle_frames(c, age=None):
    """the case as the oracle's frames: one level, no culling -- the top level IS the map"""
    kfs = [orc.OFrame(g, None, None, c["K"], 1, 0, id=i) for i, g in enumerate(c["kf_gray"])]
    for k, xi in zip(kfs, c["kf_xi"]):
        k.set_pose(xi, xi)
    ref = kfs[-1]
    ref.update_depth_sigma(c["depth"], c["sigma"])
    ref.set_age(c["age"] if age is None else age)
    obj = orc.OFrame(c["obj_gray"], None, None, c["K"], 1, 0, id=c["obj_id"])
    obj.set_pose(c["obj_xi"], c["obj_rel"])
    return kfs, obj


def run_oracle(c, age=None, census=True):
    """orc.mapper_update on the case: dict(depth, sigma, age, valid, [counts, steps, flags])"""
    kfs, obj = oracle_frames(c, age)
    ref = kfs[-1]
    if census:
        v, counts, steps, flags = orc.mapper_update_census(kfs, obj, c["seed"])
        extra = dict(counts=counts, steps=steps, flags=flags)
    else:
        v, extra = orc.mapper_update(kfs, obj, c["seed"]), {}
    return dict(depth=ref.depth(0), sigma=ref.sigma(0), age=ref.age(), valid=v, **extra)


_CACHE = {}


def reference(name, form):
    """(case, the oracle's result with the census), computed once and shared: treat both as read-only"""
    if (name, form) not in _CACHE:
        c = case(name, form)
        _CACHE[(name, form)] = (c, run_oracle(c))
    return _CACHE[(name, form)]


def bits(a):
    """float32 maps as their bit patterns, every NaN as one: equal bits <=> the same value, or NaN in the same place"""
    a = np.ascontiguousarray(a, np.float32)
    b = a.view(np.uint32).copy()
    b[np.isnan(a)] = 0x7fc00000
    return b


# ---------------------------------------------------------------- the natural-input sweep of tests/test_gpu_parity.py
# cameras of the sweep cases that do not use K640 scaled to the frame (keyed by the case's seed): a skew term (depthEstimate's full-K
# branch, k_sparse == 0) and a strongly anisotropic camera
SWEEP_K = {11: np.array([[525.0, 1.5, 319.5], [0, 525.0, 239.5], [0, 0, 1]], np.float32),
           12: np.array([[600.0, 0, 319.5], [0, 450.0, 239.5], [0, 0, 1]], np.float32)}
# (seed, w, h, gain, sig, young)
SWEEP = [(1, 640, 480, 20.0, 0.3, 0.5), (2, 640, 480, 20.0, 0.2, 0.9), (5, 640, 480, 40.0, 0.5, 0.0), (6, 640, 480, 30.0, 0.4, 0.3),
         (9, 648, 488, 25.0, 0.3, 0.5), (11, 640, 480, 20.0, 0.3, 0.5), (12, 640, 480, 25.0, 0.3, 0.5), (17, 320, 240, 30.0, 0.3, 0.5)]


def sweep_inputs(seed, w, h, gain, sig, young):
    """One case of test_mapper_update_sweep: three keyframes (oldest first, the last one the reference, its prior maps and ages set)
    and the tracked frame as orc.OFrame, and the prior maps (top_d, top_s, age) as given to the reference."""
    from dvo_amd import synth
    from util import K640
    K = np.array(K640, np.float32).copy()
    K[0] *= w / 640.0; K[1] *= h / 480.0
    K = SWEEP_K.get(seed, K)
    g, d, s, poses = synth.sequence(6, width=w, height_px=h, K=K, seed=30 + seed, sigma_value=0.5)
    g, d = g.numpy(), d.numpy()
    rng = np.random.RandomState(100 + seed)
    kfs = [orc.OFrame(g[i], d[i], np.full_like(d[i], 0.5), K, 3, 2, id=i) for i in (0, 1, 3)]
    obj = orc.OFrame(g[4], None, None, K, 3, 2, id=4)
    def twist(a, b):
        return orc.se3_log((np.linalg.inv(poses[b]) @ poses[a]).astype(np.float32)) * np.float32(gain)
    x1 = twist(0, 1); x3 = orc.se3_concatenate(x1, twist(1, 3)); rel = twist(3, 4)
    kfs[1].set_pose(x1, x1); kfs[2].set_pose(x3, twist(1, 3)); obj.set_pose(orc.se3_concatenate(x3, rel), rel)
    ref = kfs[2]
    top_d = (ref.depth(2) + rng.normal(0, 0.05, ref.depth(2).shape)).astype(np.float32)
    top_d[rng.uniform(size=top_d.shape) < 0.03] = 0.05                      # below every gate
    top_s = np.full_like(top_d, sig)
    u = rng.uniform(size=top_d.shape)
    age = np.where(u < young, 0.0, np.where(u < young + (1 - young) / 2, 1.0, 2.0)).astype(np.float32)
    ref.update_depth_sigma(top_d, top_s)
    ref.set_age(age)
    return kfs, obj, top_d, top_s, age
