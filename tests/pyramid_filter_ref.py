"""A numpy replica of the binomial-filtered gray pyramid of a sensor-depth batch (dvo_batch_set_pyramid_filter,
dvo_op_pyramid_frames_filtered), written from the contract text of include/dvo.h and not from the kernels.

One halving H: the centre tap decides validity; the nine taps are visited rows outside, columns inside; an invalid or outside tap
is skipped; S = fmaf((float)k, g, S), correctly rounded (fmaf_k), W += k, one float32 division.  The
top-level gray is H applied `culls` times to the converted source gray, the gray of level l - 1 is H of level l; depth, sigma and
wgt are the plain build's (tests/pyramid_ref.py).  Everything is exact, so the device is held to it bit for bit.

filtered_track is one tracking call on these maps: orc.optimize per level inside the tracking loop of tests/term_replay.py
(orc.se3_concatenate and the stop tests of tracker.cpp:68-73).  The outcome scene of DESIGN.md §39 lives here too, so that the CPU test recomputes the numbers the GPU test is
held to.  Test infrastructure only."""
import numpy as np

import pyramid_ref as pref

F32 = np.float32
INVALID = pref.INVALID
NONE, BINOMIAL3 = 0, 1
TAPS = [(j, i, (2 - abs(i)) * (2 - abs(j))) for j in (-1, 0, 1) for i in (-1, 0, 1)]   # the contract's order


def valid(a):
    a = np.asarray(a, F32)
    with np.errstate(invalid="ignore"):
        return ~np.isnan(a) & (a > INVALID)


def _taps(G):
    """(tap values [9][n][ho][wo], kept [9] bool) of every output pixel, outside taps not kept"""
    n, h, w = G.shape
    ho, wo = h >> 1, w >> 1
    P = np.full((n, h + 2, w + 2), INVALID, F32)
    P[:, 1:h + 1, 1:w + 1] = G
    ok = valid(P)
    vals, kept = [], []
    for j, i, _ in TAPS:
        sl = (slice(None), slice(1 + j, 1 + j + 2 * ho, 2), slice(1 + i, 1 + i + 2 * wo, 2))
        vals.append(P[sl]); kept.append(ok[sl])
    return vals, kept


def fmaf_k(k, g, S):
    """fmaf((float)k, g, S) for k = 1, 2 or 4: k * g is exact in float32, so the fused operation is one float32 addition.  Finite
    |g| >= 2^125, where k * g alone could overflow, is outside what this replica states (no test feeds it)."""
    assert k in (1, 2, 4)
    with np.errstate(all="ignore"):
        assert not (np.isfinite(g) & (np.abs(g) >= F32(2.0) ** 125)).any(), "gray beyond 2^125"
        return (F32(k) * g + S).astype(F32)


def halve(G):
    """H of maps [n][h][w] -> [n][h >> 1][w >> 1], float32, as the contract states it"""
    G = np.asarray(G, F32)
    vals, kept = _taps(G)
    S = np.zeros(vals[0].shape, F32)
    W = np.zeros(vals[0].shape, np.int32)
    for (_, _, k), v, ok in zip(TAPS, vals, kept):
        S = np.where(ok, fmaf_k(k, np.where(ok, v, F32(0)), S), S).astype(F32)
        W = W + k * ok
    with np.errstate(all="ignore"):
        q = (S / np.maximum(W, 1).astype(F32)).astype(F32)
    return np.where(kept[4], q, INVALID).astype(F32)   # (tap 4 is the centre)


def halve_exact(G):
    """the same halving as a float64 convolution with renormalisation, rounded once: equals halve() bit for bit where every partial
    sum is exact in float32 (dyadic input: multiples of 2^-8 in [0, 1])"""
    vals, kept = _taps(np.asarray(G, F32))
    S = np.zeros(vals[0].shape, np.float64)
    W = np.zeros(vals[0].shape, np.float64)
    for (_, _, k), v, ok in zip(TAPS, vals, kept):
        S += np.where(ok, k * np.where(ok, v, 0).astype(np.float64), 0.0)
        W += k * ok
    # (S is an integer multiple of 2^-8 below 2^13 and W <= 16: the float64 quotient is nowhere near a float32 midpoint it is not on,
    # so rounding it to float32 is the correctly rounded float32 quotient)
    q = (S / np.maximum(W, 1)).astype(F32)
    return np.where(kept[4], q, INVALID).astype(F32)


def filtered_gray(G0, levels, culls, halving=halve):
    """the gray pyramid [levels] of source gray [n][h][w], coarsest first"""
    top = np.asarray(G0, F32)
    for _ in range(culls):
        top = halving(top)
    out = [None] * levels
    out[levels - 1] = top.copy()
    for l in range(levels - 2, -1, -1):
        out[l] = halving(out[l + 1])
    return out


def build(w, h, levels, culls, gray, depth=None, sigma=None, cfg=None, halving=halve):
    """float maps [n][h][w] -> the filtered build: pyramid_ref.build with the gray pyramid replaced"""
    out = pref.build(w, h, levels, culls, gray, depth, sigma, False, cfg)
    out["gray"] = filtered_gray(gray, levels, culls, halving)
    for l in range(levels):
        assert out["gray"][l].shape[1:] == pref.level_shape(w, h, levels, culls, l)
    return out


def build_raw(w, h, levels, culls, rgb, depth16=None, depth_scale=0.0, cfg=None):
    g, d, s = pref.convert(rgb, depth16, depth_scale)
    return build(w, h, levels, culls, g, d, s, cfg)


def planned(ref, new, actions, levels):
    """the set a planned filtered build leaves: pyramid_ref.planned, with the gray of a SKIP sequence copied from `ref` level by level"""
    out = pref.planned(ref, new, actions, levels)
    for q, act in enumerate(actions):
        if act == pref.SEQ_SKIP:
            for l in range(levels):
                out["gray"][l][q] = ref["gray"][l][q]
    return out


class Frame:
    """What orc.OFrame is to the plain pyramid: depth, sigma and K of the oracle's frame, gray from the replica"""

    def __init__(self, gray, depth, sigma, K, levels, culls, filtered=True):
        import orc
        self.o = orc.OFrame(gray, depth, sigma, K, levels, culls)
        self.levels = levels
        self.g = [m[0] for m in filtered_gray(np.asarray(gray, F32)[None], levels, culls)] if filtered else [self.o.gray(l) for l in range(levels)]

    def gray(self, l):
        return self.g[l]

    def depth(self, l):
        return self.o.depth(l)

    def sigma(self, l):
        return self.o.sigma(l)

    def K(self, l):
        return self.o.K(l)


def filtered_track(obj, ref, levels, max_iterations, min_update, min_residual=0.0, crop=False):
    """One tracking call on two Frames: orc.optimize per level at the running pose, orc.se3_concatenate (a non-finite composition
    leaves the pose), stop on the update norm or the residual (tracker.cpp:68-73).  On plain frames it is orc.track.  (xi, log)."""
    import orc
    import term_replay

    def evaluate(l, xi):
        o = orc.optimize(obj.gray(l), ref.gray(l), ref.depth(l), ref.sigma(l), ref.K(l), xi, l, crop=crop)
        return o["xi_update"], o["residual"], dict(n_valid=o["n_valid"])
    return term_replay.track(levels, max_iterations, min_update, min_residual, evaluate)


# ---- the outcome scene of DESIGN.md §39: camera noise on the gray of synth's pairs ---------------------------------------------------
OUTCOME = dict(width=320, height=240, levels=3, culls=1, gray_sigma=0.04, sigma_t=0.005, sigma_r_deg=0.3, seeds=tuple(range(42, 50)),
               steps=(1.0, 0.75, 0.5), min_residual=0.0, min_update=2e-5, max_iterations=15, sigma_value=0.5, crop=True)


def outcome_pair(seed):
    """(gray [2][h][w], depth, sigma, K, the true twist of frame 1 against frame 0) of one seed: synth's pair with Gaussian gray noise
    from RandomState(2000 + seed)"""
    import orc
    from dvo_amd import synth
    o = OUTCOME
    K = synth.K_640.copy(); K[:2] *= 0.5
    g, d, s, poses = synth.sequence(2, o["width"], o["height"], K, seed, sigma_value=o["sigma_value"], sigma_t=o["sigma_t"], sigma_r_deg=o["sigma_r_deg"])
    g = g.numpy().astype(np.float64) + np.random.RandomState(2000 + seed).normal(0.0, o["gray_sigma"], tuple(g.shape))
    truth = orc.se3_log(np.linalg.inv(poses[1]) @ poses[0])
    return g.astype(F32), d.numpy().astype(F32), s.numpy().astype(F32), K, truth


def pose_error(xi, truth):
    return float(np.sqrt(np.sum((np.asarray(xi, np.float64) - np.asarray(truth, np.float64)) ** 2)))


def outcome_replica():
    """(error plain [8], error filtered [8]) of filtered_track on the outcome scene; the caller has set the oracle's step literals"""
    o = OUTCOME
    err = {False: [], True: []}
    for seed in o["seeds"]:
        g, d, s, K, truth = outcome_pair(seed)
        for filt in (False, True):
            ref = Frame(g[0], d[0], s[0], K, o["levels"], o["culls"], filt)
            obj = Frame(g[1], d[1], s[1], K, o["levels"], o["culls"], filt)
            xi, _ = filtered_track(obj, ref, o["levels"], o["max_iterations"], o["min_update"], o["min_residual"], crop=o["crop"])
            err[filt].append(pose_error(xi, truth))
    return np.array(err[False]), np.array(err[True])


# outcome_replica()'s figures (tests/test_pyramid_filter_abi.py recomputes them; DESIGN.md §39 has the table)
REPLICA_PLAIN = (0.0050685, 0.00069610, 0.0052994, 0.0019599, 0.0035868, 0.0065798, 0.0023276, 0.0038675)      # summed 0.029386
REPLICA_FILTERED = (0.00096513, 0.00086427, 0.0012365, 0.00014282, 0.0018474, 0.0036393, 0.0014476, 0.0026689)   # summed 0.012812
REPLICA_RATIO = 0.4360
