"""Lockstep oracle replay of the mono pipeline (System::VisualOdometry::odometrize, system.hpp:44-74).

The GPU runs free; per sequence the oracle keeps its own FrameHistory and restates orc_vo_odometrize (oracle/dvo_oracle.c) one
frame at a time with the GPU's tracked pose injected:

  tracking  every Gauss-Newton iteration of the GPU's track log is re-run by orc.optimize at that iteration's input pose against
            the oracle's newest keyframe: contributing-pixel count equal, residual within rtol 1e-4, the logged update solves the
            oracle's normal equations (backward error <= TOL_BACKWARD), xi_after is the composition of input pose and update;
  pose      world xi = concatenate(ref.xi, rel) to rounding; the oracle frame then takes the GPU's rel and world xi, and the
            keyframe flag must be needNewFrame's (mapper.cpp:45-60);
  mapping   propagate (keyframe) or Mapper::update (otherwise), then regularize + re-decimation of the newest keyframe;
  state     the GPU's newest keyframe equals the oracle's bit for bit: gray / depth / sigma at every level, age, xi, id, the
            keyframe count and the valid-update count.

Since the oracle's state equals the GPU's after every frame, the comparison stays exact over any number of frames: the chaotic
dependence of stereo matches on 1e-5 pose differences never comes into play, because both sides map from the same
pose.  Test infrastructure only."""
import numpy as np

import nonfinite_cases
import orc
from util import TOL_BACKWARD, assert_composed, backward_error

LEVELS, CULLS = 3, 2          # the mono pyramid (System::VisualOdometry, D9)
TOP = LEVELS - 1
RESIDUAL_RTOL = 1e-4
MIN_TRANSLATION = np.float32(0.02)   # mapper.cpp:45-60


def raw_gray(rgb_u8):
    """What k_ingest makes of a raw u8 frame (1 or 3 channels): cv::cvtColor's fixed-point luma, times the raw gray scale."""
    from real_data import bgr2gray_u8
    return bgr2gray_u8(np.asarray(rgb_u8, np.uint8)).astype(np.float32) * np.float32(1.0 / 255.0)


def assert_maps_equal(got, exp, where):
    """Bit-for-bit equality of two float maps (NaN == NaN); on a mismatch names the first pixel and both values."""
    got = np.asarray(got, np.float32); exp = np.asarray(exp, np.float32)
    assert got.shape == exp.shape, "%s: shape %s (GPU) vs %s (oracle)" % (where, got.shape, exp.shape)
    bad = (got != exp) & ~(np.isnan(got) & np.isnan(exp))
    if bad.any():
        ys, xs = np.nonzero(bad)
        y, x = int(ys[0]), int(xs[0])
        raise AssertionError("%s: %d pixel(s) differ, first at (x=%d, y=%d): GPU %r, oracle %r (map %dx%d)"
                             % (where, int(bad.sum()), x, y, float(got[y, x]), float(exp[y, x]), got.shape[1], got.shape[0]))


class GpuFrame:
    """What the GPU reported for one sequence after one frame.  keyframe(level) -> dict(gray, depth, sigma[, age at the top level],
    xi, id) of the newest keyframe; rel: the handle's own record of the relative pose (dvo_vo only, else None)."""

    def __init__(self, key, xi_world, log, keyframe, n_keyframes, valid_updates, rel=None):
        self.key, self.xi_world, self.log, self.keyframe = bool(key), np.asarray(xi_world, np.float32), log, keyframe
        self.n_keyframes, self.valid_updates, self.rel = n_keyframes, valid_updates, rel


def vo_frame(vo, key, first):
    """GpuFrame of a dvo_vo handle (dvo_amd.VisualOdometry) after odometrize() (first: after its first frame, which is not tracked)."""
    n = vo.keyframeCount()
    if first:
        return GpuFrame(key, np.zeros(6, np.float32), None, lambda level: vo.keyframe(n - 1, level), n, 0)
    _, xi, rel = vo.lastFramePose()
    return GpuFrame(key, xi, vo.lastTrackLog(), lambda level: vo.keyframe(n - 1, level), n, vo.lastValidUpdates(), rel=rel)


def batch_frames(mb, first):
    """GpuFrame of every sequence of a MonoBatch after one odometrize call (first: after the first one, which tracks nothing)."""
    xi, _, key = mb.world_poses()
    out = []
    for q in range(mb.n_seq):
        top = mb.keyframe(q, TOP)
        cache = {TOP: top}

        def kf(level, q=q, cache=cache):
            if level not in cache:
                cache[level] = mb.keyframe(q, level)
            return cache[level]
        out.append(GpuFrame(key[q], xi[q], None if first else mb.last_track_log(q), kf, top["n_keyframes"], top["valid_updates"]))
    return out


class Replay:
    """One sequence's oracle FrameHistory, following the GPU.  step() once per frame, in order; counts the coverage."""

    def __init__(self, K, width, height, seed, init_depth, init_sigma, crop=True, name="seq"):
        self.K = np.asarray(K, np.float32).reshape(3, 3)
        self.w, self.h, self.seed, self.crop, self.name = width, height, int(seed), crop, name
        self.init = (np.asarray(init_depth, np.float32), np.asarray(init_sigma, np.float32))
        self.hist = []
        self.frame_id = -1
        self.n_key_translation = self.n_key_count = self.n_update = self.n_update_written = self.n_iterations = 0
        self.n_nonfinite = self.n_d13 = 0     # iterations whose oracle sums were not finite; of those, D13's (NaN against the oracle's zero)
        self.updated = np.zeros((height >> CULLS, width >> CULLS), bool)   # top-map pixels some Mapper::update changed

    def _where(self, what):
        return "%s frame %d: %s" % (self.name, self.frame_id, what)

    def step(self, gray, gpu):
        self.frame_id += 1
        obj = orc.OFrame(gray, None, None, self.K, LEVELS, CULLS, id=self.frame_id)
        if not self.hist:                       # first frame: the initial depth, identity pose, no regularize (system.hpp:47-55)
            obj.update_depth_sigma(*self.init)
            self.hist.append(obj)
            assert gpu.key, self._where("the first frame is a keyframe")
            self._compare(gpu, None)
            return
        ref = self.hist[-1]
        rel = self._track(obj, ref, gpu.log)
        if gpu.rel is not None:
            assert_maps_equal(np.reshape(gpu.rel, (1, 6)), rel.reshape(1, 6), self._where("lastFramePose rel vs the track log's xi"))
        assert_composed(ref.xi, rel, gpu.xi_world, tag=self._where("world xi = concatenate(ref.xi, rel)"))
        obj.set_pose(gpu.xi_world, rel)
        need = orc.need_new_frame(rel, self.frame_id, ref.c.id)
        assert gpu.key == need, self._where("keyframe flag %s, needNewFrame %s (|t| %.6g, frames since ref %d)"
                                            % (gpu.key, need, np.linalg.norm(rel[:3].astype(np.float64)), self.frame_id - ref.c.id))
        valid = None
        if need:                                # Mapper::estimate, mapper.cpp:16-33
            if np.sqrt(np.sum(rel[:3].astype(np.float64) ** 2)) > float(MIN_TRANSLATION):
                self.n_key_translation += 1
            else:
                self.n_key_count += 1
            d, s, a = orc.propagate(ref.depth(TOP), ref.sigma(TOP), ref.age(), rel, obj.K(TOP))
            obj.update_depth_sigma(d, s)
            obj.set_age(a)
            self.hist.append(obj)
        else:
            before = ref.depth(TOP)
            valid = orc.mapper_update(self.hist, obj, self.seed)
            self.n_update += 1
            self.n_update_written += int(valid > 0)
            self.updated |= ref.depth(TOP) != before
        kf = self.hist[-1]                      # mapper.cpp:139-144 (regularize, re-decimate the depth)
        kf.update_depth_sigma(orc.regularize(kf.depth(TOP), kf.sigma(TOP)), kf.sigma(TOP))
        self._compare(gpu, valid)

    def _track(self, obj, ref, log):
        """Every iteration of the GPU's log at the GPU's own input pose; returns the final twist (the relative pose)."""
        assert log is not None and len(log["n_iter"]) >= LEVELS, self._where("no track log")
        xi = np.zeros(6, np.float32)
        for l in range(LEVELS):
            n = int(log["n_iter"][l])
            assert n >= 1, self._where("level %d ran no iteration" % l)
            for it in range(n):
                where = self._where("level %d iteration %d" % (l, it))
                o = orc.optimize(obj.gray(l), ref.gray(l), ref.depth(l), ref.sigma(l), ref.K(l), xi, l, crop=self.crop)
                upd, after = log["xi_update"][l][it], log["xi_after"][l][it]
                assert o["n_valid"] == int(log["n_valid"][l][it]), (where, "n_valid GPU %d oracle %d" % (log["n_valid"][l][it], o["n_valid"]))
                if o["n_valid"] > 0 and not (np.isfinite(o["H"]).all() and np.isfinite(o["g"]).all() and np.isfinite(o["sum_r2"])):
                    # a NaN / inf pixel passed the gates ("Non-finite pixels"): no normal equations to solve.
                    # The residual is the oracle's within the usual tolerance where both are finite and of its class otherwise; the
                    # update is of the class tests/nonfinite_cases.py derives from the terms
                    res = np.float32(log["residual"][l][it])
                    if np.isfinite(res) and np.isfinite(o["residual"]):
                        np.testing.assert_allclose(res, o["residual"], rtol=RESIDUAL_RTOL, err_msg=where)
                    else:
                        assert (np.isnan(res) and np.isnan(o["residual"])) or res == o["residual"], (where, "residual class", res, o["residual"])
                    t = orc.optimize_terms(obj.gray(l), ref.gray(l), ref.depth(l), ref.sigma(l), ref.K(l), xi, l, crop=self.crop)
                    kind = nonfinite_cases.assert_update_class(upd, o, t, where)      # (all NaN where the oracle answers zero: D13)
                    self.n_nonfinite += 1
                    self.n_d13 += int(kind == "nan")
                elif o["n_valid"] > 0:
                    np.testing.assert_allclose(log["residual"][l][it], o["residual"], rtol=RESIDUAL_RTOL, err_msg=where)
                    back = backward_error(o["H"], o["g"], upd)
                    assert back <= TOL_BACKWARD, (where, "backward error %.3g" % back)
                else:                            # optimize.cpp:92-93
                    assert log["residual"][l][it] == -1.0 and not np.any(upd), (where, "no valid pixels", log["residual"][l][it], upd)
                nxt = orc.se3_concatenate(xi, upd)
                if np.all(np.isfinite(nxt)):
                    assert_composed(xi, upd, after, tag=where)
                else:                            # testXi (tracker.cpp:47-51): the pose is left unchanged
                    assert_maps_equal(np.reshape(after, (1, 6)), xi.reshape(1, 6), where + " (testXi)")
                xi = np.asarray(after, np.float32).copy()
                self.n_iterations += 1
        return xi

    def _compare(self, gpu, valid):
        kf = self.hist[-1]
        assert gpu.n_keyframes == len(self.hist), self._where("keyframe count GPU %d oracle %d" % (gpu.n_keyframes, len(self.hist)))
        for level in range(LEVELS):
            g = gpu.keyframe(level)
            for name in ("gray", "depth", "sigma"):
                assert_maps_equal(g[name], getattr(kf, name)(level), self._where("keyframe %s, level %d" % (name, level)))
            if level == TOP:
                assert_maps_equal(g["age"], kf.age(), self._where("keyframe age"))
                assert_maps_equal(np.reshape(g["xi"], (1, 6)), kf.xi.reshape(1, 6), self._where("keyframe xi"))
                assert g["id"] == kf.c.id, self._where("keyframe id GPU %d oracle %d" % (g["id"], kf.c.id))
        if valid is not None:
            assert gpu.valid_updates == valid, self._where("valid updates GPU %d oracle %d" % (gpu.valid_updates, valid))

    def coverage(self):
        return dict(key_translation=self.n_key_translation, key_count=self.n_key_count, updates=self.n_update,
                    updates_written=self.n_update_written, iterations=self.n_iterations,
                    nonfinite_iterations=self.n_nonfinite, d13_iterations=self.n_d13)


def total(replays):
    """coverage summed over replays"""
    out = {}
    for r in replays:
        for k, v in r.coverage().items():
            out[k] = out.get(k, 0) + v
    return out
