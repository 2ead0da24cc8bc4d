"""What a missing photometric calibration costs.  synth's mono scene at 320x240 goes through a simulated camera
(photometric_ref.expose: a cos^4 vignette falling to 0.4 in the corners, then a gamma-2.2 response, rounded to u8) and is tracked
from the ground-truth initial depth with the converging configuration of §15's outcome test, once with set_photometric and once
without.  Compared: the maximum world translation error over the tracked frames.

The reference ratio comes from the CPU oracle (orc.OVO, same scene, configuration and initial depth, fed correct_np of the
simulated frames against their plain raw_gray): 0.01174 m corrected, 0.1411 m uncorrected, R = 0.0832 (the float render itself:
0.01524 m).  The GPU must reach right <= ((R + 1) / 2) * missing: §30's margin rule, half the oracle's gain left as room for the
differences between the oracle's tracker and the batch's."""
import functools

import numpy as np
import pytest

import dvo_amd as dvo
import orc
import photometric_ref as pr
from dvo_amd import synth

pytestmark = pytest.mark.gpu

W, H, N = 320, 240, 6
K = np.array([[262.5, 0, 159.75], [0, 262.5, 119.75], [0, 0, 1]], np.float32)   # K_640 / 2
ORACLE_R = 0.0832


def _converging_cfg():
    return dvo.default_config(rng_seed=3, gn_pixels_per_thread=4, step_default=1.0, step_level1=0.75, step_level2=0.5, min_residual=0.0)


@functools.lru_cache(maxsize=None)
def _scene():
    g, d, _, poses = synth.sequence(N, W, H, K, seed=7, sigma_value=0.5)
    g, d = g.numpy(), d.numpy()
    V = pr.cos4_vignette(W, H, 0.4)
    raw = np.stack([pr.expose(g[k], pr.gamma_forward(2.2), V) for k in range(N)])
    return raw, d, poses, V


def _trajectory_error(calibrated):
    import torch
    raw, d, poses, V = _scene()
    mb = dvo.MonoBatch(1, K, W, H, cfg=_converging_cfg())
    init = orc.cull_image(d[0], 2).astype(np.float32)       # ground-truth initial depth: mono scale anchored
    mb.setInitialDepth(init, np.full_like(init, 0.5))
    if calibrated:
        mb.set_photometric(pr.gamma_response(2.2), V)
    errs = []
    for k in range(N):
        t = torch.from_numpy(raw[k][None].copy()).cuda(); torch.cuda.synchronize()
        mb.odometrize_raw_device(t.data_ptr(), 1)
        _, T, _ = mb.world_poses()
        if k:
            gt = np.linalg.inv(poses[k]) @ poses[0]           # camera k <- camera 0
            E = T[0].astype(np.float64) @ np.linalg.inv(gt)
            errs.append(float(np.linalg.norm(E[:3, 3])) if np.isfinite(E).all() else np.inf)
    mb.close()
    return max(errs)


def test_a_missing_calibration_costs_accuracy():
    right, missing = _trajectory_error(True), _trajectory_error(False)
    print("gamma 2.2 + cos^4 vignette to 0.4: max world translation error with set_photometric %.4g m, without %.4g m (ratio %.3f; oracle %.3f)"
          % (right, missing, right / missing, ORACLE_R))
    assert right <= ((ORACLE_R + 1) / 2) * missing, (right, missing)
