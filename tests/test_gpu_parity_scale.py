"""Parity at the bench's own scale: a 1024-sequence dvo_batch at sigma = 0.1 -- multi-workgroup
k_gn_solve, active-list compaction across 128 solve workgroups, ~77 k-workgroup k_track_gn grids -- against (1) the same
sequences tracked alone (bit-identical pose AND per-iteration log) and (2) the CPU oracle, iteration by iteration; plus the
rank-deficient branch of the device 6x6 solve (the stand-in for cv::solve(DECOMP_SVD), optimize.cpp:96-97)."""
import numpy as np
import pytest

import dvo_amd as dvo
import orc
from dvo_amd import synth
import gn_sums
from util import K640, TOL_BACKWARD, assert_composed, backward_error

pytestmark = pytest.mark.gpu


def _rel_err(xi, P_ref, P_obj):
    E = synth.se3_exp_np(np.asarray(xi, np.float64)) @ np.linalg.inv(np.linalg.inv(P_obj) @ P_ref)
    return float(np.linalg.norm(E[:3, 3]))


@pytest.mark.timeout(900)
def test_batch_1024_sequences_match_single_tracker_and_oracle():
    import torch
    B, NSEED, F = 1024, 256, 5
    dev = torch.device("cuda", 0)
    # sequence s of the batch = bench.py's sequence (s % 256) (trajectory seed 42 + b), frame pair (p, p + 1), p = s // 256
    trajs = [synth.trajectory(F, seed=42 + b) for b in range(NSEED)]
    gray = torch.empty((NSEED, F, 480, 640), dtype=torch.float32, device=dev)
    depth = torch.empty_like(gray)
    for b0 in range(0, NSEED, 16):
        Ts = np.stack([trajs[b][f] for b in range(b0, b0 + 16) for f in range(F)])
        g, d = synth.render_batch(Ts, K640, 640, 480, device=dev)
        gray[b0:b0 + 16] = g.reshape(16, F, 480, 640); depth[b0:b0 + 16] = d.reshape(16, F, 480, 640)
    seq_b = np.arange(B) % NSEED; seq_p = np.arange(B) // NSEED
    idx_b = torch.as_tensor(seq_b, device=dev); idx_p = torch.as_tensor(seq_p, device=dev)
    ref_g = gray[idx_b, idx_p].contiguous(); ref_d = depth[idx_b, idx_p].contiguous()
    obj_g = gray[idx_b, idx_p + 1].contiguous(); obj_d = depth[idx_b, idx_p + 1].contiguous()
    sig = torch.full_like(ref_g, 0.1)
    torch.cuda.synchronize()
    cfg = dvo.default_config(gn_pixels_per_thread=4)    # one tile size for batch and single: results must then be bit-identical
    bt = dvo.Batch(B, K640, 640, 480, 4, 1, cfg=cfg)
    bt.push_device(ref_g.data_ptr(), ref_d.data_ptr(), sig.data_ptr())
    bt.push_device(obj_g.data_ptr(), obj_d.data_ptr(), sig.data_ptr())
    xb = bt.last_poses()[0].copy()
    assert np.isfinite(xb).all()
    # the accuracy sample of bench.py = sequences 0..31: their error against the ground truth picks the worst ones
    err = np.array([_rel_err(xb[s], trajs[seq_b[s]][seq_p[s]], trajs[seq_b[s]][seq_p[s] + 1]) for s in range(B)])
    bench_sample = np.array([s for s in range(B) if seq_b[s] < 32])
    worst = bench_sample[np.argsort(-err[bench_sample])[:16]]
    rng = np.random.RandomState(0)
    others = rng.choice(np.setdiff1d(np.arange(B), worst), 48, replace=False)
    sample = np.concatenate([worst, others])          # 64 sequences: 16 worst of the bench sample + 48 random
    logs = {int(s): bt.last_track_log(int(s)) for s in sample}
    bt.close()

    host = {}
    for s in sample:
        s = int(s)
        host[s] = (ref_g[s].cpu().numpy(), ref_d[s].cpu().numpy(), obj_g[s].cpu().numpy())
    sg = np.full((480, 640), 0.1, np.float32)

    # (1) batch == single, bit for bit: pose and the whole per-iteration log
    iters = []
    for s in sample:
        s = int(s)
        rg, rd, og = host[s]
        x1, l1 = dvo.track(og, rg, rd, sg, K640, 4, 1, cfg=cfg)
        np.testing.assert_array_equal(xb[s], x1, err_msg="sequence %d" % s)
        lb = logs[s]
        assert list(lb["n_iter"][:4]) == list(l1["n_iter"][:4])
        for l in range(4):
            np.testing.assert_array_equal(lb["residual"][l], l1["residual"][l])
            np.testing.assert_array_equal(lb["n_valid"][l], l1["n_valid"][l])
            np.testing.assert_array_equal(lb["xi_after"][l], l1["xi_after"][l])
        iters.append(sum(lb["n_iter"][:4]))
    assert max(iters) >= 40 and len(set(iters)) >= 4   # long, differing iteration counts: the active lists were really exercised

    # (2) every iteration of 32 sequences (the 16 worst + 16 others) against the oracle, given the iteration's input pose
    n_checked = 0
    for s in list(sample[:32]):
        s = int(s)
        rg, rd, og = host[s]
        ref = orc.OFrame(rg, rd, sg, K640, 4, 1)
        obj = orc.OFrame(og, None, None, K640, 4, 1)
        lb = logs[s]
        xi = np.zeros(6, np.float32)
        for l in range(4):
            for it in range(lb["n_iter"][l]):
                o = orc.optimize(obj.gray(l), ref.gray(l), ref.depth(l), ref.sigma(l), ref.K(l), xi, l)
                assert o["n_valid"] == lb["n_valid"][l][it], (s, l, it)
                np.testing.assert_allclose(lb["residual"][l][it], o["residual"], rtol=1e-4)
                # the GPU's own update of this iteration against the oracle's normal equations at the same input pose, as a backward
                # error (conditioning independent: the over-relaxed iteration visits poses with a handful of contributing pixels),
                # then the composition of exactly that update
                if o["n_valid"] > 0:
                    back = backward_error(o["H"], o["g"], lb["xi_update"][l][it])
                    assert back <= TOL_BACKWARD, (s, l, it, back)
                else:
                    assert not lb["xi_update"][l][it].any()
                assert_composed(xi, lb["xi_update"][l][it], lb["xi_after"][l][it], tag=(s, l, it))
                xi = lb["xi_after"][l][it]      # follow the GPU's trajectory: parity of every step given its input
                n_checked += 1
    assert n_checked > 32 * 20


def _rank_deficient_case(kind):
    h, w = 48, 64
    K = np.array([[60, 0, 31.5], [0, 60, 23.5], [0, 0, 1]], np.float32)
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    if kind == "ramp":        # constant horizontal gradient: gy = 0 everywhere -> the column of J for v_y is exactly zero
        ref = np.float32(0.2) + np.float32(0.008) * x
        obj = np.float32(0.2) + np.float32(0.008) * (x + np.float32(0.5))
    else:                     # 1-D texture: still no vertical gradient, but a varying horizontal one
        ref = (np.float32(0.5) + np.float32(0.3) * np.sin(np.float32(0.31) * x)).astype(np.float32)
        obj = (np.float32(0.5) + np.float32(0.3) * np.sin(np.float32(0.31) * (x + np.float32(0.4)))).astype(np.float32)
    depth = np.full((h, w), 1.25, np.float32)
    # Rows next to the top / bottom border are gated out (depth 0): there Convert::gradiate's INVALID border value (-2) leaks into
    # the bilinear gradient sample with a ~1e-7 weight (a quirk of the reference, reproduced), which would make gy tiny but nonzero.
    depth[:2] = 0.0; depth[-2:] = 0.0
    sigma = np.full((h, w), 0.5, np.float32)
    return obj.astype(np.float32), ref.astype(np.float32), depth, sigma, K


@pytest.mark.parametrize("kind", ["ramp", "stripes"])
@gn_sums.must_be_used
def test_rank_deficient_solve_matches_min_norm_solution(kind):
    """No vertical image gradient => J's second column is exactly zero => H is singular: LDL^T hits a zero pivot and the device
    takes the eigen pseudo-inverse branch of solve6 (cut sqrt(lambda) <= 2 FLT_EPSILON sum, as cv::solve(DECOMP_SVD)).  The update
    must be the MINIMUM-NORM least-squares solution: compared with the oracle's normal-equation solve AND with its SVD least
    squares on the stacked N x 6 system (the reference's own formulation, optimize.cpp:96-97)."""
    obj, ref, depth, sigma, K = _rank_deficient_case(kind)
    xi = np.zeros(6, np.float32)
    cfg = dvo.default_config(crop_enable=0)
    r = dvo.optimize(obj, ref, depth, sigma, K, xi, 0, cfg=cfg, want_mask=True)
    o = orc.optimize(obj, ref, depth, sigma, K, xi, 0, crop=False, variant=0, want_mask=True)
    f = orc.optimize(obj, ref, depth, sigma, K, xi, 0, crop=False, variant=1)
    assert r["n_valid"] == o["n_valid"] > 1000
    np.testing.assert_array_equal(r["mask"], o["mask"])
    # every sum inside the reduction bound of its own terms (tests/gn_sums.py); the sums of the vanishing column: exactly zero
    t = orc.optimize_terms(obj, ref, depth, sigma, K, xi, 0, crop=False)
    assert not t["J"][:, 1].any()
    gn_sums.assert_gn_sums(r, t, gn_sums.depth_for_cfg(cfg), "rank deficient (%s)" % kind)
    H = orc.upper_to_full(r["H"])
    assert np.abs(H[1]).max() == 0.0 and np.abs(H[:, 1]).max() == 0.0       # exactly singular: the fast path cannot be taken
    assert np.linalg.matrix_rank(H) <= 5
    un = float(np.linalg.norm(o["xi_update"]))
    assert un > 1e-4 and np.isfinite(r["xi_update"]).all()
    assert r["xi_update"][1] == 0.0                                         # minimum norm: nothing along the null direction
    np.testing.assert_allclose(r["xi_update"], o["xi_update"], rtol=0, atol=2e-4 * un + 2e-7)
    np.testing.assert_allclose(r["xi_update"], f["xi_update"], rtol=0, atol=2e-3 * un + 2e-7)
    xn = np.linalg.pinv(H, rcond=1e-10) @ r["g"]                            # numpy's pseudo-inverse of the GPU's own H, g
    np.testing.assert_allclose(r["xi_update"], xn, rtol=0, atol=2e-4 * un + 2e-7)


@gn_sums.must_be_used
def test_solve_of_an_all_zero_system_is_zero():
    """A constant image has no gradient at all: H = 0, g = 0 -> zero update, residual = mean r^2 (optimize.cpp:92-98)."""
    h, w = 40, 56
    K = np.array([[50, 0, 27.5], [0, 50, 19.5], [0, 0, 1]], np.float32)
    ref = np.full((h, w), 0.4, np.float32); obj = np.full((h, w), 0.5, np.float32)
    depth = np.full((h, w), 1.0, np.float32); sigma = np.full((h, w), 0.5, np.float32)
    cfg = dvo.default_config(crop_enable=0)
    r = dvo.optimize(obj, ref, depth, sigma, K, np.zeros(6, np.float32), 0, cfg=cfg)
    o = orc.optimize(obj, ref, depth, sigma, K, np.zeros(6, np.float32), 0, crop=False)
    assert r["n_valid"] == o["n_valid"] > 0
    t = orc.optimize_terms(obj, ref, depth, sigma, K, np.zeros(6, np.float32), 0, crop=False)
    assert not t["J"].any() and t["r"].all()
    gn_sums.assert_gn_sums(r, t, gn_sums.depth_for_cfg(cfg), "all-zero system")     # H and g exactly zero, sum_r2 inside its bound
    assert not r["xi_update"].any() and not o["xi_update"].any()
    np.testing.assert_allclose(r["residual"], o["residual"], rtol=2e-5)


def test_zz_report_reduction_bound_ratios():
    """last in the file: under -s, the largest error / bound ratio of every assert_gn_sums call of this process"""
    gn_sums.report("test_gpu_parity_scale")
    assert all(r <= 1.0 for _, r in gn_sums.RATIOS)
