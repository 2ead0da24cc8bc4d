"""bench.py's frame renderer (one HIP kernel compiled at run time) against dvo_amd.synth.render_batch (a chain of torch kernels):
the benchmark's inputs must be the frames the torch chain renders, bit for bit."""
import types

import numpy as np
import pytest

import bench
from dvo_amd import synth


def test_renderer_compiles_for_gfx950():
    code = bench.compile_renderer("gfx950")
    assert code[:4] == b"\x7fELF" and b"render_frames" in code


def _torch_frames(rank, B, F, W, H, K):
    """what bench.py rendered before the fused kernel: synth.render_batch, quantised with torch"""
    import torch
    Ts = np.stack([synth.trajectory(F, seed=42 + 1000 * rank + b)[f] for b in range(B) for f in range(F)])
    g, d = synth.render_batch(Ts, K, W, H, device="cuda", newton_iters=6)
    g = g.reshape(B, F, H, W).permute(1, 0, 2, 3).contiguous(); d = d.reshape(B, F, H, W).permute(1, 0, 2, 3).contiguous()
    g8 = torch.clamp(torch.round(g * 255.0), 0, 255).to(torch.uint8)
    d16 = torch.clamp(torch.round(d * 5000.0), 0, 65535).to(torch.int32).to(torch.int16)
    return g, d, g8, d16


@pytest.mark.gpu
@pytest.mark.parametrize("rank,B,F,W,H,K,chunk", [(0, 5, 3, 640, 480, synth.K_640, 2), (1, 2, 2, 1920, 1080, synth.K_1080, 512)])
def test_renderer_matches_torch_chain_bitwise(rank, B, F, W, H, K, chunk):
    import torch
    env = types.SimpleNamespace(dev=torch.device("cuda", 0), rank=rank)
    g, d, g8, d16 = _torch_frames(rank, B, F, W, H, K)
    gray8 = torch.empty((F, B, H, W), dtype=torch.uint8, device=env.dev)
    depth16 = torch.empty((F, B, H, W), dtype=torch.int16, device=env.dev)
    gt = bench.render_frames(env, B, F, W, H, K, gray8, depth16, n_gt=3, chunk=chunk)
    assert len(gt) == min(3, B) and all(np.array_equal(p, q) for p, q in zip(gt[0], synth.trajectory(F, seed=42 + 1000 * rank)))
    assert torch.equal(gray8, g8), int((gray8 != g8).sum())
    assert torch.equal(depth16, d16), int((depth16 != d16).sum())
    # float32 outputs (the mono workload's float input and its ground-truth initial depth of frame 0)
    grayf = torch.empty((F, B, H, W), dtype=torch.float32, device=env.dev)
    depthf = torch.empty((1, B, H, W), dtype=torch.float32, device=env.dev)
    bench.render_frames(env, B, F, W, H, K, grayf, depthf, chunk=chunk)
    assert torch.equal(grayf.view(torch.int32), g.view(torch.int32)), int((grayf != g).sum())
    assert torch.equal(depthf[0].view(torch.int32), d[0].view(torch.int32)), int((depthf[0] != d[0]).sum())
