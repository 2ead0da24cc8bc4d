"""The split pyramid build of a sensor-depth batch's plain raw pushes (DVO_PYRAMID_SPLIT) on the GPU.

k_pyramid_raw4_coarse on the tracking stream + k_pyramid_raw4_rest on the side stream must leave, bit for bit, the maps the single
k_pyramid_raw4 launch leaves, and every wait that orders the side stream must be in place: the poses, and the maps read straight after
a push returns, are compared as uint32 between a batch created with DVO_PYRAMID_SPLIT=1 (forced on: the batches here are far below
the 1 024 sequences at which it is on by default) and one created with DVO_PYRAMID_SPLIT=0 (the single kernel everywhere)."""
import numpy as np
import pytest

import dvo_amd as dvo
from util import K640

pytestmark = pytest.mark.gpu

N_SEQ, LEVELS = 3, 4
# (raw width, raw height, culls): both give a 64 x 48 top level and 32 x 24, 16 x 12, 8 x 6 below it
GEOMETRIES = {"128x96_culls1": (128, 96, 1), "256x192_culls2": (256, 192, 2)}


def _K(w):
    k = np.array(K640, np.float32).reshape(3, 3).copy()
    k[:2] *= w / 640.0
    return k


def _frames(w, h, n, seed):
    """n raw frames of N_SEQ sequences: a smooth texture that drifts a pixel or two per frame over a slanted plane, with black pixels,
    blocks of missing depth (d == 0) and isolated missing pixels -- on kept and on dropped rows and columns alike."""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    gray = np.zeros((n, N_SEQ, h, w), np.uint8)
    depth = np.zeros((n, N_SEQ, h, w), np.uint16)
    for q in range(N_SEQ):
        ph = rng.uniform(0, 6.28, 4)
        for k in range(n):
            sx, sy = 1.3 * k * (q + 1), 0.7 * k
            t = (np.sin((xx + sx) * 24.0 / w + ph[0]) + np.sin((yy + sy) * 20.0 / h + ph[1]) + np.sin((xx + sx + yy + sy) * 9.0 / w + ph[2])
                 + np.sin((xx + sx - 2 * (yy + sy)) * 5.0 / w + ph[3]))
            g = np.clip(127.5 + 30.0 * t, 0, 255).astype(np.uint8)
            d = (7000 + 6.0 * xx + 4.0 * yy + 300 * q).astype(np.uint16)
            g[rng.rand(h, w) < 0.02] = 0                                   # black pixels
            d[rng.rand(h, w) < 0.03] = 0                                   # isolated holes
            for _ in range(4):                                             # blocks of missing depth
                by, bx = rng.randint(0, h - 16), rng.randint(0, w - 16)
                d[by:by + rng.randint(3, 16), bx:bx + rng.randint(3, 16)] = 0
            gray[k, q], depth[k, q] = g, d
    return gray, depth


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _maps(bt):
    """every level's gray and depth of every sequence, read through the accessor with nothing between it and the push"""
    return [[bt.frame(q, l) for l in range(LEVELS)] for q in range(N_SEQ)]


def _run(monkeypatch, split, geometry, order, feed, seed=5):
    """Pushes frames `order` (indices into the rendered set); per push: (maps of the pushed frame, (xi, T) or None,
    iterations per sequence and level or None)."""
    import torch
    w, h, culls = GEOMETRIES[geometry]
    gray, depth = _frames(w, h, max(order) + 1, seed)
    monkeypatch.setenv("DVO_PYRAMID_SPLIT", "1" if split else "0")
    bt = dvo.Batch(N_SEQ, _K(w), w, h, LEVELS, culls)
    out = []
    for k, f in enumerate(order):
        if feed == "host":
            bt.push_raw_host(gray[f], depth[f])
        else:
            tg, td = torch.from_numpy(gray[f]).cuda(), torch.from_numpy(depth[f].view(np.int16)).cuda()
            torch.cuda.synchronize()
            bt.push_raw_device(tg.data_ptr(), 1, td.data_ptr())
        maps = _maps(bt)                      # (first: the accessor must be ordered after the side stream by the push alone)
        out.append((maps, bt.last_poses() if k > 0 else None, [bt.last_track_log(q)["n_iter"][:LEVELS] for q in range(N_SEQ)] if k > 0 else None))
        if feed != "host":
            torch.cuda.synchronize()          # (the frame tensors go out of scope)
    bt.close()
    return out


def _assert_same(a, b):
    assert len(a) == len(b)
    for k, ((ma, pa, ia), (mb, pb, ib)) in enumerate(zip(a, b)):
        assert ia == ib, "push %d: iterations" % k
        for q in range(N_SEQ):
            for l in range(LEVELS):
                for name, xa, xb in (("gray", ma[q][l][0], mb[q][l][0]), ("depth", ma[q][l][1], mb[q][l][1])):
                    assert xa.shape == xb.shape
                    assert np.array_equal(_bits(xa), _bits(xb)), "push %d sequence %d level %d %s" % (k, q, l, name)
        assert (pa is None) == (pb is None)
        if pa is not None:
            assert np.array_equal(_bits(pa[0]), _bits(pb[0])), "push %d: twists" % k
            assert np.array_equal(_bits(pa[1]), _bits(pb[1])), "push %d: poses" % k


@pytest.mark.parametrize("feed", ["host", "device"])   # host: only the kept rows are staged (row shift 0); device: whole frames
@pytest.mark.parametrize("geometry", sorted(GEOMETRIES))
def test_split_build_matches_single_kernel(monkeypatch, geometry, feed):
    """every level of gray and depth of four frames and the poses of the three tracked ones"""
    order = [0, 1, 2, 3]
    one = _run(monkeypatch, False, geometry, order, feed)
    two = _run(monkeypatch, True, geometry, order, feed)
    _assert_same(one, two)
    # the frames do what the test needs: holes and black pixels reach the maps, and the tracker moves
    g_top, d_top = one[0][0][0][LEVELS - 1]
    assert (d_top == 0).any() and (d_top > 0).any() and not np.array_equal(g_top, one[1][0][0][LEVELS - 1][0])
    assert np.abs(one[1][1][0]).max() > 0


def test_split_build_after_a_step_that_stops_early(monkeypatch):
    """two identical frames in a row: every sequence leaves each level after its first iteration (the adaptive schedule stops
    queueing them); the step after it, on a different frame, must find complete reference maps and give the same poses"""
    order = [0, 0, 1, 2]
    one = _run(monkeypatch, False, "128x96_culls1", order, "device")
    two = _run(monkeypatch, True, "128x96_culls1", order, "device")
    _assert_same(one, two)
    cap = dvo.default_config().max_iterations
    assert all(n < cap for per_seq in one[1][2] for n in per_seq)   # (the identical pair: every level stopped before the iteration cap)
    assert np.abs(one[2][1][0]).max() > 10 * np.abs(one[1][1][0]).max()   # (and the pair after it moves)


def test_top_level_read_straight_after_push(monkeypatch):
    """the side stream writes the top-level gray and every depth level: what the accessor returns directly after the first push
    (nothing tracks: the push itself waits) and after a tracked one is the decimated input, converted as include/dvo.h says"""
    w, h, culls = GEOMETRIES["128x96_culls1"]
    gray, depth = _frames(w, h, 2, 5)
    out = _run(monkeypatch, True, "128x96_culls1", [0, 1], "device")
    for k in range(2):
        for q in range(N_SEQ):
            g_top, d_top = out[k][0][q][LEVELS - 1]
            d16 = depth[k, q, ::2, ::2]
            want_d = d16.astype(np.float32) * np.float32(1.0 / 5000.0)
            want_g = gray[k, q, ::2, ::2].astype(np.float32) * np.float32(1.0 / 255.0)
            assert np.array_equal(_bits(d_top), _bits(want_d))
            assert np.array_equal(_bits(g_top[d16 > 0]), _bits(want_g[d16 > 0])) and (g_top[d16 == 0] == -2.0).all()   # (INVALID)
            g_low, d_low = out[k][0][q][LEVELS - 2]
            assert np.array_equal(_bits(d_low), _bits(want_d[::2, ::2]))
            assert np.array_equal(_bits(g_low[d16[::2, ::2] > 0]), _bits(want_g[::2, ::2][d16[::2, ::2] > 0]))
