"""dvo_op_undistort (k_undistort) over the camera sweep of tests/undistort_sweep.py, bit for bit against the float64 camera model
(tests/real_data.py:undistort_index_np).  The gather copies the source pixel's bits unchanged -- INVALID, NaN with payloads and
either sign, -0.0, denormals and infinities included -- and the border is exactly INVALID (-2.0f)."""
import numpy as np
import pytest

import dvo_amd as dvo
from real_data import undistort_index_np
from undistort_sweep import CASES, IDS

pytestmark = pytest.mark.gpu

SPECIAL = np.array([0x7FC00000, 0x7FC12345, 0xFFC00001, 0x7F800001, 0x80000000, 0x00000001, 0x807FFFFF, 0x00400000,
                    0x7F800000, 0xFF800000, 0xC0000000], np.uint32).view(np.float32)   # NaNs, -0.0, denormals, +-inf, INVALID


def _source(w, h, seed):
    """a w x h float image whose pixels are all distinct where possible, with every special value sprinkled in"""
    rng = np.random.RandomState(seed)
    img = rng.uniform(-1, 2, (h, w)).astype(np.float32)
    n = w * h
    pick = rng.rand(n) < 0.1
    img.reshape(-1)[pick] = SPECIAL[rng.randint(len(SPECIAL), size=int(pick.sum()))]
    img.reshape(-1)[: min(n, len(SPECIAL))] = SPECIAL[: min(n, len(SPECIAL))]
    return img


def _expected(img, K, D):
    h, w = img.shape
    idx = undistort_index_np(K, D, w, h)
    exp = np.full((h, w), -2.0, np.float32)
    exp[idx >= 0] = img.reshape(-1)[idx[idx >= 0]]
    return exp


def test_sweep_has_ragged_launches():
    """sizes whose pixel count is not a multiple of the 256-thread block, and the extremes"""
    sizes = {(w, h) for _, _, _, w, h in CASES}
    assert sum((w * h) % 256 != 0 for w, h in sizes) >= 10
    assert (1, 1) in sizes and (1920, 1080) in sizes


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_undistort_op_equals_float64_model(case):
    name, K, D, w, h = case
    img = _source(w, h, seed=len(name) * 1000 + w + h)
    got = dvo.undistort(img, K, D)
    exp = _expected(img, K, D)
    bad = got.view(np.uint32) != exp.view(np.uint32)
    if bad.any():
        ys, xs = np.nonzero(bad)
        y, x = int(ys[0]), int(xs[0])
        raise AssertionError("%s: %d pixel(s) differ, first at (x=%d, y=%d): GPU 0x%08x, reference 0x%08x"
                             % (name, int(bad.sum()), x, y, got.view(np.uint32)[y, x], exp.view(np.uint32)[y, x]))
