"""undistort_source (csrc/dvo_math.h) compiled for the host, index for index against the float64 camera model of
tests/real_data.py:undistort_index_np, over the camera sweep of tests/undistort_sweep.py.  No GPU: a small C++ shim includes the
header the kernels include and is built with the library's float flags (-ffp-contract=off).

The device runs the same function (k_undistort, k_undistort_map); tests/test_gpu_undistort_exact.py and the fused-ingest tests hold
it to the same reference there."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from real_data import undistort_index_np
from undistort_sweep import CASES, IDS, census

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "direct-visual-odometry_amd", "csrc")

SHIM = r"""
#include "dvo_math.h"
extern "C" void undistort_indices(const float* K, const float* D, int w, int h, long long* out)
{
    const dvo::Intr k = dvo::make_intr(K);
    for (int v = 0; v < h; ++v)
        for (int u = 0; u < w; ++u) {
            int si;
            out[(long long)v * w + u] = dvo::undistort_source(k, v, u, D[0], D[1], D[2], D[3], D[4], w, h, si) ? si : -1;
        }
}
"""


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ is not installed")
    d = tmp_path_factory.mktemp("undistort_shim")
    src, so = d / "shim.cpp", d / "libshim.so"
    src.write_text(SHIM)
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-shared", "-fPIC", "-I", CSRC, "-o", str(so), str(src)])
    L = C.CDLL(str(so))
    L.undistort_indices.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    L.undistort_indices.restype = None

    def run(K, D, w, h):
        K = np.ascontiguousarray(K, np.float32).reshape(9); D = np.ascontiguousarray(D, np.float32).reshape(5)
        out = np.empty((h, w), np.int64)
        L.undistort_indices(K.ctypes.data, D.ctypes.data, w, h, out.ctypes.data)
        return out
    return run


def _first_difference(got, exp):
    ys, xs = np.nonzero(got != exp)
    y, x = int(ys[0]), int(xs[0])
    return "%d pixel(s) differ, first at (x=%d, y=%d): header %d, reference %d" % (int((got != exp).sum()), x, y, got[y, x], exp[y, x])


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_header_equals_float64_model(shim, case):
    name, K, D, w, h = case
    got, exp = shim(K, D, w, h), undistort_index_np(K, D, w, h)
    assert (got == exp).all(), "%s: %s" % (name, _first_difference(got, exp))


# Floors on what the sweep reaches (measured: tie_x 799, tie_y 288, neg_half 8319, far_edge 10457, d4 154227, fold 184826).
# If a change to the cases drops a total below its floor, the sweep no longer tests that edge.
FLOORS = dict(tie_x=600, tie_y=200, neg_half=6000, far_edge=8000, d4=100000, fold=100000)


def test_sweep_reaches_the_edges():
    total = dict.fromkeys(FLOORS, 0)
    for _, K, D, w, h in CASES:
        for k, v in census(K, D, w, h).items():
            total[k] += v
    print("undistortion sweep: %d cameras, %s" % (len(CASES), total))
    for k, floor in FLOORS.items():
        assert total[k] >= floor, (k, total[k], floor)


def test_ties_round_half_to_even():
    """f = 1, c = 0, p2 = 1/8 at 40 x 30 puts 75 in-image pixels on an exact .5 (47 in x, 28 in y); half away from zero (roundf)
    would send 37 of them to another source pixel"""
    from undistort_sweep import D_of, K_of
    c = census(K_of(1, 1, 0, 0), D_of(p2=0.125), 40, 30)
    assert (c["tie_x"], c["tie_y"]) == (47, 28), c


def test_skew_is_ignored(shim):
    """make_intr reads fx, fy, cx, cy only: the header with a skew term K[0, 1] gives the indices of the camera without it
    """
    from undistort_sweep import D_TUM
    K = np.array([[517.3, 0, 318.6], [0, 516.5, 255.3], [0, 0, 1]], np.float32)
    Ks = K.copy(); Ks[0, 1] = 3.5
    np.testing.assert_array_equal(shim(Ks, D_TUM, 640, 480), undistort_index_np(K, D_TUM, 640, 480))
