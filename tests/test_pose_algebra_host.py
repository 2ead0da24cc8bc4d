"""The serial double chain of every Gauss-Newton iteration -- solve6 / solve6_pinv, se3_exp_d, se3_log_d, se3_concatenate_f,
se3_update_pose, jacobi_eig6 (csrc/dvo_math.h) -- against a 60-digit reference, on the host.  No GPU.

tests/golden/pose_algebra.npz holds the cases of tests/pose_cases.py and their references (tests/pose_ref.py, mpmath); the bounds are
those of tests/pose_algebra.py, derived in DESIGN.md §6 by counting roundings.  Two builds of the header run here through a g++ shim
with the library's float flags: the header as the host code of libdvo includes it (libm's sin, cos, atan2), and its device flavour
-- sincos_dev, katan_d, atan2_dev, the polynomial kernels and reductions the GPU runs -- opened for the host compiler.
tests/test_gpu_pose_algebra.py holds the device itself to the same bounds through dvo_op_pose_algebra.

The last test changes one thing at a time in a copy of the header and shows that the bounds notice, and which of the suite's older
tolerances do not."""
import ctypes as C
import os
import re
import shutil

import numpy as np
import pytest

import dvo_amd as dvo
import pose_algebra as pa

ROOT = pa.ROOT
needs_gxx = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ is not installed")


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return pa.build_shim(tmp_path_factory.mktemp("pose_host"))


@pytest.fixture(scope="module")
def device_flavour(tmp_path_factory):
    return pa.build_shim(tmp_path_factory.mktemp("pose_devflavour"), pa.device_flavour(pa.header_text()))


# ---------------------------------------------------------------- the entry point
def test_entry_point_is_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "dvo.h")).read()
    assert re.search(r"int dvo_op_pose_algebra\(int dev, int op, int n, const double\* in, double\* out\);", hdr)
    assert "dvo_op_pose_algebra" in dvo.EXPORTS and hasattr(dvo.lib(), "dvo_op_pose_algebra")
    assert dvo.POSE_ALGEBRA_ROWS == pa.ROWS
    kh = open(os.path.join(pa.CSRC, "dvo_kernels.h")).read()
    for op, (ni, no) in pa.ROWS.items():          # the launcher's row table is the header's
        assert "case %d: n_in = %d; n_out = %d; return true;" % (op, ni, no) in kh


def test_entry_point_refuses_bad_arguments():
    L = dvo.lib()
    DP = C.POINTER(C.c_double)
    a = np.zeros(64, np.float64); o = np.zeros(64, np.float64)
    pa_, po = a.ctypes.data_as(DP), o.ctypes.data_as(DP)
    bad = dvo.DVO_ERR_BAD_ARGUMENT
    assert L.dvo_op_pose_algebra(0, 0, 1, None, po) == bad
    assert L.dvo_op_pose_algebra(0, 0, 1, pa_, None) == bad
    assert L.dvo_op_pose_algebra(0, 0, 0, pa_, po) == bad
    assert L.dvo_op_pose_algebra(0, 0, -3, pa_, po) == bad
    assert L.dvo_op_pose_algebra(0, 6, 1, pa_, po) == bad
    assert L.dvo_op_pose_algebra(0, -1, 1, pa_, po) == bad


@pytest.mark.skipif(dvo.device_count() > 0, reason="only meaningful on a box without a GPU")
def test_entry_point_fails_loudly_without_a_gpu():
    with pytest.raises(dvo.DvoError):
        dvo.pose_algebra(0, np.zeros((1, 6)))


# ---------------------------------------------------------------- the fixture
def test_fixture_is_what_the_modules_generate():
    """The inputs are what tests/pose_cases.py generates, and every 16th case's (hi, lo) reference, recomputed with mpmath from the
    file's input, equals the frozen one bit for bit.  (The inputs are compared to 1e-12: the generator goes through BLAS and LAPACK
    -- norms, a QR, matrix products -- whose last bit may depend on the processor; a case one bit away is the same case, and the
    reference is checked against the input the file holds.)"""
    pytest.importorskip("mpmath")
    import pose_cases
    import pose_ref as pr
    f = pa.fixture()

    def same(a, b):
        nf = ~np.isfinite(a)
        assert a.shape == b.shape and (nf == ~np.isfinite(b)).all() and ((a[nf] == b[nf]) | (np.isnan(a[nf]) & np.isnan(b[nf]))).all()
        fa, fb = np.where(np.isfinite(a), a, 0.0), np.where(np.isfinite(b), b, 0.0)
        assert (np.abs(fa - fb) <= 1e-12 * np.abs(fb) + 1e-15 * np.abs(fb).max(axis=1, keepdims=True)).all()

    same(pose_cases.exp_inputs(), f["exp_in"])
    same(pose_cases.pair_inputs(), f["pair_in"])
    rin, must = pose_cases.rejected_inputs()
    same(rin, f["rej_in"])
    assert (must == f["rej_must"]).all()
    sin, tags = pose_cases.solve_inputs()
    same(sin, f["solve_in"])          # (entries of H that are exact zeros or integers by construction are so on every machine)
    assert (tags == f["solve_tag"]).all()
    cand = pose_cases.log_inputs(f["exp_in"], f["exp_hi"])
    for r in f["log_in"]:
        assert (np.abs(cand - r) <= 1e-12 * (1 + np.abs(r))).all(axis=1).any()
    n = 0
    for op, key in ((0, "exp"), (1, "log"), (2, "pair"), (4, "solve")):
        for i in range(0, len(f[key + "_in"]), 16):
            if op == 4 and f["solve_tag"][i]:
                continue
            v, aux = pose_cases.reference(op, f[key + "_in"][i])     # (raises Undecided if a case's branch were ambiguous)
            hi, lo = pr.hi_lo(v)
            assert pa.bits_equal(hi, f[key + "_hi"][i]) and pa.bits_equal(lo, f[key + "_lo"][i]), (key, i)
            if aux:
                assert pa.bits_equal(np.array(aux), f[key + "_aux"][i]), (key, i)
            n += 1
    assert n > 150


def test_fixture_reaches_the_branches():
    """the cases the tolerances of old never reached are in the file: both sides of every switch of the header's SE(3) section"""
    f = pa.fixture()
    th = np.linalg.norm(f["exp_in"][:, 3:], axis=1)
    thf = th.astype(np.float32)
    assert (th == 0).any() and ((th > 0) & (th < 2.0 ** -52)).any() and ((th >= 2.0 ** -52) & (thf <= pa.T6F)).any()
    assert (thf == pa.T6F).any() and (thf == np.nextafter(pa.T6F, np.float32(1))).any() and (thf == np.nextafter(pa.T6F, np.float32(0))).any()
    assert ((th > np.pi / 4 * (1 - 1e-8)) & (th <= np.pi / 4)).any() and ((th > np.pi / 4) & (th < np.pi / 4 * (1 + 1e-8))).any()
    k = np.rint(th * (2 / np.pi)); r = np.abs(th - k * (np.pi / 2))
    fast = (th > np.pi / 4) & (th < 1e5)
    assert (fast & (r < 1e-5) & (r > 0.8e-5)).any() and (fast & (r >= 1e-5) & (r < 1.2e-5)).any()      # the |r| < 1e-5 fall-back, both sides
    for n in range(4):
        assert (fast & (r >= 1e-5) & (k.astype(np.int64) % 4 == n)).any()                             # every quadrant
    assert ((th >= 1e5) & (th < 1.1e5)).any() and ((th < 1e5) & (th > 0.9e5)).any() and (th > 1e6).any()
    assert {0.0, 1e-3 * 0.7, 0.7, 21.0, 7e3} <= set(np.abs(f["exp_in"][:, 1]).round(12))              # translation scales
    # the arctangent: every interval of katan_d and both sides of its break points, x > 0 and x < 0, x == 0, y == 0
    R = f["log_in"][:, :9]
    s = 0.5 * np.sqrt((R[:, 7] - R[:, 5]) ** 2 + (R[:, 2] - R[:, 6]) ** 2 + (R[:, 3] - R[:, 1]) ** 2)
    c = 0.5 * (R[:, 0] + R[:, 4] + R[:, 8] - 1)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = s / np.abs(c)
    for b in (0.4375, 0.6875, 1.1875, 2.4375):
        for sign in (1, -1):
            side = (np.sign(c) == sign) & (s > 0)
            assert (side & (q < b) & (q > b * (1 - 1e-8))).any() and (side & (q >= b) & (q < b * (1 + 1e-8))).any(), (b, sign)
    assert ((c == 0) & (s > 0)).any() and ((s == 0) & (c < 0)).any() and ((s == 0) & (c == 1)).any()
    assert ((c < 0) & (s > 0) & (s < 1e-4)).any()                                                     # x < 0 close to pi
    # the solve: both paths, the rule's two sides, the cut's two sides
    aux, ok = f["solve_aux"], f["solve_tag"] == 0
    assert (aux[ok, 0] == 0).any() and (aux[ok, 0] == 1).any() and (aux[ok, 3] == 0).any()
    assert ((aux[ok, 0] == 1) & (aux[ok, 3] < 6) & (aux[ok, 3] > 0)).any()
    with np.errstate(divide="ignore", invalid="ignore"):
        kappa = aux[ok, 1] / aux[ok, 2]
    assert (kappa[aux[ok, 3] == 6] > 1e12).any()


# ---------------------------------------------------------------- the header on the host, both flavours
def _assert_inside(rep, name):
    print("pose algebra, %s:" % name)
    for ln in rep.lines():
        print("  " + ln)
    assert not rep.bad, "%s: %d violation(s):\n%s" % (name, len(rep.bad), "\n".join(rep.bad[:20]))


@needs_gxx
def test_host_header_stays_inside_the_bounds(host):
    rep, _ = pa.check_all(host)
    _assert_inside(rep, "dvo_math.h as the host code includes it (libm)")


@needs_gxx
def test_device_flavour_stays_inside_the_bounds(device_flavour):
    rep, _ = pa.check_all(device_flavour)
    _assert_inside(rep, "dvo_math.h's device flavour (sincos_dev, atan2_dev) compiled for the host")


@needs_gxx
def test_device_flavour_differs_from_libm_only_in_last_bits(host, device_flavour):
    """the two flavours are different arithmetic (that is why both are measured); where both round to float they mostly agree"""
    for op, sl in ((2, slice(0, 6)), (4, slice(0, 6))):
        a, b = host(op, pa.inputs(op))[:, sl], device_flavour(op, pa.inputs(op))[:, sl]
        fin = np.isfinite(a) & np.isfinite(b)
        print("op %d: %d of %d float results differ between the libm and the polynomial flavour" % (op, int((a[fin] != b[fin]).sum()), int(fin.sum())))
    a, b = host(0, pa.inputs(0)), device_flavour(0, pa.inputs(0))
    assert (a != b).any()          # the device flavour did run its own sine and cosine


# ---------------------------------------------------------------- mutations
MUTATIONS = [
    # (name, old text, new text, occurrences, which older tolerance accepts it)
    ("the lo term of the pi/2 reduction dropped", "        r = fma(-k, 6.12323399573676603587e-17, r);\n", "", 1, "se3"),
    ("ksin_d's last coefficient altered in its 6th digit", "1.58969099521155010221e-10", "1.58960099521155010221e-10", 1, "se3"),
    ("Rm[1] taken from Rp[1] instead of Rp[3]", "Rm[1] = Rp[3]", "Rm[1] = Rp[1]", 1, "composed"),
    ("the pivot rule at 1e-10", "ok = ok && (dj > 1e-12 * maxd);", "ok = ok && (dj > 1e-10 * maxd);", 1, "backward"),
    ("the pseudo-inverse's cut at 20 FLT_EPSILON", "thr = 2.0 * 1.1920928955078125e-07 * sum", "thr = 20.0 * 1.1920928955078125e-07 * sum", 1, "backward"),
    ("B built from ith2 instead of ith2 * ith", "B = (th - s) * (ith2 * ith)", "B = (th - s) * (ith2)", 2, None),
]


def _old_se3_accepts(run, good):
    """tests/test_gpu_parity.py::test_se3_device_matches_oracle's sample and tolerances, with the unmutated header in the oracle's place
    (the oracle is the same formulas in double)"""
    rng = np.random.RandomState(0)
    f32 = lambda x: x.astype(np.float32).astype(np.float64)
    try:
        for scale in (1e-7, 1e-3, 0.05, 1.0):
            for _ in range(8):
                a = f32(rng.uniform(-1, 1, 6) * scale)
                b = f32(rng.uniform(-1, 1, 6) * scale * 0.3)
                T = f32(good(0, a))
                np.testing.assert_allclose(f32(run(0, a)), T, rtol=0, atol=1.2e-7)
                np.testing.assert_allclose(f32(run(1, T)), f32(good(1, T)), rtol=2e-6, atol=1e-9)
                ab = np.concatenate([a, b])
                np.testing.assert_allclose(run(2, ab), good(2, ab), rtol=2e-6, atol=1e-9)
    except AssertionError:
        return False
    return True


def _old_composed_accepts(run, good):
    """tests/util.py::assert_composed on the tracker-sized updates of the fixture: 4 ulp of max(1, |xi|) on xi' alone"""
    rows = pa.fixture()["pair_in"]
    got, ref = run(3, rows)[:, 1:7], good(2, rows)
    tol = 4 * np.spacing(np.maximum(1.0, np.abs(ref).max(axis=1)).astype(np.float32)).astype(np.float64)
    return bool((np.abs(got - ref) <= tol[:, None]).all())


def _old_backward_accepts(run, good):
    """tests/util.py::TOL_BACKWARD, the backward error of the update against the normal equations, on the well-conditioned systems of
    the fixture (what image-built sums are: condition up to 1e7, scale 1)"""
    f = pa.fixture()
    rows = f["solve_in"][(f["solve_tag"] == 0) & (f["solve_aux"][:, 3] == 6) & (f["solve_aux"][:, 1] / np.maximum(f["solve_aux"][:, 2], 1e-300) < 2e7)
                         & (f["solve_aux"][:, 1] > 0.5) & (f["solve_aux"][:, 1] < 2)]
    assert len(rows) >= 8
    x = run(4, rows)[:, :6]
    for r, xi in zip(rows, x):
        H = np.asarray(pa.full6(r[:21]), np.float64); g = r[21:]
        if np.abs(H @ xi - g).max() / max((np.abs(H) @ np.abs(xi) + np.abs(g)).max(), 1e-300) > 2e-6:
            return False
    return True


@needs_gxx
def test_every_mutation_is_rejected_by_the_bounds(tmp_path, device_flavour):
    """One substitution each in a copy of the header's device flavour (match counts asserted), run over the whole fixture.  Every one
    falls outside the bounds; the first five pass the tolerance that covered that code before (1.2e-7 / 2e-6 relative on 32 random
    twists, assert_composed's 4 float ulp of xi', TOL_BACKWARD on well-conditioned systems): only the gross one, B, does not."""
    base = pa.device_flavour(pa.header_text())
    old = dict(se3=_old_se3_accepts, composed=_old_composed_accepts, backward=_old_backward_accepts)
    accepted_before = 0
    for k, (name, a, b, count, tol) in enumerate(MUTATIONS):
        run = pa.build_shim(tmp_path / ("m%d" % k), pa.sub_exact(base, a, b, count))
        rep, _ = pa.check_all(run)
        worst = max(rep.ratio.values())
        passes_old = [t for t, fn in old.items() if fn(run, device_flavour)]
        print("%-52s %2d violation(s), largest error / bound %.3g; still accepted by: %s" % (name, len(rep.bad), worst, ", ".join(passes_old) or "none"))
        assert rep.bad, "not rejected: " + name
        if tol is not None:
            assert tol in passes_old, "%s: expected the old %s tolerance to accept it" % (name, tol)
            accepted_before += 1
        else:
            assert "se3" not in passes_old       # (the old test does see a wrong B)
    assert accepted_before >= 3
