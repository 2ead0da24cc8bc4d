"""The device's solve and SE(3) chain against the 60-digit reference of tests/golden/pose_algebra.npz, through dvo_op_pose_algebra
(k_pose_algebra: the functions of csrc/dvo_math.h that k_gn_solve, k_track_gn_fused, k_track_persist, k_track_level and the mapping
side's pose bookkeeping call, one case per thread, doubles in and out).  Bounds: tests/pose_algebra.py, derived in DESIGN.md §6.
One launch per op over a few thousand cases; the references were frozen with mpmath, which this run does not need."""
import shutil

import numpy as np
import pytest

import dvo_amd as dvo
import pose_algebra as pa

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def device():
    """(report, outputs per op) of one pass over the fixture"""
    return pa.check_all(dvo.pose_algebra)


def test_all_six_ops_stay_inside_the_bounds(device):
    rep, _ = device
    print("pose algebra on the device, largest error / bound per op:")
    for ln in rep.lines():
        print("  " + ln)
    assert not rep.bad, "%d violation(s):\n%s" % (len(rep.bad), "\n".join(rep.bad[:20]))
    assert set(rep.ratio) == {0, 1, 2, 3, 4, 5} and max(rep.ratio.values()) > 0.0


def test_update_is_concatenate_then_exp_bit_for_bit(device):
    """se3_update_pose == se3_concatenate_f followed by pose_from_xi(., -1), and se3_exp_pair_d == se3_exp_d(xi), se3_exp_d(-xi): the
    two claims of dvo_math.h, on every finite pair of the fixture (check_all compares them too; here they are asserted one by one)"""
    _, out = device
    n = len(pa.fixture()["pair_in"])
    o3 = out[3][:n]
    assert (o3[:, 0] == 1.0).all()
    xin = o3[:, 1:7]
    assert pa.bits_equal(xin, out[2])                                                      # xi' is op 2 of (xi, upd)
    assert (xin == xin.astype(np.float32)).all()                                           # float values
    assert pa.bits_equal(o3[:, 7:19], dvo.pose_algebra(0, xin))                            # Tc' is op 0 of xi'
    assert pa.bits_equal(o3[:, 19:31], dvo.pose_algebra(0, -xin).astype(np.float32).astype(np.float64))   # pose is float32(op 0 of -xi')


def test_refused_updates_leave_the_state_alone(device):
    _, out = device
    f = pa.fixture()
    rej = out[3][len(f["pair_in"]):]
    must = f["rej_must"] == 1
    assert (rej[must, 0] == 0.0).all()                     # a NaN anywhere in the update, an infinite rotation: refused
    x0 = f["rej_in"][:, :6]
    keep = rej[:, 0] == 0.0
    assert pa.bits_equal(rej[keep, 1:7], x0[keep])
    assert pa.bits_equal(rej[keep, 7:19], dvo.pose_algebra(0, x0[keep]))
    assert pa.bits_equal(rej[keep, 19:31], dvo.pose_algebra(0, -x0[keep]).astype(np.float32).astype(np.float64))
    assert not np.isnan(rej[~keep, 1:]).any()              # 1e30 is a finite twist: testXi refuses NaN, nothing else
    # a system with a NaN sum: x is not finite on either path of the solve, and the update it would be is refused
    x = out[4][f["solve_tag"] == 1, :6]
    assert len(x) == 2 and not np.isfinite(x).all(axis=1).any()
    o = dvo.pose_algebra(3, np.concatenate([np.tile(x0[0], (2, 1)), x], axis=1))
    assert (o[:, 0] == 0.0).all() and pa.bits_equal(o[:, 1:7], np.tile(x0[0], (2, 1)))


def test_old_entry_points_are_float32_of_the_new_ops(device):
    """dvo_op_se3_exp / _log / _concatenate (k_se3) on a sample of the fixture equal float32 of ops 0, 1, 2 bit for bit"""
    _, out = device
    f = pa.fixture()
    f32 = lambda a: np.asarray(a, np.float64).astype(np.float32)
    for i in range(0, len(f["exp_in"]), 97):
        xi = f["exp_in"][i]
        if not (xi == f32(xi)).all():
            xi = f32(xi).astype(np.float64)               # the old entry point takes floats: give op 0 the same values
            new = dvo.pose_algebra(0, xi)[0]
        else:
            new = out[0][i]
        T = dvo.se3.exp(f32(xi))
        assert np.array_equal(T[:3, :3].ravel(), f32(new[:9])) and np.array_equal(T[:3, 3], f32(new[9:])), i
    for i in range(0, len(f["log_in"]), 23):
        r = f["log_in"][i]
        if not (r == f32(r)).all():
            continue                                      # (the double-rounded rotations have no float form)
        T = np.eye(4, dtype=np.float32); T[:3, :3] = f32(r[:9]).reshape(3, 3); T[:3, 3] = f32(r[9:])
        assert np.array_equal(dvo.se3.log(T), f32(out[1][i])), i
    for i in range(0, len(f["pair_in"]), 7):
        r = f["pair_in"][i]
        assert np.array_equal(dvo.se3.concatenate(f32(r[:6]), f32(r[6:])), f32(out[2][i])), i


def test_pinv_flag_is_the_references_branch(device):
    _, out = device
    f = pa.fixture()
    ok = f["solve_tag"] == 0
    np.testing.assert_array_equal(out[4][ok, 6], f["solve_aux"][ok, 0])
    assert (out[4][ok, 6] == 1).any() and (out[4][ok, 6] == 0).any()


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ is not installed")
def test_report_device_against_host(device, tmp_path):
    """Host code (libm) and the device (sincos_dev, atan2_dev) may differ in the last bit; both are inside the bounds,
    which is the only pass condition.  Reported: how many float results differ, per op."""
    _, out = device
    host = pa.build_shim(tmp_path / "host")
    flav = pa.build_shim(tmp_path / "flavour", pa.device_flavour(pa.header_text()))
    n = len(pa.fixture()["pair_in"])
    for op, cols, rows in ((2, slice(0, 6), slice(None)), (3, slice(1, 7), slice(0, n)), (3, slice(19, 31), slice(0, n)), (4, slice(0, 6), slice(None))):
        d = out[op][rows, cols]
        for name, run in (("host (libm)", host), ("device flavour on the host", flav)):
            h = run(op, pa.inputs(op))[rows, cols]
            fin = np.isfinite(d) & np.isfinite(h)
            print("op %d columns %d-%d: %d of %d float results differ from the %s" % (op, cols.start, cols.stop - 1, int((d[fin] != h[fin]).sum()), int(fin.sum()), name))
    for op in (0, 1):
        d, h = out[op], flav(op, pa.inputs(op))
        print("op %d: %d of %d double results differ from the device flavour on the host" % (op, int((d != h).sum()), d.size))
