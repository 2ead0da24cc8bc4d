"""CPU tests of dvo_op_depth_update_batch (include/dvo.h), the operator-level entry point of a mono batch's mapping update: it is
declared, exported, listed and bound, the header states the contract the GPU test (tests/test_gpu_depth_update_batch.py) builds its
reference from, the argument block has the layout the binding assumes, INTEGRATION.md has its row, and every bad argument is refused
with DVO_ERR_BAD_ARGUMENT before anything touches the GPU -- here, on a machine without one, a call that got as far as the device
would answer DVO_ERR_NO_DEVICE."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import dvo_amd as dvo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "dvo_op_depth_update_batch"


def _header():
    return open(os.path.join(ROOT, "include", "dvo.h")).read()


def test_declared_exported_and_listed():
    txt = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert re.search(r"\bint\s+dvo_op_depth_update_batch\s*\(\s*int\s+dev\s*,\s*const\s+dvo_config\s*\*\s*\w+\s*,\s*const\s+dvo_depth_update_batch_args\s*\*", txt)
    assert hasattr(dvo.lib(), NAME) and NAME in dvo.EXPORTS
    assert callable(dvo.op_depth_update_batch)
    assert NAME in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_the_header_states_the_contract():
    txt = " ".join(re.sub(r"\n\s*\*", " ", _header()).split())
    for phrase in ("k_age_table over each sequence's keyframe ring", "k_depth_update_cam with per_camera", "(w >> 2) x (h >> 2)",
                   "OLDEST FIRST", "ring slot (n_total - n_hist + i) % ring", "its maps come back as given",
                   "searched against the oldest retained keyframe and counted in clamped[q]", "a negative age (>= n_hist) leaves the pixel alone",
                   "returned before anything is queued"):
        assert phrase in txt, phrase


def test_struct_layout():
    A = dvo.DepthUpdateBatchArgs
    assert C.sizeof(A) == 96
    assert [getattr(A, f).offset for f in ("struct_size", "n_seq", "w", "h", "ring", "per_camera")] == list(range(0, 24, 4))
    assert [getattr(A, f).offset for f in ("K", "n_total", "kf_gray", "kf_xi", "obj_gray", "obj_xi", "obj_rel_xi", "need", "frame_id")] == list(range(24, 96, 8))


N, W, H, R = 2, 256, 192, 3
_MAP = np.zeros((N, H // 4, W // 4), np.float32)
_GOOD = dict(K=np.array([256, 0, 128, 0, 256, 96, 0, 0, 1], np.float32), n_total=np.array([1, 4], np.int32),
             kf_gray=np.zeros((N, R, H // 4, W // 4), np.float32), kf_xi=np.zeros((N, R, 6), np.float32), obj_gray=_MAP,
             obj_xi=np.zeros((N, 6), np.float32), obj_rel_xi=np.zeros((N, 6), np.float32), need=np.array([0, 1], np.int32),
             frame_id=np.array([3, 4], np.int32))


def _args(**kw):
    a = dvo.DepthUpdateBatchArgs()
    a.struct_size = C.sizeof(dvo.DepthUpdateBatchArgs)
    a.n_seq, a.w, a.h, a.ring, a.per_camera = N, W, H, R, 0
    for k, v in dict(_GOOD, **kw).items():
        setattr(a, k, v.ctypes.data if isinstance(v, np.ndarray) else v)
    return a


def _call(a, maps=(True, True, True)):
    d, s, g = (_MAP.copy() if m else None for m in maps)
    ptr = lambda x: x.ctypes.data_as(C.POINTER(C.c_float)) if x is not None else None
    return dvo.lib().dvo_op_depth_update_batch(0, None, C.byref(a) if a is not None else None, ptr(d), ptr(s), ptr(g), None, None)


_K2 = np.tile(_GOOD["K"], (N, 1))
BAD = {
    "struct_size": dict(struct_size=64),
    "n_seq": dict(n_seq=0),
    "w below 64": dict(w=60),
    "h below 64": dict(h=32),
    "ring 0": dict(ring=0),
    "ring 65": dict(ring=65),
    "K NULL": dict(K=None),
    "K not finite": dict(K=np.array([256, 0, 128, 0, np.nan, 96, 0, 0, 1], np.float32)),
    "fx 0": dict(K=np.array([0, 0, 128, 0, 256, 96, 0, 0, 1], np.float32)),
    "second camera fy negative": dict(per_camera=1, K=np.concatenate([_K2[0], _K2[1] * np.array([1, 1, 1, 1, -1, 1, 1, 1, 1], np.float32)])),
    "n_total NULL": dict(n_total=None),
    "n_total 0": dict(n_total=np.array([1, 0], np.int32)),
    "kf_gray NULL": dict(kf_gray=None),
    "kf_xi NULL": dict(kf_xi=None),
    "obj_gray NULL": dict(obj_gray=None),
    "obj_xi NULL": dict(obj_xi=None),
    "obj_rel_xi NULL": dict(obj_rel_xi=None),
    "need NULL": dict(need=None),
    "need 2": dict(need=np.array([0, 2], np.int32)),
    "frame_id NULL": dict(frame_id=None),
}


@pytest.mark.parametrize("case", sorted(BAD))
def test_bad_arguments_are_refused_before_the_device(case):
    assert _call(_args(**BAD[case])) == dvo.DVO_ERR_BAD_ARGUMENT, case
    assert dvo.lib().dvo_last_error()    # (says which)


def test_null_args_and_null_maps_are_refused():
    assert _call(None) == dvo.DVO_ERR_BAD_ARGUMENT
    for maps in ((False, True, True), (True, False, True), (True, True, False)):
        assert _call(_args(), maps) == dvo.DVO_ERR_BAD_ARGUMENT, maps


@pytest.mark.skipif(dvo.device_count() > 0, reason="only meaningful on a box without a GPU")
def test_good_arguments_reach_the_device_and_fail_loudly_without_one():
    for kw in (dict(), dict(per_camera=1, K=_K2)):
        st = _call(_args(**kw))
        assert st not in (dvo.DVO_OK, dvo.DVO_ERR_BAD_ARGUMENT), kw.keys()
