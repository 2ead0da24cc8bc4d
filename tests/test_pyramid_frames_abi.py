"""CPU tests of dvo_op_pyramid_frames (include/dvo.h), the operator-level entry point of the batched pyramid build: it is declared,
exported, listed and bound, the header states the contract the reference (tests/pyramid_ref.py) is written from, the argument block
has the layout the binding assumes, INTEGRATION.md has its row, and every bad argument is refused with DVO_ERR_BAD_ARGUMENT before
anything touches the GPU -- here, on a machine without one, a call that got as far as the device would answer DVO_ERR_NO_DEVICE."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import dvo_amd as dvo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "dvo_op_pyramid_frames"


def _header():
    return open(os.path.join(ROOT, "include", "dvo.h")).read()


def test_declared_exported_and_listed():
    txt = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert re.search(r"\bint\s+dvo_op_pyramid_frames\s*\(\s*int\s+dev\s*,\s*const\s+dvo_config\s*\*\s*\w+\s*,\s*const\s+dvo_pyramid_frames_args\s*\*", txt)
    assert re.search(r"typedef\s+struct\s+dvo_pyramid_kernel\s*\{\s*int\s+kind,\s*culls,\s*plan;\s*\}", txt)
    for name, val in (("DVO_PYRAMID_KERNEL_SCALAR", 0), ("DVO_PYRAMID_KERNEL_RAW4", 1), ("DVO_PYRAMID_KERNEL_SPLIT", 2),
                      ("DVO_PYRAMID_KERNEL_REMAP", 3), ("DVO_PYRAMID_ROWS_DECIMATED", 1), ("DVO_PYRAMID_FORCE_WEIGHT_MAPS", 2),
                      ("DVO_PYRAMID_SPLIT", 4)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, val), txt), name
    assert hasattr(dvo.lib(), NAME) and NAME in dvo.EXPORTS
    assert (dvo.PYRAMID_KERNEL_SCALAR, dvo.PYRAMID_KERNEL_RAW4, dvo.PYRAMID_KERNEL_SPLIT, dvo.PYRAMID_KERNEL_REMAP) == (0, 1, 2, 3)
    assert (dvo.PYRAMID_ROWS_DECIMATED, dvo.PYRAMID_FORCE_WEIGHT_MAPS, dvo.PYRAMID_SPLIT) == (1, 2, 4)
    assert callable(dvo.op_pyramid_frames)
    assert NAME in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_the_header_states_the_contract():
    txt = " ".join(re.sub(r"\n\s*\*", " ", _header()).split())
    for phrase in ("(float)g8 * (float)(1/255)", "(R * 4899 + G * 9617 + B * 1868 + 8192) >> 14", "depth = (float)d16 * depth_scale",
                   "sigma = 0.1f where d16 > 0 else 1.0f", "gray = DVO_INVALID where d16 == 0", "s = culls + (levels - 1 - l)",
                   "NaN and every value <= DVO_INVALID replaced by DVO_INVALID", "the top level at culls = 0, which is the input unchanged",
                   "step_l / min(max(sigma, sigma_min), sigma_max), one float division", "keep_sigma = true", "words of 0xffffffff",
                   "which is no error: *ran says what ran", "A's top-level values decimated as above and A's wgt",
                   "its second input frame is not read", "returned before anything is queued"):
        assert phrase in txt, phrase


def test_struct_layouts():
    A = dvo.PyramidFramesArgs
    assert C.sizeof(A) == 128 and C.sizeof(dvo.PyramidKernel) == 12
    assert [getattr(A, f).offset for f in ("struct_size", "n_seq", "w", "h", "levels", "culls", "flags", "channels", "depth_scale")] == list(range(0, 36, 4))
    assert [getattr(A, f).offset for f in ("gray", "depth", "sigma", "rgb", "depth16", "seq_action", "gray2", "depth2", "sigma2", "rgb2",
                                           "depth16_2")] == list(range(40, 128, 8))
    k = dvo.PyramidKernel
    assert k(0, 0, 1).name() == "k_pyramid<true>" and k(1, 2, 0).name() == "k_pyramid_raw4<2, false>"
    assert k(2, 1, 0).name() == "k_pyramid_raw4_coarse<1> + k_pyramid_raw4_rest<1>"


W, H, LEVELS, CULLS, N = 88, 72, 4, 1, 2
_G = np.zeros((N, H, W), np.float32)
_U8 = np.zeros((N, H, W), np.uint8)
_U16 = np.zeros((N, H, W), np.uint16)
_ACT = np.array([0, 1], np.uint8)


def _args(**kw):
    a = dvo.PyramidFramesArgs()
    a.struct_size = C.sizeof(dvo.PyramidFramesArgs)
    a.n_seq, a.w, a.h, a.levels, a.culls, a.channels = N, W, H, LEVELS, CULLS, 1
    for k, v in kw.items():
        setattr(a, k, v.ctypes.data if isinstance(v, np.ndarray) else v)
    return a


def _call(a):
    return dvo.lib().dvo_op_pyramid_frames(0, None, C.byref(a) if a is not None else None, None, None, None, None, None)


BAD = {
    "struct_size": dict(rgb=_U8, struct_size=64),
    "n_seq": dict(rgb=_U8, n_seq=0),
    "neither input": dict(),
    "both inputs": dict(rgb=_U8, gray=_G),
    "depth without sigma": dict(gray=_G, depth=_G),
    "sigma without depth": dict(gray=_G, sigma=_G),
    "float maps beside raw": dict(rgb=_U8, depth=_G, sigma=_G),
    "raw depth beside float maps": dict(gray=_G, depth16=_U16),
    "channels": dict(rgb=_U8, channels=2),
    "depth_scale negative": dict(rgb=_U8, depth16=_U16, depth_scale=-1.0),
    "depth_scale nan": dict(rgb=_U8, depth16=_U16, depth_scale=float("nan")),
    "flags": dict(rgb=_U8, flags=8),
    "levels": dict(rgb=_U8, levels=9),
    "too small for the levels": dict(rgb=_U8, levels=5),
    "culls": dict(rgb=_U8, culls=-1),
    "rows decimated at culls 0": dict(rgb=_U8, culls=0, flags=1),
    "rows decimated at an odd height": dict(rgb=_U8, h=73, flags=1),
    "second frames without actions": dict(rgb=_U8, rgb2=_U8),
    "second depth without actions": dict(rgb=_U8, depth16=_U16, depth16_2=_U16),
    "actions without second frames": dict(rgb=_U8, seq_action=_ACT),
    "second frames of another kind": dict(rgb=_U8, seq_action=_ACT, gray2=_G),
    "second frames lack the depth": dict(rgb=_U8, depth16=_U16, seq_action=_ACT, rgb2=_U8),
    "second frames add a depth": dict(gray=_G, seq_action=_ACT, gray2=_G, depth2=_G, sigma2=_G),
    "bad action": dict(rgb=_U8, seq_action=np.array([1, 3], np.uint8), rgb2=_U8),
}


@pytest.mark.parametrize("case", sorted(BAD))
def test_bad_arguments_are_refused_before_the_device(case):
    assert _call(_args(**BAD[case])) == dvo.DVO_ERR_BAD_ARGUMENT, case
    assert dvo.lib().dvo_last_error()    # (says which)


def test_null_args_are_refused():
    assert _call(None) == dvo.DVO_ERR_BAD_ARGUMENT


@pytest.mark.skipif(dvo.device_count() > 0, reason="only meaningful on a box without a GPU")
def test_good_arguments_reach_the_device_and_fail_loudly_without_one():
    for kw in (dict(rgb=_U8), dict(rgb=_U8, depth16=_U16, flags=7 & ~1), dict(gray=_G, depth=_G, sigma=_G),
               dict(rgb=_U8, depth16=_U16, seq_action=_ACT, rgb2=_U8, depth16_2=_U16)):
        st = _call(_args(**kw))
        assert st not in (dvo.DVO_OK, dvo.DVO_ERR_BAD_ARGUMENT), kw.keys()
