"""CPU tests of the read-only view of a batch's level plan (include/dvo.h, dvo_debug_batch_level_plan): the entry point is declared,
exported and bound on both batch kinds, its launch-form constants agree between C and Python, and a NULL handle is refused before
anything touches the GPU.  A level outside the pyramid needs a live handle: tests/test_gpu_gn_instances.py holds that case."""
import os
import re

import dvo_amd as dvo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "dvo_debug_batch_level_plan"


def test_declared_exported_and_listed():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dvo.h")).read(), flags=re.S)
    args = r"dvo_batch\s*\*\s*\w+\s*,\s*int\s+\w+" + r"\s*,\s*int\s*\*\s*\w+" * 5
    assert re.search(r"\bint\s+%s\s*\(\s*%s\s*\)\s*;" % (NAME, args), txt)
    assert hasattr(dvo.lib(), NAME)
    assert NAME in dvo.EXPORTS
    assert NAME in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_launch_forms_are_declared():
    txt = open(os.path.join(ROOT, "include", "dvo.h")).read()
    for name, v in (("PAIRS", 0), ("ITERATION", 1), ("LEVEL", 2), ("LDS_PATCH", 3)):
        assert re.search(r"#define\s+DVO_PLAN_%s\s+%d\b" % (name, v), txt), name
        assert getattr(dvo, "PLAN_" + name) == v


def test_both_batches_bind_it():
    for cls in (dvo.Batch, dvo.MonoBatch):
        assert callable(getattr(cls, "level_plan", None)), cls.__name__


def test_null_handle_is_refused():
    import ctypes as C
    L = dvo.lib()
    v = [C.c_int(-7) for _ in range(5)]
    assert L.dvo_debug_batch_level_plan(None, 0, *[C.byref(x) for x in v]) == dvo.DVO_ERR_BAD_ARGUMENT
    assert L.dvo_debug_batch_level_plan(None, 0, None, None, None, None, None) == dvo.DVO_ERR_BAD_ARGUMENT
    assert all(x.value == -7 for x in v)    # nothing was written
