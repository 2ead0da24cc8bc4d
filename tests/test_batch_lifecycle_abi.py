"""CPU tests of the per-sequence skip / restart interface of a sensor-depth batch (include/dvo.h, dvo_batch_set_actions): the three
entry points are declared, exported and bound, the constants have their documented values, a NULL handle is refused without a
GPU, and the C++ facade's new methods compile."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

import dvo_amd as dvo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["dvo_batch_set_actions", "dvo_batch_last_status", "dvo_batch_copy_status_device"]
CONSTANTS = {"DVO_SEQ_SKIP": 0, "DVO_SEQ_TRACK": 1, "DVO_SEQ_RESTART": 2,
             "DVO_SEQ_TRACKED": 0, "DVO_SEQ_SKIPPED": 1, "DVO_SEQ_STARTED": 2, "DVO_SEQ_BAD_ACTION": 3}


def _header():
    return open(os.path.join(ROOT, "include", "dvo.h")).read()


def test_lifecycle_functions_are_declared_exported_and_bound():
    txt = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    L = dvo.lib()
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, txt), name
        assert hasattr(L, name), name
        assert name in dvo.EXPORTS, name


def test_lifecycle_constants_have_their_values():
    txt = _header()
    for name, value in CONSTANTS.items():
        m = re.search(r"#define\s+%s\s+(\d+)" % name, txt)
        assert m and int(m.group(1)) == value, name
        assert getattr(dvo, name[len("DVO_"):]) == value, name


def test_set_actions_refuses_a_null_handle():
    L = dvo.lib()
    acts = (C.c_uint8 * 4)(0, 1, 2, 1)
    assert L.dvo_batch_set_actions(None, acts, 0) == 1           # DVO_ERR_BAD_ARGUMENT
    assert L.dvo_batch_set_actions(None, None, 0) == 1
    st = (C.c_int * 4)()
    assert L.dvo_batch_last_status(None, st) == 1
    assert L.dvo_batch_copy_status_device(None, st) == 1


def test_facade_lifecycle_methods_compile(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("g++ not available")
    src = tmp_path / "snippet.cpp"
    src.write_text(r"""
#include "dvo.hpp"
#include <cstdint>
#include <vector>
int use(dvo::BatchTracker& bt, int* status_dev)
{
    std::vector<uint8_t> a(4, DVO_SEQ_TRACK);
    a[1] = DVO_SEQ_SKIP; a[2] = DVO_SEQ_RESTART;
    bt.setActions(a.data(), false);
    bt.setActions(nullptr, false);
    std::vector<int> st = bt.lastStatus();
    bt.copyStatusDevice(status_dev);
    return st.empty() ? -1 : (st[0] == DVO_SEQ_TRACKED ? 0 : st[0]);
}
""")
    r = subprocess.run([gxx, "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
