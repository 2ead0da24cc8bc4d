"""Freeze the cases of tests/pose_cases.py and their 60-digit references (tests/pose_ref.py, mpmath) into pose_algebra.npz.

    python tests/golden/make_pose_algebra.py

tests/test_pose_algebra_host.py regenerates every 16th case and compares, so the file cannot drift from the two modules."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import pose_cases  # noqa: E402

if __name__ == "__main__":
    out = pose_cases.build()
    path = os.path.join(HERE, "pose_algebra.npz")
    np.savez_compressed(path, **out)
    for k, v in sorted(out.items()):
        print("%-10s %s" % (k, v.shape))
    print("%s: %d bytes" % (path, os.path.getsize(path)))
