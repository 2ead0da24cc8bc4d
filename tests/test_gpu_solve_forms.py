"""Both forms of solve_gather behind every opt-in term's solve tail.

A solve kernel sums a sequence's partial rows with a 32-lane team per row class when the launch handles one or two sequences and with
a team per sequence, eight sequences per workgroup, otherwise; every term's serial tail runs behind both.  For each of the eight
sensor-depth states of tests/test_gpu_term_combinations.py, batches of 1, 2 (the wide form), 3 (the team form) and 9 sequences (one
sequence alone in a second solve workgroup) are fed the same three frames in every sequence: a start push and two tracking pushes.
Every sequence of every batch must then hold the same bits: xi, T, the track log, and the term's record and log.

The shape is test_gpu_geometric.py::test_every_kernel_instance's: 320x240, culls 1, three levels (40x30, 80x60, 160x120), crop off,
4 pixels per thread; the terms' configurations are their test files'."""
import numpy as np
import pytest

import dvo_amd as dvo
import term_batch as tb
from term_batch import CULLS, GEO, HUBER, KH, LEVELS, SIZE, STATES

pytestmark = pytest.mark.gpu

BATCHES = (1, 2, 3, 9)
PUSHES = (0, 1, 2)    # the frame every sequence is given at each push
AFF = dict(mode=dvo.AFFINE_ESTIMATE)

# how each setter of STATES is called, and what each state records: (name, read(bt, b) -> bytes or a tuple of them)
SET = dict(robust_weights=lambda bt: bt.set_robust_weights(**tb.rob(HUBER)),
           robust_median=lambda bt: bt.set_robust_median(**tb.md(HUBER)),
           affine_brightness=lambda bt: bt.set_affine_brightness(**AFF),
           geometric=lambda bt: bt.set_geometric(**GEO),
           geometric_affine=lambda bt: bt.set_geometric_affine(affine_mode=AFF["mode"], **GEO),
           step_control=lambda bt: bt.set_step_control())
ROBUST = [("last_robust_scales", lambda bt, b: bt.last_robust_scales()[b].tobytes())]
MEDIAN = ROBUST + [("last_robust_log", lambda bt, b: tb.rlogbits(bt.last_robust_log(b)))]
AFFINE = [("last_affine", lambda bt, b: bt.last_affine()[b].tobytes()), ("last_affine_log", lambda bt, b: tb.alogbits(bt.last_affine_log(b)))]
GEOMETRIC = [("last_geometric", lambda bt, b: bt.last_geometric()[b].tobytes()),
             ("last_geometric_log", lambda bt, b: tb.glogbits(bt.last_geometric_log(b)))]
STEP = [("last_step_control", lambda bt, b: bt.last_step_control()[b].tobytes()),
        ("last_step_control_log", lambda bt, b: tb.lmbits(bt.last_step_control_log(b)))]
RECORDS = dict(N=[], R=ROBUST, M=MEDIAN, A=AFFINE, RA=ROBUST + AFFINE, G=GEOMETRIC, GA=GEOMETRIC + AFFINE, L=STEP)


def _run(state, B):
    """per tracking push and sequence: dict(xi, T, log, <the state's records>), everything as bytes"""
    g, d, s = tb.frames(SIZE)
    bt = dvo.Batch(B, KH, SIZE[0], SIZE[1], LEVELS, CULLS, cfg=tb.cfg(fixed_iterations=0))
    for setter in STATES[state]:
        SET[setter](bt)
    keep, outs = [], []
    for k, frame in enumerate(PUSHES):
        t = [tb.dev(np.repeat(x[frame][None], B, axis=0)) for x in (g, d, s)]
        keep.append(t)
        bt.push_device(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr())
        if k == 0:
            continue
        xi, T = bt.last_poses()
        outs.append([dict([("xi", xi[b].tobytes()), ("T", T[b].tobytes()), ("log", tb.logbits(bt.last_track_log(b)))] +
                          [(name, read(bt, b)) for name, read in RECORDS[state]]) for b in range(B)])
    bt.close()
    return outs


@pytest.mark.parametrize("state", list(STATES))
def test_every_batch_size_gives_the_same_bits(state):
    assert set(RECORDS) == set(STATES)
    ref = _run(state, BATCHES[0])
    assert len(ref) == len(PUSHES) - 1
    for k, push in enumerate(ref):    # the frames move: something was tracked, and the records are not all empty
        assert np.frombuffer(push[0]["xi"], np.float32).any(), (state, k)
    for B in BATCHES[1:]:
        got = _run(state, B)
        for k, push in enumerate(got):
            assert len(push) == B
            for b, seq in enumerate(push):
                for name, bits in seq.items():
                    assert bits == ref[k][0][name], "state %s, B = %d, push %d, sequence %d: %s differs from the batch of one" % (
                        state, B, k + 1, b, name)
