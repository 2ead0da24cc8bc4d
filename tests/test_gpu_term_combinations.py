"""Which opt-in tracking terms of a batch combine: the whole matrix of states and setters, through the C API.

One sensor-depth batch and one mono batch of two sequences, no frame pushed.  For every reachable state and every setter's "on" call:
the status, after a refusal the message (the C function's name, the offending term that is really on and that term's setter), that
the refusal changed nothing, and that every "off" form is always allowed."""
import ctypes as C

import pytest

import dvo_amd as dvo
from term_batch import CULLS, KH, LEVELS, SIZE, STATES
from util import K640

pytestmark = pytest.mark.gpu

# (STATES, tests/term_batch.py: the setters that make up each reachable state, from "everything off")
# An offender: the word the message must contain and the setter it must name
ROBUST = ("robust", "dvo_batch_set_robust_weights")
MEDIAN = ("median", "dvo_batch_set_robust_median")
ROBUST_M = ("robust", "dvo_batch_set_robust_median")    # the median scale, refused as robust weights
AFFINE = ("affine", "dvo_batch_set_affine_brightness")
GEO = ("geometric", "dvo_batch_set_geometric")
LM = ("step control", "dvo_batch_set_step_control")
# TABLE[setter][state]: () = DVO_OK, else DVO_ERR_BAD_ARGUMENT naming one of these offenders
TABLE = {
    "robust_weights":    dict(N=(), R=(), M=(), A=(), RA=(), G=(GEO,), GA=(GEO,), L=(LM,)),
    "robust_median":     dict(N=(), R=(), M=(), A=(AFFINE,), RA=(AFFINE,), G=(GEO,), GA=(GEO, AFFINE), L=(LM,)),
    "affine_brightness": dict(N=(), R=(), M=(MEDIAN,), A=(), RA=(), G=(GEO,), GA=(GEO,), L=(LM,)),
    "geometric":         dict(N=(), R=(ROBUST,), M=(ROBUST_M,), A=(AFFINE,), RA=(ROBUST, AFFINE), G=(), GA=(AFFINE,), L=(LM,)),
    "geometric_affine":  dict(N=(), R=(ROBUST,), M=(ROBUST_M,), A=(), RA=(ROBUST,), G=(), GA=(), L=(LM,)),
    "step_control":      dict(N=(), R=(ROBUST,), M=(MEDIAN,), A=(AFFINE,), RA=(AFFINE, ROBUST), G=(GEO,), GA=(GEO, AFFINE), L=()),
}
MONO_STATES = ["N", "R", "M", "A", "RA", "L"]
MONO_SETTERS = ["robust_weights", "robust_median", "affine_brightness", "step_control"]


def _robust(kind, mode):
    return dvo.RobustConfig(C.sizeof(dvo.RobustConfig), kind, mode, 1.345, 1e-3)


def _affine(mode):
    return dvo.AffineConfig(C.sizeof(dvo.AffineConfig), mode, 64, 1e-3, 0.25, 4.0)


def _geo(mode):
    return dvo.GeometricConfig(C.sizeof(dvo.GeometricConfig), mode, 10.0, 0.1)


def _lm(mode):
    c = dvo.lm_default_config()
    c.mode = mode
    return c


def _on(L, p, setter):
    """the setter's "on" call: (status, the C function's name)"""
    if setter == "robust_weights":
        return L.dvo_batch_set_robust_weights(p, C.byref(_robust(dvo.ROBUST_HUBER, dvo.ROBUST_SCALE_ADAPTIVE))), "dvo_batch_set_robust_weights"
    if setter == "robust_median":
        return L.dvo_batch_set_robust_median(p, C.byref(_robust(dvo.ROBUST_HUBER, dvo.ROBUST_SCALE_MEDIAN))), "dvo_batch_set_robust_median"
    if setter == "affine_brightness":
        return L.dvo_batch_set_affine_brightness(p, C.byref(_affine(dvo.AFFINE_ESTIMATE))), "dvo_batch_set_affine_brightness"
    if setter == "geometric":
        return L.dvo_batch_set_geometric(p, C.byref(_geo(dvo.GEOMETRIC_ON))), "dvo_batch_set_geometric"
    if setter == "geometric_affine":
        return (L.dvo_batch_set_geometric_affine(p, C.byref(_geo(dvo.GEOMETRIC_ON)), C.byref(_affine(dvo.AFFINE_ESTIMATE))),
                "dvo_batch_set_geometric_affine")
    return L.dvo_batch_set_step_control(p, C.byref(_lm(dvo.LM_ON))), "dvo_batch_set_step_control"


def _off_forms(L, p, mono):
    """every setter's "off" forms (NULL and the OFF / NONE mode), as (name, status)"""
    out = [("robust_weights(NULL)", L.dvo_batch_set_robust_weights(p, None)),
           ("robust_weights(NONE)", L.dvo_batch_set_robust_weights(p, C.byref(_robust(dvo.ROBUST_NONE, dvo.ROBUST_SCALE_ADAPTIVE)))),
           ("robust_median(NULL)", L.dvo_batch_set_robust_median(p, None)),
           ("affine_brightness(NULL)", L.dvo_batch_set_affine_brightness(p, None)),
           ("affine_brightness(OFF)", L.dvo_batch_set_affine_brightness(p, C.byref(_affine(dvo.AFFINE_OFF)))),
           ("step_control(NULL)", L.dvo_batch_set_step_control(p, None)),
           ("step_control(OFF)", L.dvo_batch_set_step_control(p, C.byref(_lm(dvo.LM_OFF))))]
    if not mono:
        out += [("geometric(NULL)", L.dvo_batch_set_geometric(p, None)),
                ("geometric(OFF)", L.dvo_batch_set_geometric(p, C.byref(_geo(dvo.GEOMETRIC_OFF))))]
    return out


def _matrix(L, p, states, setters, mono):
    """walks the table; returns the cells that disagree"""
    wrong = []

    def reach(state, what):
        for name, st in _off_forms(L, p, mono):
            if st != dvo.DVO_OK:
                wrong.append("%s: %s returned %d" % (what, name, st))
        for s in STATES[state]:
            st, _ = _on(L, p, s)
            if st != dvo.DVO_OK:
                wrong.append("%s: reaching %s, %s returned %d (%s)" % (what, state, s, st, L.dvo_last_error().decode()))

    for state in states:
        for setter in setters:
            cell = "%s in state %s" % (setter, state)
            reach(state, cell)
            st, fn = _on(L, p, setter)
            offenders = TABLE[setter][state]
            if st != (dvo.DVO_ERR_BAD_ARGUMENT if offenders else dvo.DVO_OK):
                wrong.append("%s: status %d" % (cell, st))
            if not offenders or st == dvo.DVO_OK:
                continue
            msg = L.dvo_last_error().decode()
            if not msg.startswith(fn + ": "):
                wrong.append("%s: the message does not start with the function's name: %r" % (cell, msg))
            if not any(word in msg for word, _ in offenders):
                wrong.append("%s: the message names none of %s: %r" % (cell, [w for w, _ in offenders], msg))
            if not any(word in msg and "(" + their + ")" in msg for word, their in offenders):
                wrong.append("%s: the message names no offender's setter: %r" % (cell, msg))
            # the refusal changed nothing: what was on goes off and on again (reach asserts both), and the same call is refused again
            reach(state, cell + ", after the refusal")
            if _on(L, p, setter)[0] != dvo.DVO_ERR_BAD_ARGUMENT:
                wrong.append("%s: allowed at the second attempt" % cell)
        reach("N", "leaving state %s" % state)
    return wrong


def test_sensor_depth_batch_matrix():
    L = dvo.lib()
    bt = dvo.Batch(2, KH, SIZE[0], SIZE[1], LEVELS, CULLS)
    wrong = _matrix(L, bt._p, list(STATES), list(TABLE), mono=False)
    bt.close()
    print("\n".join(wrong))
    assert not wrong, "%d cells disagree with the table" % len(wrong)


def test_mono_batch_matrix():
    L = dvo.lib()
    mb = dvo.MonoBatch(2, K640, 640, 480, cfg=dvo.default_config(rng_seed=3))
    wrong = _matrix(L, mb._p, MONO_STATES, MONO_SETTERS, mono=True)
    # the geometric setters need a sensor-depth batch, whatever is on and whatever they ask for (ahead of the table)
    for state in MONO_STATES:
        for s in STATES[state]:
            assert _on(L, mb._p, s)[0] == dvo.DVO_OK
        for setter in ("geometric", "geometric_affine"):
            st, fn = _on(L, mb._p, setter)
            msg = L.dvo_last_error().decode()
            if st != dvo.DVO_ERR_BAD_ARGUMENT or not msg.startswith(fn + ": ") or "sensor-depth batch" not in msg:
                wrong.append("%s on a mono batch in state %s: status %d, %r" % (setter, state, st, msg))
        assert all(st == dvo.DVO_OK for _, st in _off_forms(L, mb._p, True))
    mb.close()
    print("\n".join(wrong))
    assert not wrong, "%d cells disagree with the table" % len(wrong)
