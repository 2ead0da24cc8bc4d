"""tests/term_batch.py holds what the six copies it replaced held: run() makes its calls in the one order, same() rejects a difference
in every field the copies compared, and walk() follows the references and keeps the closing counts.

No device: a fake batch stands in for dvo.Batch, records every call and hands back values drawn from a seeded generator; the frames
are a few pixels and go through the host feed, so neither torch nor the library is loaded."""
import copy

import numpy as np
import pytest

import term_batch as tb
from term_batch import LEVELS, SKIPPED, STARTED, TRACKED

B = 3
F32 = np.float32
ALL = tuple(tb.FAMILIES)


class FakeBatch:
    """records (method, note) in self.calls; the notes tell the calls of one name apart"""
    made = []

    def __init__(self, n, K, w, h, levels, culls, cfg=None):
        self.calls = [("Batch", (n, w, h, levels, culls))]
        self.rng = np.random.default_rng(7)
        FakeBatch.made.append(self)

    def _arr(self, shape, dtype=F32):
        return self.rng.random(shape).astype(dtype) if dtype == F32 else self.rng.integers(1, 9, shape).astype(dtype)

    def _side_log(self, **fields):
        return dict(levels=LEVELS, n_iter=self._arr(LEVELS, np.int32), **{k: self._arr((LEVELS, 4), t) for k, t in fields.items()})

    def __getattr__(self, name):     # the setters, the feed and close: recorded, nothing returned
        def call(*a, **kw):
            note = a[0] if name in ("set_intrinsics", "set_actions", "set_pose_guess") else None
            self.calls.append((name, None if note is None else float(np.asarray(note).ravel()[0])))
        return call

    def _returns(name, make):
        def method(self, *a):
            self.calls.append((name, a[0] if a else None))
            return make(self)
        return method

    level_plan = _returns("level_plan", lambda s: dict(ppt=4))
    last_status = _returns("last_status", lambda s: np.full(B, TRACKED, np.uint8))
    last_track_quality = _returns("last_track_quality", lambda s: s._arr(B))
    last_poses = _returns("last_poses", lambda s: (s._arr((B, 6)), s._arr((B, 4, 4))))
    world_poses = _returns("world_poses", lambda s: (s._arr((B, 6)), s._arr((B, 4, 4)), s._arr(B, np.uint8)))
    last_track_log = _returns("last_track_log", lambda s: dict(s._side_log(residual=F32, upd_norm=F32, n_valid=np.int32),
                                                               xi_after=s._arr((LEVELS, 4, 6)), xi_update=s._arr((LEVELS, 4, 6))))
    last_robust_scales = _returns("last_robust_scales", lambda s: s._arr(B))
    last_robust_log = _returns("last_robust_log", lambda s: dict(s._side_log(s2=F32, median_bin=np.int32, count=np.int32), prime_bin=3, prime_count=5))
    last_robust_histogram = _returns("last_robust_histogram", lambda s: s._arr(256, np.uint32))
    last_affine = _returns("last_affine", lambda s: s._arr((B, 2)))
    last_affine_log = _returns("last_affine_log", lambda s: dict(s._side_log(a=F32, b=F32), prime_a=F32(1.5), prime_b=F32(0.25)))
    last_geometric = _returns("last_geometric", lambda s: s._arr(B))
    last_geometric_log = _returns("last_geometric_log", lambda s: s._side_log(n_geo=np.int32, sum_sq=F32))
    last_step_control = _returns("last_step_control", lambda s: s._arr(B))
    last_step_control_log = _returns("last_step_control_log", lambda s: s._side_log(lambda_=F32, decision=np.int32))
    last_start_poses = _returns("last_start_poses", lambda s: s._arr((B, 6)))


@pytest.fixture(autouse=True)
def _fake(monkeypatch):
    FakeBatch.made.clear()
    monkeypatch.setattr(tb.dvo, "Batch", FakeBatch)


def _maps(k, b):
    return tuple(np.full((6, 8), v + k + 0.1 * b, F32) for v in (0.0, 1.0, 2.0))


def _run(pushes=2, **kw):
    kw.setdefault("maps", _maps)
    outs = tb.run(None, B, [[0] * B] * pushes, feed="host", size=(8, 6), **kw)
    return outs, FakeBatch.made[-1].calls


# ------------------------------------------------------------------------------------------------------------------ run
def test_run_makes_its_calls_in_the_one_order():
    seen = []

    def maps(k, b):
        FakeBatch.made[-1].calls.append(("maps", (k, b)))
        return _maps(k, b)

    def setup(bt, keep):
        bt.set_step_control()
        keep.append("rows")
        seen.append(keep)
    cams, new = np.full((B, 3, 3), 1.0, F32), np.full((B, 3, 3), 2.0, F32)
    outs, calls = _run(setup=setup, reads=("step", "start"), maps=maps, at={1: lambda bt: bt.set_geometric(None)}, acts=np.full((2, B), 5, np.uint8),
                       kf=True, cams=cams, cams_at=(1, new), D=np.zeros(5, F32), guess=[np.full((B, 6), 3.0, F32), np.full((B, 6), 4.0, F32)])
    per_b = lambda name: [(name, b) for b in range(B)]
    after = ([("last_status", None), ("last_track_quality", None), ("last_step_control", None)] + per_b("last_step_control_log") +
             [("last_start_poses", None), ("last_poses", None)] + per_b("last_track_log") + [("world_poses", None)])
    want = ([("Batch", (B, 8, 6, tb.LEVELS, tb.CULLS)), ("set_keyframe_tracking", None), ("set_track_quality", None), ("set_intrinsics", 1.0),
             ("set_distortion", None), ("set_pose_guess_mode", None), ("set_step_control", None)] + per_b("level_plan") +
            [("maps", (0, b)) for b in range(B)] + [("set_actions", 5.0), ("set_pose_guess", 3.0), ("push_host", None)] + after +
            [("set_geometric", None)] + [("maps", (1, b)) for b in range(B)] +
            [("set_actions", 5.0), ("set_pose_guess", 4.0), ("set_intrinsics", 2.0), ("push_host", None)] + after + [("close", None)])
    assert calls == want
    assert seen == [["rows"]]     # (the host feed keeps nothing more)
    assert all(o["plan"] == [dict(ppt=4)] * LEVELS and len(o["maps"]) == B for o in outs)
    assert all(set(o) == {"status", "q", "maps", "plan", "rec", "lmlogs", "start", "xi", "T", "logs", "world"} for o in outs)


def test_run_without_options_sets_nothing():
    outs, calls = _run(quality=False)
    names = [c[0] for c in calls]
    assert names[:1 + LEVELS] == ["Batch"] + ["level_plan"] * LEVELS and names[1 + LEVELS] == "push_host"
    assert not [n for n in names if n.startswith("set_")] and "last_track_quality" not in names
    assert outs[0]["q"] is None and set(outs[0]) == {"status", "q", "maps", "plan"}


@pytest.mark.parametrize("kw,first,world", [({}, False, False), (dict(acts=np.zeros((2, B), np.uint8)), True, False), (dict(kf=True), True, True)])
def test_poses_and_logs_are_read_under_the_stated_conditions_only(kw, first, world):
    """xi, T and logs: from the second push on, or from the first with actions or keyframe tracking; world: with keyframe tracking"""
    outs, _ = _run(**kw)
    for k, o in enumerate(outs):
        assert all((key in o) == (k > 0 or first) for key in ("xi", "T", "logs")), (k, sorted(o))
        assert ("world" in o) == world


def test_unknown_feed_is_refused():
    with pytest.raises(AssertionError):
        tb.run(None, B, [[0] * B], maps=_maps, feed="prefetch", size=(8, 6))


# ------------------------------------------------------------------------------------------------------------------ same
def _flip(a):
    a.view(np.uint8).reshape(-1)[0] ^= 1


def _bump(d, key):
    d[key] = type(d[key])(d[key] + 1)


# one field of a push that same() must compare -> (family or None, mutate(o))
FIELDS = {
    "status": (None, lambda o: _flip(o["status"])), "xi": (None, lambda o: _flip(o["xi"])), "T": (None, lambda o: _flip(o["T"])),
    "q": (None, lambda o: _flip(o["q"])), "world flags": (None, lambda o: _flip(o["world"][2])), "world T": (None, lambda o: _flip(o["world"][1])),
    "log n_iter": (None, lambda o: _flip(o["logs"][1]["n_iter"])), "log residual": (None, lambda o: _flip(o["logs"][1]["residual"])),
    "log upd_norm": (None, lambda o: _flip(o["logs"][0]["upd_norm"])), "log xi_after": (None, lambda o: _flip(o["logs"][2]["xi_after"])),
    "log xi_update": (None, lambda o: _flip(o["logs"][0]["xi_update"])), "log n_valid": (None, lambda o: _flip(o["logs"][1]["n_valid"])),
    "s2": ("robust", lambda o: _flip(o["s2"])), "hist": ("median", lambda o: _flip(o["hist"])),
    "rlog s2": ("median", lambda o: _flip(o["rlogs"][1]["s2"])), "rlog median_bin": ("median", lambda o: _flip(o["rlogs"][0]["median_bin"])),
    "rlog count": ("median", lambda o: _flip(o["rlogs"][2]["count"])), "rlog prime_bin": ("median", lambda o: _bump(o["rlogs"][0], "prime_bin")),
    "rlog prime_count": ("median", lambda o: _bump(o["rlogs"][0], "prime_count")), "rlog n_iter": ("median", lambda o: _flip(o["rlogs"][0]["n_iter"])),
    "ab": ("affine", lambda o: _flip(o["ab"])), "alog a": ("affine", lambda o: _flip(o["alogs"][1]["a"])),
    "alog b": ("affine", lambda o: _flip(o["alogs"][1]["b"])), "alog prime_a": ("affine", lambda o: _bump(o["alogs"][2], "prime_a")),
    "alog prime_b": ("affine", lambda o: _bump(o["alogs"][2], "prime_b")), "alog n_iter": ("affine", lambda o: _flip(o["alogs"][0]["n_iter"])),
    "alog levels": ("affine", lambda o: _bump(o["alogs"][0], "levels")),
    "grec": ("geometric", lambda o: _flip(o["grec"])), "glog n_geo": ("geometric", lambda o: _flip(o["glogs"][1]["n_geo"])),
    "glog sum_sq": ("geometric", lambda o: _flip(o["glogs"][1]["sum_sq"])), "glog n_iter": ("geometric", lambda o: _flip(o["glogs"][2]["n_iter"])),
    "glog levels": ("geometric", lambda o: _bump(o["glogs"][2], "levels")),
    "rec": ("step", lambda o: _flip(o["rec"])), "lmlog lambda": ("step", lambda o: _flip(o["lmlogs"][0]["lambda_"])),
    "lmlog decision": ("step", lambda o: _flip(o["lmlogs"][1]["decision"])), "lmlog n_iter": ("step", lambda o: _flip(o["lmlogs"][1]["n_iter"])),
    "start": ("start", lambda o: _flip(o["start"])),
}


@pytest.fixture(scope="module")
def full_run():
    """three pushes with every family read and keyframe tracking on: every key a push can have"""
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(tb.dvo, "Batch", FakeBatch)
        return tb.run(None, B, [[0] * B] * 3, maps=_maps, feed="host", size=(8, 6), reads=ALL, kf=True)


def test_same_accepts_a_copy(full_run):
    tb.same(full_run, copy.deepcopy(full_run))
    tb.same(full_run, copy.deepcopy(full_run), families=ALL)
    assert {f for f, _ in FIELDS.values()} == set(ALL) | {None}
    assert {k for fam in tb.FAMILIES.values() for k in fam.keys} <= set(full_run[0])


@pytest.mark.parametrize("field", list(FIELDS))
@pytest.mark.parametrize("side", [0, 1])
def test_same_rejects_one_flipped_bit(field, side, full_run):
    runs = [copy.deepcopy(full_run), copy.deepcopy(full_run)]
    FIELDS[field][1](runs[side][1])
    for families in (None, ALL):
        with pytest.raises(AssertionError):
            tb.same(runs[0], runs[1], families=families)
    tb.same(runs[0], runs[1], pushes=(0, 2))    # (the other pushes are untouched)


@pytest.mark.parametrize("family", ALL)
def test_same_rejects_a_family_read_in_one_run_only(family, full_run):
    other = copy.deepcopy(full_run)
    for key in tb.FAMILIES[family].keys:
        del other[2][key]
    with pytest.raises(AssertionError):
        tb.same(full_run, other)
    with pytest.raises(AssertionError):
        tb.same(other, full_run)
    if family not in ("robust", "median"):    # (the two share s2)
        tb.same(full_run, other, families=tuple(f for f in ALL if f not in (family, "robust", "median")))


@pytest.mark.parametrize("field", list(FIELDS))
def test_same_with_a_restriction_ignores_the_excluded_families_only(field, full_run):
    family = FIELDS[field][0]
    other = copy.deepcopy(full_run)
    FIELDS[field][1](other[0])
    shares = lambda f: f == family or (field == "s2" and f == "median")    # (the median family reads s2 as well)
    if family:
        tb.same(full_run, other, families=tuple(f for f in ALL if not shares(f)))
    for families in [(), ("affine",), ("robust", "step"), ("median", "geometric", "start")]:
        if family is None or any(shares(f) for f in families):
            with pytest.raises(AssertionError):
                tb.same(full_run, other, families=families)
        else:
            tb.same(full_run, other, families=families)


@pytest.mark.parametrize("reads,field", [(("robust",), "s2"), (("affine", "geometric"), "glog sum_sq"), ((), "q")])
def test_same_compares_the_families_a_run_has_read(reads, field):
    """a run that read the scales alone is a robust run although the median family fills s2 as well"""
    a = tb.run(None, B, [[0] * B] * 2, maps=_maps, feed="host", size=(8, 6), reads=reads)
    b = copy.deepcopy(a)
    tb.same(a, b)
    FIELDS[field][1](b[1])
    with pytest.raises(AssertionError):
        tb.same(a, b)


def test_same_rejects_runs_of_different_shape(full_run):
    with pytest.raises(AssertionError):
        tb.same(full_run, full_run[:2])
    for key in ("xi", "world", "q"):
        other = copy.deepcopy(full_run)
        if key == "q":
            other[1]["q"] = None
        else:
            del other[1][key]
        with pytest.raises((AssertionError, KeyError)):
            tb.same(full_run, other)


# ------------------------------------------------------------------------------------------------------------------ walk
def _outs(statuses, promoted=None):
    """pushes with the given status rows; promoted[k][b]: the keyframe flag of world_poses"""
    return [dict(status=np.array(row, np.uint8), empty=[True] * len(row), world=(None, None, np.array(promoted[k] if promoted else [0] * len(row))))
            for k, row in enumerate(statuses)]


def _walk(outs, its=4, **kw):
    seen = []

    def check(k, b, kr, o, K):
        assert o is outs[k]
        seen.append((k, b, kr, float(K[0, 0])))
        return its
    n, n_it = tb.walk(outs, len(outs[0]["status"]), check, lambda o, b: o["empty"][b], **kw)
    assert (n, n_it) == (len(seen), its * len(seen))
    return seen


S, T, X = STARTED, TRACKED, SKIPPED
KH00 = float(tb.KH[0, 0])


def test_walk_follows_the_last_tracked_or_started_push():
    seen = _walk(_outs([[S, S], [T, X], [T, T]]), min_tracked=3)
    assert seen == [(1, 0, 0, KH00), (2, 0, 1, KH00), (2, 1, 0, KH00)]     # (the skipped push of sequence 1 holds no reference)


def test_walk_with_keyframes_follows_promotions_only():
    outs = _outs([[S, S], [T, T], [T, T], [T, T]], promoted=[[0, 0], [0, 1], [1, 0], [0, 0]])
    assert [s[:3] for s in _walk(outs, kf=True)] == [(1, 0, 0), (1, 1, 0), (2, 0, 0), (2, 1, 1), (3, 0, 2), (3, 1, 1)]
    assert [s[:3] for s in _walk(outs)] == [(1, 0, 0), (1, 1, 0), (2, 0, 1), (2, 1, 1), (3, 0, 2), (3, 1, 2)]


@pytest.mark.parametrize("kf", [False, True])
def test_walk_restart_resets_the_reference(kf):
    outs = _outs([[S, S], [T, T], [S, T], [T, T]], promoted=[[0, 0], [1, 0], [0, 0], [0, 0]])
    seen = _walk(outs, kf=kf, min_tracked=5)
    assert [s[:3] for s in seen if s[1] == 0] == [(1, 0, 0), (3, 0, 2)]
    assert [s[:3] for s in seen if s[1] == 1] == [(1, 1, 0), (2, 1, 0 if kf else 1), (3, 1, 0 if kf else 2)]


def test_walk_switches_cameras_at_the_push():
    cams, new = np.full((2, 3, 3), 1.0, F32), np.full((2, 3, 3), 2.0, F32)
    cams[1] *= 3; new[1] *= 3
    outs = _outs([[S, S], [T, T], [T, T]])
    assert [s[3] for s in _walk(outs, cams=cams)] == [1.0, 3.0, 1.0, 3.0]
    assert [s[3] for s in _walk(outs, cams=cams, cams_at=(2, new))] == [1.0, 3.0, 2.0, 6.0]
    assert [s[3] for s in _walk(outs, cams_at=(2, new))] == [KH00, KH00, 2.0, 6.0]


def test_walk_filters_sequences_but_not_the_empty_rule():
    outs = _outs([[S, S, S], [T, T, X], [T, T, T]])
    assert [s[:2] for s in _walk(outs, seqs=(1,))] == [(1, 1), (2, 1)]
    outs[1]["empty"][2] = False     # a record on the SKIPPED sequence, which is not among seqs
    with pytest.raises(AssertionError):
        _walk(outs, seqs=(1,))
    outs[1]["empty"] = [False, False, True]     # (a TRACKED sequence is never asked)
    _walk(outs, seqs=(1,))


@pytest.mark.parametrize("status", [S, X, tb.BAD])
def test_walk_rejects_a_record_on_a_sequence_that_did_not_track(status):
    outs = _outs([[S, S], [T, status], [T, T]])
    _walk(outs, min_tracked=3)
    outs[1]["empty"][1] = False
    with pytest.raises(AssertionError):
        _walk(outs, min_tracked=3)


def test_walk_closing_counts():
    outs = _outs([[S, S], [T, X], [T, T]])
    with pytest.raises(AssertionError):
        _walk(outs)                     # 3 tracked, every sequence at both pushes asked
    _walk(outs, min_tracked=3)
    with pytest.raises(AssertionError):
        _walk(outs, min_tracked=4)
    with pytest.raises(AssertionError):
        _walk(outs, min_tracked=3, its=3)   # more than three iterations per sequence
    _walk(outs, min_tracked=3, its=3, iters_per_seq=2)
    with pytest.raises(AssertionError):
        _walk(outs, min_tracked=0, its=0, iters_per_seq=0)   # something must have been replayed
    with pytest.raises(AssertionError):
        _walk(_outs([[S, S], [X, T], [T, T]]), seqs=(0,))    # sequence 0 tracked once, both pushes are asked
