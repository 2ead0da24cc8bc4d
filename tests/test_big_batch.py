"""The helper of the batches above 1024 sequences (tests/big_batch.py) on the CPU: the replication table, the sample, the subset sums and,
with the oracle alone (orc.OVO), that the chosen bases, frame orders and replication counts produce every keyframe-count class that
tests/test_gpu_batch_over_1024.py asserts on the device's flags -- the condition that keeps the GPU test from passing vacuously."""
import numpy as np
import pytest

import big_batch as bb
import orc
import test_gpu_mono_lockstep as tl

SIZES = [(192, 144), (200, 152)]      # tests/test_gpu_batch_over_1024.py: every level a multiple of 4 pixels; none of them
CASES = [(1025, 8), (2600, 10)]


def test_sizes_of_the_paths_above_1024():
    assert [bb.scan_per(n) for n in (1, 1024, 1025, 2048, 2049, 2600, 32808)] == [1, 1, 2, 2, 3, 3, 33]
    assert [bb.list_rounds(n, 2600) for n in (0, 1, 1024, 1025, 2048, 2049, 2600)] == [0, 1, 1, 2, 2, 3, 3]
    assert bb.list_rounds(1025, 1025) == 2 and bb.list_rounds(12, 12) == 1 and bb.list_rounds(1000, 12) == 84
    assert [bb.grid_z(n) for n in (1, 32767, 32768, 32769, 32808)] == [1, 1, 1, 2, 2]
    assert [bb.key_class(n) for n in (0, 1, 1023, 1024, 1025, 2048, 2049)] == ["0", "1..1023", "1..1023", "1024", "1025..2048",
                                                                             "1025..2048", ">2048"]


@pytest.mark.parametrize("B,M", CASES + [(32808, 10)])
def test_replication_table_and_sample(B, M):
    counts = bb.skewed_counts(B, M)
    assert sum(counts) == B and len(counts) == M
    for target in (0, 1, 1023, 1024, 1025, B) + ((2049,) if B >= 2600 else ()):
        sub = bb.subset_with_sum(counts, target)
        assert sum(counts[m] for m in sub) == target
    base = bb.replicate(B, counts)
    assert base.tobytes() == bb.replicate(B, counts).tobytes()          # a fixed seed
    assert not np.array_equal(base, np.sort(base)) and not np.array_equal(base, np.arange(B) % M)
    for b in bb.BOUNDARIES:
        if b < B:
            assert base[b - 1] != base[b]
    s = bb.sample(base)
    assert len(s) >= 32 and len(set(s)) == len(s) and B - 1 in s
    assert all(q in s for q in bb.MUST_SAMPLE if q < B)
    assert {int(base[q]) for q in s} == set(range(M))                   # every base is sampled somewhere
    cov = bb.rounds_covered(base, s)
    for r in (1, 2):
        lo, hi = r * bb.LIST_SLOTS, min(B, (r + 1) * bb.LIST_SLOTS)
        assert cov[r] == {int(m) for m in np.unique(base[lo:hi])}, r    # every base that has a replica in that round's indices


def test_even_replication_mixes_neighbours_and_pins():
    B, M = 32808, 10
    pin = np.arange(32769, 32769 + 20)
    counts = bb.split_even(B - 20, M - 1) + [20]
    base = bb.replicate(B, counts, pinned={M - 1: pin})
    assert (base[pin] == M - 1).all() and (base == M - 1).sum() == 20
    assert bb.neighbour_mix(base) > 0.8                                 # (1 - 1 / 9 for an even table)
    assert base[32767] != base[32768]
    with pytest.raises(ValueError):
        bb.skewed_counts(900, 8)
    with pytest.raises(ValueError):
        bb.subset_with_sum([1, 2, 4], 8)


def _oracle_flags(w, h, counts, Ks=None):
    """per call and base: (keyframe flag, |t| of the tracked twist, valid updates) of orc.OVO on the schedule of big_batch.mono_orders"""
    orders, n_ctl = bb.mono_orders(counts)
    flags, tn, upd = [], [], []
    for m, order in enumerate(orders):
        K = tl._scaled(tl.K640 if Ks is None else Ks[m], w, h)
        g, _ = tl.render(K, w, h)
        init = tl.init_depth(K, w, h)
        ovo = orc.OVO(K, w, h, seed=tl.SEED)
        ovo.set_initial_depth(init, np.full_like(init, tl.INIT_SIGMA))
        f, t, u = [], [], []
        for i in order:
            _, key = ovo.odometrize(g[i])
            fr = ovo.keyframe(ovo.keyframe_count() - 1) if key else ovo.last_frame()
            f.append(key); t.append(float(np.linalg.norm(np.asarray(fr.rel_xi, np.float64)[:3]))); u.append(ovo.last_valid_updates())
        flags.append(f); tn.append(t); upd.append(u)
    return np.array(flags).T, np.array(tn).T, np.array(upd).T, n_ctl


@pytest.mark.parametrize("w,h", SIZES)
def test_the_oracle_alone_reaches_every_keyframe_count_class(w, h):
    seen = set()
    for B, M in CASES:
        counts = bb.skewed_counts(B, M)
        flags, tn, upd, n_ctl = _oracle_flags(w, h, counts)
        n, cls = bb.classes_of(flags, counts)
        print("%dx%d B = %d: keyframe-creating sequences per call %s" % (w, h, B, n))
        want = {"0", "1..1023", "1024", "1025..2048"} | ({">2048"} if B > 2049 else set())
        assert want <= cls, (B, n)
        seen |= cls
        # the controlled calls decide far from the rule's threshold: a twist of 0 or a translation of at least ten times 0.02
        ctl = tn[1:n_ctl]
        assert ((ctl < 0.002) | (ctl > 0.2)).all(), ctl
        assert upd[n_ctl:].max() > 0, "no stereo update in the free calls"
        assert max(bb.list_rounds(v, B) for v in n) >= (3 if B > 2049 else 2)
    assert seen == set(bb.CLASSES)


def test_the_oracle_reaches_the_classes_with_per_sequence_cameras():
    B, M = CASES[0]
    counts = bb.skewed_counts(B, M)
    cams = [tl.K640, tl.K_ANISO, tl.K_OFFCENTRE, tl.K_SKEW]
    flags, tn, _, n_ctl = _oracle_flags(192, 144, counts, Ks=[cams[m % 4] for m in range(M)])
    n, cls = bb.classes_of(flags, counts)
    assert {"0", "1..1023", "1024", "1025..2048"} <= cls, n
    ctl = tn[1:n_ctl]
    assert ((ctl < 0.002) | (ctl > 0.2)).all(), ctl


@pytest.mark.parametrize("B,M", CASES)
def test_sensor_schedule_reaches_every_list_length(B, M):
    counts = bb.skewed_counts(B, M)
    act, listed = bb.sensor_schedule(counts)
    want = {0, 1, 1023, 1024, 1025, B} | ({2049} if B >= 2600 else set())
    assert want <= set(listed), listed
    restarts = [int(((act[k] == 2) * np.asarray(counts)).sum()) for k in range(len(listed))]
    by_rule = [n - r for n, r in zip(listed[1:], restarts[1:])]
    assert max(by_rule) > 1024 and min(by_rule) == 0, by_rule        # promotions by the rule: a strided round of their own
    assert restarts[1:] == [r if r in want else 0 for r in bb.SENSOR_RESTARTS[1:]]
