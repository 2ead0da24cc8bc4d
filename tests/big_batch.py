"""Batches above 1024 sequences built by replication (tests/test_gpu_batch_over_1024.py).

Sequences of a batch are independent, so a batch of B sequences in which sequence q is fed what base sequence base[q] of an M-sequence
batch is fed must return base[q]'s bits for q.  This module holds what does not need a GPU: the replication table (a fixed-seed
permutation with different bases on both sides of 1024, 2048 and 32 768), the sample, the replication counts whose subset sums reach
the list lengths and keyframe-count classes the tests drive, the mono frame schedule that produces those classes by the keyframe rule
alone, and the sizes of the paths that change above 1024 (rounds of a list slot, sequences per thread of k_points_scan, grid z).
Test infrastructure only."""
import itertools

import numpy as np

LIST_SLOTS = 1024          # DVO_LIST_SLOTS (dvo_map_kernels.hip): sequence slots of a launch that works through need_list
SCAN_THREADS = 1024        # k_points_scan: one workgroup, ceil(n_seq / 1024) consecutive sequences per thread
GRID_SEQ_Y = 32768         # DVO_GRID_SEQ_Y (dvo_kernels.h): seq = blockIdx.z * 32768 + blockIdx.y
BOUNDARIES = (1024, 2048, 32768)
MUST_SAMPLE = (0, 1023, 1024, 1025, 2047, 2048)
KEY_FRAMES = 6             # needNewFrame's frame-count rule (mapper.cpp:45-60): a keyframe once id - ref_id >= 6
N_RENDER = 6               # frames of tests/test_gpu_mono_lockstep.py's render
CLASSES = ("0", "1..1023", "1024", "1025..2048", ">2048")


def list_rounds(n_listed, n_seq):
    """rounds the busiest slot of a listed launch walks: entries j, j + n_slots, ... with n_slots = min(n_seq, 1024)"""
    n_slots = min(n_seq, LIST_SLOTS)
    return -(-n_listed // n_slots)


def scan_per(n_seq):
    """sequences per thread of k_points_scan"""
    return -(-n_seq // SCAN_THREADS)


def grid_z(n_seq):
    """seq_grid()'s z extent"""
    gy = min(max(n_seq, 1), GRID_SEQ_Y)
    return -(-n_seq // gy)


def key_class(n):
    """the class of a call in which n sequences created a keyframe"""
    if n == 0:
        return "0"
    if n < 1024:
        return "1..1023"
    if n == 1024:
        return "1024"
    return "1025..2048" if n <= 2048 else ">2048"


def split_even(total, parts):
    return [total // parts + (1 if i < total % parts else 0) for i in range(parts)]


def skewed_counts(B, M):
    """Replication counts (M of them, every base at least once, sum B) whose subset sums reach 1, 1023, 1024, 1025 and, where B allows,
    2049: [1, 1, 1, 1022, 1024, the rest split evenly] from B = 2049 + (M - 5) on; below that M - 1 single replicas and one big base."""
    if M >= 6 and B >= 2049 + (M - 5):
        c = [1, 1, 1, 1022, 1024] + split_even(B - 2049, M - 5)
    else:
        big = B - (M - 1)
        if not (1025 <= B and 0 <= 1023 - big <= M - 1):
            raise ValueError("skewed_counts: no table for B = %d, M = %d" % (B, M))
        c = [1] * (M - 1) + [big]
    assert sum(c) == B and min(c) >= 1 and len(c) == M
    return c


def subset_with_sum(counts, target):
    """the bases of the smallest subset of `counts` that sums to `target` (lowest indices first among equals); ValueError if none"""
    M = len(counts)
    if target == 0:
        return []
    for r in range(1, M + 1):
        for sub in itertools.combinations(range(M), r):
            if sum(counts[i] for i in sub) == target:
                return list(sub)
    raise ValueError("no subset of %s sums to %d" % (counts, target))


def replicate(B, counts, seed=1024, pinned=None):
    """base [B] (int64): counts[m] replicas of base m at the places of a fixed-seed permutation.  pinned: {base: indices} puts every
    replica of those bases at exactly these indices (the others never go there).  The two sides of every boundary below B hold
    different bases (a boundary pair that the permutation made equal is mended by a swap with the nearest index that is
    neither pinned nor beside a boundary)."""
    counts = list(counts)
    pinned = {int(m): np.asarray(ix, np.int64) for m, ix in (pinned or {}).items()}
    assert sum(counts) == B and min(counts) >= 1
    base = np.full(B, -1, np.int64)
    for m, ix in pinned.items():
        assert len(ix) == counts[m] and len(set(ix.tolist())) == len(ix) and ix.min() >= 0 and ix.max() < B
        assert (base[ix] == -1).all()
        base[ix] = m
    free = np.nonzero(base < 0)[0]
    pool = np.repeat([m for m in range(len(counts)) if m not in pinned], [counts[m] for m in range(len(counts)) if m not in pinned])
    assert len(pool) == len(free)
    base[free] = np.random.RandomState(seed).permutation(pool)
    is_pinned = np.zeros(B, bool)
    for ix in pinned.values():
        is_pinned[ix] = True
    edge = set()
    for b in BOUNDARIES:
        edge.update((b - 1, b))
    for b in BOUNDARIES:
        if b >= B or base[b - 1] != base[b]:
            continue
        for j in sorted(range(B), key=lambda j: (abs(j - b), j)):
            if j in edge or is_pinned[j] or is_pinned[b] or base[j] == base[b - 1]:
                continue
            base[b], base[j] = base[j], base[b]
            break
    check_replication(base, counts)
    return base


def check_replication(base, counts):
    B = len(base)
    assert np.bincount(base, minlength=len(counts)).tolist() == list(counts)
    for b in BOUNDARIES:
        if b < B:
            assert base[b - 1] != base[b], "both sides of index %d hold base %d" % (b, base[b])


def neighbour_mix(base):
    """share of neighbouring pairs (q, q + 1) with different bases"""
    base = np.asarray(base)
    return float((base[1:] != base[:-1]).mean())


def sample(base, n=32, seed=7):
    """Sorted indices: 0, 1023, 1024, 1025, 2047, 2048 (those below B), B - 1, one replica of every base from 1024..2047 and one from
    2048..3071 where the base has one there (the list's second and third round when the list holds every sequence in order), one
    replica of every base anywhere, one on each side of 32 768, then a fixed-seed fill up to at least n."""
    base = np.asarray(base)
    B = len(base)
    out = {q for q in MUST_SAMPLE if q < B}
    out.add(B - 1)
    for lo in (0, LIST_SLOTS, 2 * LIST_SLOTS, GRID_SEQ_Y):
        hi = B if lo in (0, GRID_SEQ_Y) else min(B, lo + LIST_SLOTS)
        for m in np.unique(base):
            ix = np.nonzero(base[lo:hi] == m)[0]
            if len(ix) and not any(base[q] == m and lo <= q < hi for q in out):
                out.add(int(lo + ix[len(ix) // 2]))
    for b in BOUNDARIES:
        if b < B:
            out.update((b - 1, b))
    rest = np.setdiff1d(np.arange(B), np.fromiter(out, np.int64))
    if len(out) < n and len(rest):
        out.update(int(q) for q in np.random.RandomState(seed).choice(rest, min(n - len(out), len(rest)), replace=False))
    return sorted(out)


def rounds_covered(base, sample_ix):
    """{round: bases with a sampled replica at an index of that list round}, rounds 1 and 2 (the second and third)"""
    base = np.asarray(base)
    return {r: {int(base[q]) for q in sample_ix if r * LIST_SLOTS <= q < (r + 1) * LIST_SLOTS} for r in (1, 2)}


# ---- the mono schedule: keyframe-count classes by the keyframe rule alone ------------------------------------------------------------
# A sequence that sees its keyframe's frame again tracks a zero twist: no keyframe until the frame-count rule fires, KEY_FRAMES calls
# after its last keyframe.  A sequence that jumps three renders ahead tracks a translation far above 0.02 at these sizes (tests/
# test_big_batch.py measures the margin on the oracle): a keyframe.  So "who moves when" sets the number of keyframes of every call:
#   call 0              every sequence starts                                  (not counted)
#   call 1              nobody moves                                           0
#   call 2              base 0 (one replica) jumps                             1
#   call 6              everybody else's frame-count rule fires                B - 1      (1024 at B = 1025, above 2048 at B = 2600)
#   call 7              B = 2600: the subset that sums to 1024 jumps           1024       (B = 1025: nobody moves, 0)
#   call 8              base 0's frame-count rule fires (call 2 + 6) and       1025..2048
#                       B = 1025: everybody else jumps (1025); B = 2600: a subset that sums to 1133 jumps (1134)
#   calls 9 ..          every base steps one render per call (small baselines: stereo updates; whatever keyframes the rule gives)
FREE_CALLS = 3


def mono_moves(counts):
    """{call: bases that jump}, and the number of controlled calls"""
    B = sum(counts)
    moves = {2: [0]}
    if B - 1 == 1024:
        moves[KEY_FRAMES + 2] = list(range(1, len(counts)))
        n = KEY_FRAMES + 3
    else:
        moves[KEY_FRAMES + 1] = subset_with_sum(counts, 1024)
        rest = [m for m in range(1, len(counts)) if m not in moves[KEY_FRAMES + 1]]
        pick, tot = [], 0
        for m in sorted(rest, key=lambda m: -counts[m]):
            if tot < 1025:
                pick.append(m); tot += counts[m]
        assert 1025 <= tot + 1 <= 2048, tot          # (+ base 0, whose frame-count rule fires at call 8)
        moves[KEY_FRAMES + 2] = sorted(pick)
        n = KEY_FRAMES + 3
    return moves, n


def mono_orders(counts, free_calls=FREE_CALLS):
    """per base the render index at every call of the schedule above; (orders [M][n_calls], n_controlled)"""
    moves, n = mono_moves(counts)
    M = len(counts)
    orders = []
    for m in range(M):
        f, seq = m % N_RENDER, []
        for k in range(n):
            if m in moves.get(k, ()):
                f = (f + 3) % N_RENDER
            seq.append(f)
        for k in range(free_calls):
            f = (f + 1) % N_RENDER
            seq.append(f)
        orders.append(seq)
    return orders, n


def classes_of(key_flags, counts, first=1):
    """key_flags [n_calls][M] bool (per base) -> (the per-call number of keyframe-creating sequences from call `first` on, their classes)"""
    c = np.asarray(counts, np.int64)
    n = [int((np.asarray(k, bool) * c).sum()) for k in key_flags[first:]]
    return n, {key_class(v) for v in n}


# ---- the sensor-depth schedule: list lengths set exactly by RESTART actions, promotions by the frame-count rule between them -------
SENSOR_MAX_FRAMES = 4      # keyframe_max_frames of the schedule below (keyframe_min_translation 1.0: the frame-count rule alone)
SENSOR_RESTARTS = (None, 0, 1, 1023, 0, 1024, 1025, 2049, 0, 0, 0, 0)    # per push: None = every sequence starts; else the RESTART count


def sensor_schedule(counts, restarts=SENSOR_RESTARTS, max_frames=SENSOR_MAX_FRAMES, skip=0, track=1, restart=2):
    """(act uint8 [n_push][M], listed [n_push]): the per-base actions whose RESTART subset of every push sums to restarts[k] (the
    nearest reachable smaller target where B cannot reach it is NOT taken: an unreachable target becomes an all-TRACK push), and the
    number of sequences that enter need_list at every push -- the restarts plus the sequences whose frame-count rule fires
    (k - ref >= max_frames, ref = the push of the sequence's last keyframe), by the rule of k_kf_decide restated here."""
    M, B = len(counts), sum(counts)
    act = np.full((len(restarts), M), track, np.uint8)
    ref = np.zeros(M, np.int64)
    listed = []
    for k, r in enumerate(restarts):
        if r is None:
            ref[:] = k
            listed.append(B)
            continue
        sub = []
        if r:
            try:
                sub = subset_with_sum(counts, r)
            except ValueError:
                sub = []
        act[k, sub] = restart
        n = 0
        for m in range(M):
            if m in sub or k - ref[m] >= max_frames:
                ref[m] = k
                n += counts[m]
        listed.append(n)
    return act, listed
