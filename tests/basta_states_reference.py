"""Host restatement of beagleBastaSampleStates (include/beagle_mi355.h), vectorised over replicates.

It restates BastaLikelihood.traverseSampleByCoalescentIntervals (src/dr/evomodel/coalescent/basta/BastaLikelihood.java:755-943):
the root from p f (:889-909), then every operation from the last interval to the first, each input from the matrix row its `dest`
state selects times the input's vector (:911-943), a vector with one positive entry without a draw (:846-867) — with the engine's
stateless random numbers and drawChoice (tests/ancestral_reference.py).  It is written from the vectors and matrices alone, so it
runs on the host restatement of the likelihood (tests/basta_reference.py) as well as on what an engine reads back.  Every product,
sum and difference is one IEEE double operation in the order the kernel forms it, so the states must agree bit for bit.
"""
import numpy as np

import ancestral_reference as ar

AS_WRITTEN = 2


def mix64(state, key):
    """The (key + 1)-th SplitMix64 output from `state`, elementwise (either may be an array; uint64 arithmetic modulo 2^64)."""
    state = np.asarray(state, dtype=np.uint64)
    key = np.asarray(key, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = state + (key + np.uint64(1)) * np.uint64(ar.GOLDEN)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(ar.MIX1)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(ar.MIX2)
        z = z ^ (z >> np.uint64(31))
    return z


def uniforms(seed, replicates, buffer):
    """u[r] of vector `buffer`: ancestralUniform(mix64(seed, r), buffer)"""
    streams = mix64(np.uint64(seed & 0xFFFFFFFFFFFFFFFF), replicates)
    return (mix64(streams, buffer) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def interval_of(intervals, n):
    """per operation, the interval (index into the offsets) it belongs to"""
    return np.searchsorted(np.asarray(intervals), np.arange(n), side="right") - 1


def weights(matrix, s, p, as_written):
    """[replicate][j]: M[s][j] p_j (default) or M[j][s] p_j (as written), s per replicate"""
    rows = matrix[:, s].T if as_written else matrix[s, :]
    return rows * p[None, :]


def sample(ops, intervals, partials, matrix_of, frequencies, replicates, seed, use_map=False, as_written=False, first_replicate=0):
    """partials: [buffer][S] as stored after the update; matrix_of(m) -> [S][S] as getTransitionMatrix returns it.
    -> (states uint8 [replicates][buffer], occupancy int64 [intervals][S], changes int64 [S][S], any_bad)"""
    ops = np.asarray(ops, dtype=np.int64).reshape(-1, 8)
    partials = np.asarray(partials, dtype=np.float64)
    frequencies = np.asarray(frequencies, dtype=np.float64)
    n, (V, S) = len(ops), partials.shape
    reps = np.arange(first_replicate, first_replicate + replicates, dtype=np.uint64)
    states = np.full((replicates, V), 255, dtype=np.uint8)
    occupancy = np.zeros((len(intervals) - 1, S), dtype=np.int64)
    changes = np.zeros((S, S), dtype=np.int64)
    where = interval_of(intervals, n)
    any_bad = False
    for k in range(n - 1, -1, -1):
        dest, in1, m1, in2, m2, acc1, acc2, _ = (int(x) for x in ops[k])
        if states[0, dest] == 255:                           # nothing read it: a root
            p = partials[dest]
            drawn, bad = ar.draw_choice([np.full(replicates, p[i] * frequencies[i]) for i in range(S)], uniforms(seed, reps, dest), use_map)
            any_bad |= bool(bad.any())
            states[:, dest] = drawn
        s = states[:, dest].astype(np.int64)
        for inp, m, acc in ((in1, m1, acc1), (in2, m2, acc2)):
            if inp < 0:
                continue
            p = partials[inp]
            if np.count_nonzero(p > 0.0) == 1:
                t = np.full(replicates, int(np.argmax(p > 0.0)), dtype=np.int64)
            else:
                w = weights(matrix_of(m), s, p, as_written)
                t, bad = ar.draw_choice([w[:, j] for j in range(S)], uniforms(seed, reps, inp), use_map)
                any_bad |= bool(bad.any())
            states[:, inp] = t
            if in2 >= 0:
                states[:, acc] = t
            occupancy[where[k]] += np.bincount(t, minlength=S)
            np.add.at(changes, (s, t), 1)
    return states, occupancy, changes, any_bad


def counts_from_states(ops, intervals, states, state_count):
    """occupancy and changes recomputed from the states alone"""
    ops = np.asarray(ops, dtype=np.int64).reshape(-1, 8)
    where = interval_of(intervals, len(ops))
    occupancy = np.zeros((len(intervals) - 1, state_count), dtype=np.int64)
    changes = np.zeros((state_count, state_count), dtype=np.int64)
    for k, op in enumerate(ops):
        s = states[:, op[0]].astype(np.int64)
        for inp in (op[1], op[3]):
            if inp >= 0:
                t = states[:, inp].astype(np.int64)
                occupancy[where[k]] += np.bincount(t, minlength=state_count)
                np.add.at(changes, (s, t), 1)
    return occupancy, changes


def coalescence_depth(ops):
    """The largest number of two-input operations on a path from a root of the list down (a root that is no coalescence counting as
    one): the launches of one chunk."""
    ops = np.asarray(ops, dtype=np.int64).reshape(-1, 8)
    above = {}                                               # buffer -> coalescences at or above the operation that reads it
    depth = 0
    for op in ops[::-1]:
        root = int(op[0]) not in above
        d = above.get(int(op[0]), 0) + (1 if op[3] >= 0 or root else 0)
        depth = max(depth, d)
        above[int(op[1])] = d
        if op[3] >= 0:
            above[int(op[3])] = d
    return depth
