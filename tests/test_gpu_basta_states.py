"""beagleBastaSampleStates on the device against its host restatement (tests/basta_states_reference.py) run on the vectors and
matrices read back from the device: the states bit for bit, the two count arrays exactly."""
import ctypes as C
import os

import numpy as np
import pytest

import basta_states_cases as cases
import basta_states_reference as sr
import beast_mcmc_amd as bm
from beast_mcmc_amd import basta
from beast_mcmc_amd.inputs import substmodel

pytestmark = pytest.mark.gpu
Beagle, BeagleException, FLAG_EIGEN_COMPLEX = bm.beagle.Beagle, bm.beagle.BeagleException, bm.beagle.FLAG_EIGEN_COMPLEX


class Case:
    """A BASTA instance after one evaluation, with what the restatement needs read back from it (once)."""

    def __init__(self, state_count, tip_count, kind="distinct", tips="ambiguous", seed=None, symmetric=False):
        x = self.x = cases.Inputs(state_count, tip_count, kind=kind, seed=state_count + tip_count if seed is None else seed, tips=tips,
                                  symmetric=symmetric)
        w, v = np.linalg.eig(x.q)
        eig = basta.transpose_eigen(substmodel.EigenDecomposition(np.real(v), np.real(np.linalg.inv(v)), np.real(w)))
        self.like = basta.BastaLikelihood(x.tree, x.tips, eig, x.sizes, rate=cases.RATE, sub_intervals=x.sub)
        self.logl = self.like.log_likelihood(matrices=x.matrices)
        self.tr = self.like.traversal
        self.read_back()

    def read_back(self):
        b, s = self.like.beagle, self.x.state_count
        self.buffers = b.bastaStats()[3]
        self.vectors = np.stack([b.getPartials(i).reshape(s) for i in range(self.buffers)])
        self.matrices = {m: b.getTransitionMatrix(m).reshape(s, s) for m, _ in self.tr.matrices}

    def device(self, replicates, seed, **kw):
        return self.like.sample_states(replicates, seed, root_frequencies=self.x.frequencies, **kw)

    def host(self, replicates, seed, use_map=False, as_written=False):
        tr = self.tr
        return sr.sample(tr.operations, tr.intervals, self.vectors, lambda m: self.matrices[m], self.x.frequencies, replicates, seed,
                         use_map=use_map, as_written=as_written)

    def close(self):
        self.like.close()


ALL = [(r, w, m) for r in (1, 3, 130) for w in (False, True) for m in (False, True)]
SOME = [(130, False, False), (3, True, False), (1, False, True), (130, True, True)]
# 61: the largest state count whose matrix goes through LDS, 65 the first that does not; 2 / 4, 12, 20 / 32: the three register counts of
# the kernel that asks for a step's matrix a step ahead, 33: the first state count it does not take; the ladder: the most launches
CASES = [(2, 5, "distinct", ALL), (4, 5, "distinct", ALL), (20, 5, "distinct", ALL), (61, 5, "distinct", ALL), (65, 5, "distinct", ALL),
         (12, 5, "distinct", SOME), (32, 5, "distinct", SOME), (33, 5, "distinct", SOME),
         (4, 12, "ladder", ALL), (61, 12, "ladder", SOME), (65, 12, "ladder", SOME), (4, 51, "distinct", SOME), (20, 51, "distinct", SOME)]


@pytest.mark.parametrize("state_count,tip_count,kind,combos", CASES)
def test_states_and_counts_are_the_restatements(state_count, tip_count, kind, combos):
    case = Case(state_count, tip_count, kind)
    try:
        for replicates, as_written, use_map in combos:
            seed = 1000 * replicates + 10 * as_written + use_map
            got = case.device(replicates, seed, map=use_map, as_written=as_written, occupancy=True, changes=True)
            states, occupancy, changes, bad = case.host(replicates, seed, use_map, as_written)
            differ = int(np.count_nonzero(got["states"] != states))
            print("S=%d T=%d %s R=%d as_written=%d map=%d: %d of %d states differ, launches %d" % (
                state_count, tip_count, kind, replicates, as_written, use_map, differ, states.size, case.like.beagle.bastaStatesStats()[1]))
            assert not bad and not got["bad"]
            assert got["states"].shape == states.shape and differ == 0
            assert np.array_equal(got["occupancy"], occupancy.astype(np.float64))
            assert np.array_equal(got["changes"], changes.astype(np.float64))
    finally:
        case.close()


def test_counts_alone_repeats_chunks_and_a_new_update():
    case = Case(4, 51, "distinct")
    try:
        b = case.like.beagle
        first = case.device(130, 42, occupancy=True, changes=True)
        # without outStates: the same two arrays; the second call: the same bytes
        counts = case.device(130, 42, states=False, occupancy=True, changes=True)
        assert "states" not in counts
        again = case.device(130, 42, occupancy=True, changes=True)
        for key in ("occupancy", "changes"):
            assert np.array_equal(first[key], counts[key]) and np.array_equal(first[key], again[key])
        assert first["states"].tobytes() == again["states"].tobytes()
        only = case.device(130, 42)
        assert only["states"].tobytes() == first["states"].tobytes() and "occupancy" not in only
        # cut into chunks of 64 replicates: the same bytes
        assert b.bastaStatesStats()[2] == 1
        os.environ["BEAGLE_MI355_BASTA_STATES_CHUNK"] = "64"
        try:
            cut = case.device(130, 42, occupancy=True, changes=True)
        finally:
            del os.environ["BEAGLE_MI355_BASTA_STATES_CHUNK"]
        assert b.bastaStatesStats()[2] == 3
        assert cut["states"].tobytes() == first["states"].tobytes()
        assert np.array_equal(cut["occupancy"], first["occupancy"]) and np.array_equal(cut["changes"], first["changes"])
        # the list was sent once, by the update
        assert b.bastaStats()[0] == 1
        # the likelihood is untouched by the draws
        tr = case.tr
        out = np.zeros(1)
        b.accumulateBastaPartials(tr.operations, len(tr.operations), tr.intervals, len(tr.intervals), tr.lengths, case.like.sizes_index, 0, out)
        assert out[0] == case.logl
        # other branch lengths: another draw, still the restatement's
        longer = {m: x @ x for m, x in case.x.matrices.items()}
        assert case.like.log_likelihood(matrices=longer) != case.logl
        case.read_back()
        changed = case.device(130, 42, occupancy=True, changes=True)
        assert changed["states"].tobytes() != first["states"].tobytes()
        states, occupancy, changes, _ = case.host(130, 42)
        assert np.array_equal(changed["states"], states)
        assert np.array_equal(changed["occupancy"], occupancy.astype(np.float64)) and np.array_equal(changed["changes"], changes.astype(np.float64))
    finally:
        case.close()


@pytest.mark.parametrize("state_count,tip_count,kind", [(4, 12, "ladder"), (4, 51, "distinct"), (65, 12, "ladder")])
def test_the_launch_count_is_the_depth_in_coalescences(state_count, tip_count, kind):
    case = Case(state_count, tip_count, kind)
    try:
        b = case.like.beagle
        b.kernelTimer(1)
        case.device(3, 1)
        ms, launches = b.kernelTimer(0)
        calls, per_chunk, chunks, chains = b.bastaStatesStats()
        depth = sr.coalescence_depth(case.tr.operations)
        print("T=%d %s: %d launches (%.3f ms), depth %d, %d chains" % (tip_count, kind, launches, ms, depth, chains))
        assert per_chunk == launches == depth and chunks == 1 and calls == 1
        if kind == "ladder":
            assert depth == tip_count - 1
        assert chains == 2 * (tip_count - 1)
    finally:
        case.close()


def test_error_returns():
    lib = bm.beagle.engine().lib
    I, D = C.POINTER(C.c_int), C.POINTER(C.c_double)
    f = lib.beagleBastaSampleStates
    f.argtypes = [C.c_int, I, C.c_int, I, C.c_int, C.c_int, C.c_int, C.c_ulonglong, C.c_int, C.c_void_p, D, D]
    f.restype = C.c_int

    def run(h, ops, intervals, replicates=2, flags=0, frequencies_index=1, buffers=8, states=True, changes=True):
        o = np.ascontiguousarray(ops, dtype=np.int32).reshape(-1)
        iv = np.ascontiguousarray(intervals, dtype=np.int32)
        out = np.full((max(replicates, 1), buffers), 77, dtype=np.uint8)
        ch = np.zeros((3, 3))
        rc = f(h, o.ctypes.data_as(I), len(o) // 8, iv.ctypes.data_as(I), len(iv), frequencies_index, replicates, 5, flags,
               out.ctypes.data if states else None, None, ch.ctypes.data_as(D) if changes else None)
        return rc, out, ch

    good = [[2, 0, 0, -1, -1, 2, -1, 0], [3, 2, 1, 1, 1, 4, 5, 1]]
    b = Beagle(0, 8, 0, 3, 1, 2, 4, 1, 1, requirementFlags=FLAG_EIGEN_COMPLEX)
    plain = Beagle(0, 8, 0, 3, 5, 2, 4, 1, 1)                  # an ordinary instance
    one = Beagle(0, 8, 0, 3, 1, 2, 4, 1, 1)                    # one pattern, one category, but no BASTA buffers
    gpus = len(bm.beagle.engine().resource_list()) - 2
    sharded = Beagle(0, 8, 0, 3, 1, 2, 4, 1, 1, resourceList=(gpus + 1,))
    try:
        h = b.instance
        assert run(h, good, [0, 1, 2])[0] == -7                # before AllocateCoalescentBuffers
        assert run(plain.instance, good, [0, 1, 2])[0] == -7 and run(one.instance, good, [0, 1, 2])[0] == -7
        assert run(sharded.instance, good, [0, 1, 2])[0] == -7
        b.allocateCoalescentBuffers(5, 4, 8, 1)
        vectors = np.array([[0.2, 0.3, 0.5], [0.6, 0.0, 0.4]])
        for i in range(2):
            b.setPartials(i, vectors[i])
        b.setStateFrequencies(0, [1.0, 2.0, 3.0])
        b.setStateFrequencies(1, [0.2, 0.5, 0.3])
        matrices = np.random.default_rng(3).dirichlet(np.ones(3), size=(2, 3))
        for m in range(2):
            b.setTransitionMatrix(m, matrices[m])
        b.updateBastaPartials(np.array(good, dtype=np.int32), 2, np.array([0, 1, 2], dtype=np.int32), 3, 0, 0)
        rc, states, changes = run(h, good, [0, 1, 2])
        assert rc == 0 and np.all(states[:, :6] < 3) and np.all(states[:, 6:] == 255) and changes.sum() == 2 * 3
        # out of range
        assert run(h, good, [0, 1, 2], replicates=0)[0] == -5 and run(h, good, [0, 1, 2], replicates=-3)[0] == -5
        assert run(h, good, [0, 1, 2], flags=4)[0] == -5 and run(h, good, [0, 1, 2], frequencies_index=2)[0] == -5
        assert run(h, good, [0, 1, 2], states=False, changes=False)[0] == -5
        assert run(h, good, [0, 2, 1])[0] == -5
        for at, value in ((0, 8), (1, -1), (2, 4), (13, 8), (11, 8)):
            ops = np.array(good).reshape(-1)
            ops[at] = value
            assert run(h, ops, [0, 1, 2])[0] == -5, (at, value)
        # not the forest: a vector read twice (a stored one, then a produced one), one written twice, one read where it is written
        assert run(h, [[2, 0, 0, -1, -1, 2, -1, 0], [3, 2, 1, 0, 1, 4, 5, 1]], [0, 1, 2])[0] == -7
        assert run(h, [[2, 0, 0, -1, -1, 2, -1, 0], [3, 2, 1, -1, -1, 3, -1, 1], [4, 2, 1, 1, 1, 5, 6, 1]], [0, 1, 3])[0] == -7
        assert run(h, [[2, 0, 0, -1, -1, 2, -1, 0], [2, 1, 1, -1, -1, 2, -1, 1]], [0, 1, 2])[0] == -7
        assert run(h, [[2, 0, 0, -1, -1, 2, -1, 0], [3, 2, 1, 1, 1, 4, 5, 0]], [0, 2, 2])[0] == -7
        assert run(h, good, [0, 1, 2])[0] == 0                 # (and the good list still runs after them)
        # a zero vector: -8, state 0 there, the other states as without it
        _, before, _ = run(h, good, [0, 1, 2], replicates=7)
        b.setPartials(1, [0.0, 0.0, 0.0])
        rc, after, _ = run(h, good, [0, 1, 2], replicates=7)
        assert rc == -8
        assert np.all(after[:, 1] == 0) and np.all(after[:, 5] == 0)
        keep = [0, 2, 3, 4, 6, 7]
        assert np.array_equal(after[:, keep], before[:, keep])
        with pytest.raises(BeagleException):
            b.sampleBastaStates(np.array(good, dtype=np.int32), 2, np.array([0, 1, 2], dtype=np.int32), 3, 1, 0, 5)
    finally:
        b.finalize(); plain.finalize(); one.finalize(); sharded.finalize()
