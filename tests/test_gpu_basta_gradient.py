"""beagleBastaGradient on the device against its host restatement (tests/basta_gradient_reference.py adjoint) run on the vectors,
matrices and coalescent probabilities read back from the device: the adjoints and both gradients bit for bit; one larger case against
finite differences of the likelihood restatement in numpy.longdouble."""
import ctypes as C

import numpy as np
import pytest

import basta_gradient_reference as gr
import basta_states_cases as cases
import basta_states_reference as sr
import beast_mcmc_amd as bm
from beast_mcmc_amd import basta
from beast_mcmc_amd.inputs import substmodel

pytestmark = pytest.mark.gpu
Beagle, BeagleException, FLAG_EIGEN_COMPLEX = bm.beagle.Beagle, bm.beagle.BeagleException, bm.beagle.FLAG_EIGEN_COMPLEX


class Case:
    """A BASTA instance after one evaluation (matrices from the eigen system on the device, or uploaded), with what the restatement
    needs read back from it."""

    def __init__(self, state_count, tip_count, kind="distinct", tips="one-hot", sub=1, upload=False, seed=None, tree=None):
        x = self.x = cases.Inputs(state_count, tip_count, kind=kind, seed=state_count + tip_count if seed is None else seed, tips=tips,
                                  sub_intervals=sub)
        if tree is not None:
            x.tree = tree
        _, eig = substmodel.decompose_complex(x.q)
        self.upload = upload
        self.like = basta.BastaLikelihood(x.tree, x.tips, basta.transpose_eigen(eig), x.sizes, rate=cases.RATE, sub_intervals=sub)
        self.evaluate()

    def evaluate(self):
        """(the uploaded matrices are those of the inputs' own traversal: after a branch move they are merely other matrices)"""
        self.logl = self.like.log_likelihood(matrices=self.x.matrices if self.upload else None)
        self.tr = self.like.traversal
        self.read_back()

    def read_back(self):
        b, s = self.like.beagle, self.x.state_count
        self.buffers = b.bastaStats()[3]
        self.vectors = np.stack([b.getPartials(i).reshape(s) for i in range(self.buffers)])
        self.matrices = {m: b.getTransitionMatrix(m).reshape(s, s) for m, _ in self.tr.matrices}
        self.coalescent = b.getBastaBuffer(0)

    def device(self, **kw):
        return self.like.gradient(adjoints=True, **kw)

    def host(self, dtype=np.float64):
        tr = self.tr
        return gr.adjoint(tr.operations, tr.intervals, tr.lengths, basta.interval_distances(tr), self.vectors, self.matrices,
                          self.like.sizes, self.coalescent, dtype=dtype)

    def close(self):
        self.like.close()


def same(got, want):
    """the adjoints and both gradients, bit for bit"""
    for key in ("adjoints", "theta", "migration"):
        a, b = np.asarray(got[key]), np.asarray(want[key])
        if key == "adjoints" and a.shape[0] != b.shape[0]:  # (an instance that has grown holds more buffers: untouched, so zero)
            rows = min(a.shape[0], b.shape[0])
            assert not np.any(a[rows:]) and not np.any(b[rows:])
            a, b = np.ascontiguousarray(a[:rows]), np.ascontiguousarray(b[:rows])
        assert a.shape == b.shape, key
        differ = int(np.count_nonzero(a.view(np.uint64) != b.view(np.uint64)))
        zeros = differ and np.array_equal(a, b)             # (only the sign of a zero)
        assert differ == 0 or zeros, "%s: %d of %d values differ, worst %.3e" % (key, differ, a.size, float(np.abs(a - b).max()))


def check(case, label=""):
    """-> the fp64 restatement's own error against numpy.longdouble, relative to the largest entry (W, G_theta)"""
    got, want = case.device(), case.host()
    assert not got["bad"]
    assert np.abs(got["migration"]).max() > 0.0 and np.abs(got["theta"]).max() > 0.0 and np.abs(got["adjoints"]).max() > 0.0
    wide = case.host(np.longdouble)
    own = [float(np.abs(want[k] - wide[k]).max() / np.abs(wide[k]).max()) for k in ("migration", "theta")]
    dev = [float(np.abs(got[k] - wide[k]).max() / np.abs(wide[k]).max()) for k in ("migration", "theta")]
    print("%s: fp64 restatement vs longdouble W %.2e G %.2e; device W %.2e G %.2e; launches %d" % (
        label, own[0], own[1], dev[0], dev[1], case.like.beagle.bastaGradientStats()[1]))
    same(got, want)
    return own


# 8 / 9: one load of the matrix or more; 32 / 33, 64 / 65: the state counts at which the likelihood and the sampler change kernels
# (64 / 65 is also where a lane starts to carry more than one state); 61: the deme count of the bench
@pytest.mark.parametrize("sub", [1, 3])
@pytest.mark.parametrize("state_count", [2, 4, 8, 9, 20, 32, 33, 61, 64, 65])
def test_adjoints_and_gradients_are_the_restatements(state_count, sub):
    """The host mirrors both reductions' order, so W and G_theta are asserted EQUAL to the fp64 restatement, not within a multiple of
    its error: the device's error against numpy.longdouble is the restatement's own, ratio 1 (measured: W up to 1.1e-15, G_theta up to
    5.7e-16 of the largest entry over these cases; each case prints its own)."""
    case = Case(state_count, 12, sub=sub)
    try:
        check(case, "S=%d sub=%d" % (state_count, sub))
    finally:
        case.close()


@pytest.mark.parametrize("tip_count,kind,tips,upload", [(9, "ladder", "one-hot", False), (2, "distinct", "one-hot", False),
                                                        (12, "distinct", "ambiguous", False), (12, "distinct", "one-hot", True)])
def test_four_states_ladder_two_tips_ambiguous_tips_and_uploaded_matrices(tip_count, kind, tips, upload):
    case = Case(4, tip_count, kind=kind, tips=tips, upload=upload)
    try:
        check(case, "T=%d %s %s upload=%d" % (tip_count, kind, tips, upload))
        calls, launches, levels, chains = case.like.beagle.bastaGradientStats()
        assert levels == sr.coalescence_depth(case.tr.operations) and chains == 2 * (tip_count - 1)
        if kind == "ladder":
            assert levels == tip_count - 1
    finally:
        case.close()


def test_repeats_list_handling_and_what_the_call_leaves_alone():
    case = Case(4, 12, tips="ambiguous", sub=3)
    fresh = None
    try:
        b, tr = case.like.beagle, case.tr
        n, m = len(tr.operations), len(tr.intervals)
        uploads = b.bastaStats()[0]
        efgh = [b.getBastaBuffer(i) for i in range(1, 5)]
        drawn = case.like.sample_states(5, 7, occupancy=True, changes=True)
        b.kernelTimer(1)
        first = case.device()
        ms, timed = b.kernelTimer(0)
        again = case.device()
        same(first, again)
        same(first, case.host())
        # the list was sent once, by the update; launches = levels + (e-h, their total, the two reductions)
        assert b.bastaStats()[0] == uploads == 1
        calls, launches, levels, chains = b.bastaGradientStats()
        assert calls == 2 and launches == levels + 4 == timed and levels == sr.coalescence_depth(tr.operations)
        # e, f, g, h, the draws and the likelihood: the same bits after the call
        for i in range(4):
            assert np.array_equal(b.getBastaBuffer(i + 1), efgh[i])
        after = case.like.sample_states(5, 7, occupancy=True, changes=True)
        for key in ("states", "occupancy", "changes"):
            assert np.array_equal(drawn[key], after[key])
        out = np.zeros(1)
        b.accumulateBastaPartials(tr.operations, n, tr.intervals, m, tr.lengths, case.like.sizes_index, 0, out)
        assert out[0] == case.logl
        assert case.like.log_likelihood() == case.logl
        same(case.device(), first)
        # one output at a time: the same bits; without distances only when W is not asked for
        only = case.like.gradient(wrt="population")
        assert "migration" not in only and np.array_equal(only["theta"], first["theta"])
        only = case.like.gradient(wrt="migration", frequencies=case.x.frequencies)
        assert "theta" not in only and np.array_equal(only["migration"], first["migration"])
        assert np.array_equal(only["migration_rates"], basta.migration_rate_chain_rule(first["migration"], case.x.frequencies))
        assert np.array_equal(first["population_sizes"], -first["theta"] / case.like.sizes ** 2)
        # without beagleBastaAccumulatePartials before it: the call forms e, f, g, h itself
        bare = Case(4, 12, tips="ambiguous", sub=3)
        try:
            bb = bare.like.beagle
            bb.allocateCoalescentBuffers(basta.COALESCENT_BUFFER_COUNT, bare.like.max_intervals, bare.like.partials_count, 0)
            bb.updateBastaPartials(tr.operations, n, tr.intervals, m, bare.like.sizes_index, 0)
            assert not np.any(bb.getBastaBuffer(1))
            same(bare.device(), first)
            for i in range(4):
                assert np.array_equal(bb.getBastaBuffer(i + 1), efgh[i])
        finally:
            bare.close()
        # a branch move: a new list, and the numbers of an instance that never saw the old one
        tree = case.x.tree
        height = [float(v) for v in tree.height]
        for node in range(tree.tip_count, tree.node_count - 1):              # below an event that lay between it and its children
            low = max(height[int(tree.left[node])], height[int(tree.right[node])])
            between = [v for v in height if low < v < height[node]]
            if between:
                break
        old = tr.operations.copy()
        case.like.set_node_height(node, 0.5 * (low + min(between)))
        case.evaluate()
        assert case.tr.operations.shape != old.shape or not np.array_equal(case.tr.operations, old)
        assert b.bastaStats()[0] == 2
        after_move = case.device()
        assert not np.array_equal(after_move["migration"], first["migration"])
        same(after_move, case.host())
        fresh = Case(4, 12, tips="ambiguous", sub=3, tree=case.x.tree)
        same(fresh.device(), after_move)
        # other population sizes at the other index
        sizes = case.like.sizes * np.linspace(0.5, 1.5, 4)
        case.like.set_population_sizes(sizes, flip=True)
        assert case.like.sizes_index == 1
        case.evaluate()
        flipped = case.device()
        assert not np.array_equal(flipped["theta"], after_move["theta"])
        same(flipped, case.host())
        fresh.like.set_population_sizes(sizes)
        fresh.evaluate()
        same(fresh.device(), flipped)
    finally:
        case.close()
        if fresh is not None:
            fresh.close()


def test_two_hundred_tips_twenty_demes_against_finite_differences():
    """The device's W and G_theta along four random directions against central differences (eps 1e-6) of basta_reference's likelihood in
    numpy.longdouble, from the matrices read back: 1e-6 relative (measured: at most 6.4e-9)."""
    case = Case(20, 200, seed=11)
    try:
        got = case.device()
        assert not got["bad"]
        tr, x = case.tr, case.x
        rng = np.random.default_rng(5)
        distances = basta.interval_distances(tr)
        for k in range(4):
            dw, dt = rng.normal(size=(20, 20)), rng.normal(size=20) / case.like.sizes
            want = gr.directional_difference(x.tips, tr.operations, tr.intervals, tr.lengths, distances, case.matrices, case.like.sizes,
                                             tr.buffer_count, tr.interval_count, direction_w=dw, direction_theta=dt)
            have = np.sum(got["migration"].astype(np.longdouble) * dw) + np.sum(got["theta"].astype(np.longdouble) * dt)
            rel = float(abs(have - want) / abs(want))
            print("direction %d: device %.12e, differences %.12e, relative %.2e" % (k, float(have), float(want), rel))
            assert rel <= 1e-6
    finally:
        case.close()


def test_error_returns():
    lib = bm.beagle.engine().lib
    I, D = C.POINTER(C.c_int), C.POINTER(C.c_double)
    f = lib.beagleBastaGradient
    f.argtypes = [C.c_int, I, C.c_int, I, C.c_int, D, D, C.c_int, C.c_int, C.c_int, D, D, D]
    f.restype = C.c_int

    def run(h, ops, intervals, flags=0, sizes_index=0, coalescent_index=0, outputs=(True, True, True), distances=True, lengths=True,
            buffers=8):
        o = np.ascontiguousarray(ops, dtype=np.int32).reshape(-1)
        iv = np.ascontiguousarray(intervals, dtype=np.int32)
        ln, ds = np.array([0.3, 0.7, 0.2]), np.array([0.24, 0.56, 0.16])
        g, w, lam = np.full(3, 77.0), np.full((3, 3), 77.0), np.full((buffers, 3), 77.0)
        rc = f(h, o.ctypes.data_as(I), len(o) // 8, iv.ctypes.data_as(I), len(iv), ln.ctypes.data_as(D) if lengths else None,
               ds.ctypes.data_as(D) if distances else None, sizes_index, coalescent_index, flags,
               g.ctypes.data_as(D) if outputs[0] else None, w.ctypes.data_as(D) if outputs[1] else None,
               lam.ctypes.data_as(D) if outputs[2] else None)
        return rc, g, w, lam

    def untouched(result):
        return all(np.all(a == 77.0) for a in result[1:])

    good = [[2, 0, 0, -1, -1, 2, -1, 0], [3, 2, 1, 1, 1, 4, 5, 1]]
    b = Beagle(0, 8, 0, 3, 1, 2, 4, 1, 1, requirementFlags=FLAG_EIGEN_COMPLEX)
    plain = Beagle(0, 8, 0, 3, 5, 2, 4, 1, 1)                  # an ordinary instance
    one = Beagle(0, 8, 0, 3, 1, 2, 4, 1, 1)                    # one pattern, one category, but no BASTA buffers
    gpus = len(bm.beagle.engine().resource_list()) - 2
    sharded = Beagle(0, 8, 0, 3, 1, 2, 4, 1, 1, resourceList=(gpus + 1,))
    parted = Beagle(0, 8, 0, 3, 6, 2, 4, 1, 1)                 # two pattern partitions
    try:
        parted.setPatternPartitions(2, [0, 0, 0, 1, 1, 1])
        h = b.instance
        assert run(h, good, [0, 1, 2])[0] == -7                # before AllocateCoalescentBuffers
        assert run(plain.instance, good, [0, 1, 2])[0] == -7 and run(one.instance, good, [0, 1, 2])[0] == -7
        assert run(sharded.instance, good, [0, 1, 2])[0] == -7 and run(parted.instance, good, [0, 1, 2])[0] == -7
        b.allocateCoalescentBuffers(5, 4, 8, 1)
        vectors = np.array([[0.2, 0.3, 0.5], [0.6, 0.0, 0.4]])
        for i in range(2):
            b.setPartials(i, vectors[i])
        b.setStateFrequencies(0, [1.0, 2.0, 3.0])
        matrices = np.random.default_rng(3).dirichlet(np.ones(3), size=(2, 3))
        for m in range(2):
            b.setTransitionMatrix(m, matrices[m])
        b.updateBastaPartials(np.array(good, dtype=np.int32), 2, np.array([0, 1, 2], dtype=np.int32), 3, 0, 0)
        ok = run(h, good, [0, 1, 2])
        assert ok[0] == 0 and np.all(np.isfinite(ok[3])) and np.all(ok[3][6:] == 0.0) and np.all(ok[3][3] == 0.0)
        # out of range: nothing is written
        for bad in (run(h, good, [0, 1, 2], flags=1), run(h, good, [0, 1, 2], flags=4), run(h, good, [0, 1, 2], sizes_index=2),
                    run(h, good, [0, 1, 2], coalescent_index=5), run(h, good, [0, 1, 2], outputs=(False, False, False)),
                    run(h, good, [0, 2, 1]), run(h, good, [0, 1, 2], distances=False), run(h, good, [0, 1, 2], lengths=False),
                    run(h, [], [0, 0])):
            assert bad[0] == -5 and untouched(bad)
        assert run(h, good, [0, 1, 2], distances=False, outputs=(True, False, True))[0] == 0      # no W: no distances needed
        for at, value in ((0, 8), (1, -1), (2, 4), (13, 8), (11, 8), (15, 4)):
            ops = np.array(good).reshape(-1)
            ops[at] = value
            assert run(h, ops, [0, 1, 2])[0] == -5, (at, value)
        # not the forest: a vector read twice, one written twice, one read where it is written
        for ops, intervals in (([[2, 0, 0, -1, -1, 2, -1, 0], [3, 2, 1, 0, 1, 4, 5, 1]], [0, 1, 2]),
                               ([[2, 0, 0, -1, -1, 2, -1, 0], [3, 2, 1, -1, -1, 3, -1, 1], [4, 2, 1, 1, 1, 5, 6, 1]], [0, 1, 3]),
                               ([[2, 0, 0, -1, -1, 2, -1, 0], [2, 1, 1, -1, -1, 2, -1, 1]], [0, 1, 2]),
                               ([[2, 0, 0, -1, -1, 2, -1, 0], [3, 2, 1, 1, 1, 4, 5, 0]], [0, 2, 2])):
            refused = run(h, ops, intervals)
            assert refused[0] == -7 and untouched(refused)
        # (and the good list still runs after them, from the vectors as they stand: the same bits)
        b.updateBastaPartials(np.array(good, dtype=np.int32), 2, np.array([0, 1, 2], dtype=np.int32), 3, 0, 0)
        again = run(h, good, [0, 1, 2])
        assert again[0] == 0 and all(np.array_equal(x, y) for x, y in zip(ok[1:], again[1:]))
        # tips in different demes and matrices that move nothing: J = 0, -8, and the outputs are written
        b.setPartials(0, [1.0, 0.0, 0.0])
        b.setPartials(1, [0.0, 1.0, 0.0])
        for m in range(2):
            b.setTransitionMatrix(m, np.eye(3))
        b.updateBastaPartials(np.array(good, dtype=np.int32), 2, np.array([0, 1, 2], dtype=np.int32), 3, 0, 0)
        assert b.getBastaBuffer(0)[1] == 0.0
        nothing = run(h, good, [0, 1, 2])
        assert nothing[0] == -8 and not untouched(nothing) and not np.all(np.isfinite(nothing[3]))
        with pytest.raises(BeagleException):
            b.bastaGradient(np.array(good, dtype=np.int32), 2, np.array([0, 1, 2], dtype=np.int32), 3, [0.3, 0.7], [0.2, 0.5], 0, 0, flags=8)
        # the three natives of BastaJNIWrapper stay unbuilt
        assert lib.beagleBastaUpdatePartialsGrad(h, None, 0, None, 0, 0, 0) == -7
        assert lib.beagleBastaUpdateTransitionMatricesGrad(h, None, None, 0) == -7
        assert lib.beagleBastaAccumulatePartialsGrad(h, None, 0, None, 0, None, 0, 0, None) == -7
    finally:
        b.finalize(); plain.finalize(); one.finalize(); sharded.finalize(); parted.finalize()
