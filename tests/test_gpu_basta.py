"""The BASTA structured-coalescent likelihood on the device (beagleBasta*, beast_mcmc_amd.basta) against the host restatement
(tests/basta_reference.py).

Bounds.  With the SAME fp64 matrices on both sides every vector component is compared within 4 d (S + 4) 2^-53 relative, d = the
number of matrix-vector products on the longest dependency path that ends in the vector, a two-child operation counting as three
(basta_reference.depths): matrices and vectors are non-negative, nothing cancels, the componentwise relative error of a chain of
S-term dot products grows additively — each side is within d (S + 4) 2^-53 of the exact value (tests/test_basta_host.py checks the
restatement against long double), and a factor 2 on top covers fused against separate multiply-add.  A component that is exactly
zero in the restatement must be exactly zero on the device.  Through updateTransitionMatrices the matrices themselves differ in
the last bits, and the log-density is held to the project's parity bound, 1e-10 relative.
"""
import os
import subprocess

import numpy as np
import pytest

import basta_reference as ref
import beast_mcmc_amd as bm
import helpers
from beast_mcmc_amd import basta
from beast_mcmc_amd.inputs import substmodel, trees

pytestmark = pytest.mark.gpu
Beagle, BeagleException, FLAG_EIGEN_COMPLEX = bm.beagle.Beagle, bm.beagle.BeagleException, bm.beagle.FLAG_EIGEN_COMPLEX
ROOT = helpers.ROOT
EPS = 2.0 ** -53


def make_tree(kind, tip_count, seed):
    rng = np.random.default_rng(seed)
    if kind == "distinct":
        return trees.heterochronous_coalescent_tree(tip_count, rng, sampling_span=1.0, population=3.0)
    if kind == "tied":
        return trees.heterochronous_coalescent_tree(tip_count, rng, sampling_span=1.0, population=3.0, tied=5)
    assert kind == "caterpillar"
    return trees.caterpillar_tree(tip_count, root_height=2.0)


def random_rates(state_count, rng):
    q = rng.gamma(2.0, 0.5, size=(state_count, state_count)) / state_count
    np.fill_diagonal(q, 0.0)
    np.fill_diagonal(q, -q.sum(axis=1))
    return q


def matrices_for(q, tr):
    """fp64 matrices exp(Q^T t) of the traversal's matrix operations (any non-negative matrices would do: both sides get these)"""
    w, v = np.linalg.eig(q.T)
    vi = np.linalg.inv(v)
    return {m: np.abs(np.real((v * np.exp(w * t)[None, :]) @ vi)) for m, t in tr.matrices}


class Case:
    def __init__(self, state_count, tip_count, sub_intervals=1, kind="distinct", seed=0, tips="one-hot"):
        rng = np.random.default_rng(1000 + seed)
        self.tree = make_tree(kind, tip_count, seed)
        self.q = random_rates(state_count, rng)
        self.sizes = rng.gamma(4.0, 0.5, size=state_count) + 0.05
        self.demes = rng.integers(0, state_count, size=tip_count)
        tip_data = self.demes
        if tips == "ambiguous":
            tip_data = np.zeros((tip_count, state_count))
            for i in range(tip_count):
                on = rng.random(state_count) < 0.5
                on[self.demes[i]] = True
                tip_data[i] = on / on.sum()
        w, v = np.linalg.eig(self.q)
        self.like = basta.BastaLikelihood(self.tree, tip_data, basta.transpose_eigen(substmodel.EigenDecomposition(np.real(v), np.real(np.linalg.inv(v)), np.real(w))),
                                          self.sizes, rate=0.8, sub_intervals=sub_intervals)
        self.sub = sub_intervals

    def traversal(self):
        return basta.traverse(self.tree, 0.8, self.sub)

    def reference(self, matrices, sizes=None):
        tr = self.traversal()
        return ref.evaluate(self.like.tips, tr.operations, tr.intervals, tr.lengths, matrices,
                            self.sizes if sizes is None else sizes, tr.buffer_count, tr.interval_count)

    def close(self):
        self.like.close()


def check_vectors(case, tr, partials, probabilities):
    s = case.like.state_count
    d, per_op = ref.depths(tr.operations, tr.buffer_count)
    worst = 0.0
    for k, op in enumerate(tr.operations):
        for buffer in ([op[0]] if op[3] < 0 else [op[0], op[5], op[6]]):
            got, want = case.like.partials(int(buffer)), partials[buffer]
            zero = want == 0.0
            assert np.all(got[zero] == 0.0), (k, buffer)
            bound = 4.0 * d[buffer] * (s + 4) * EPS
            rel = np.abs(got[~zero] - want[~zero]) / want[~zero]
            if rel.size:
                worst = max(worst, float(rel.max()) / bound)
                assert rel.max() <= bound, (k, buffer, float(rel.max()), bound)
        if op[3] >= 0:
            got, want = probabilities_got(case)[op[7]], probabilities[op[7]]
            bound = 4.0 * per_op[k] * (s + 4) * EPS
            assert abs(got - want) <= bound * want, (k, got, want)
    return worst


_probabilities = {}


def probabilities_got(case):
    if _probabilities.get("case") is not case:
        _probabilities["case"], _probabilities["v"] = case, case.like.coalescent_probabilities()
    return _probabilities["v"]


VECTOR_CASES = [(s, t, 1, "distinct", "one-hot") for s in (2, 3, 4, 7, 20, 61) for t in (4, 51, 500)] + \
               [(3, 51, 2, "distinct", "one-hot"), (20, 51, 2, "tied", "one-hot"), (4, 500, 2, "distinct", "one-hot"), (61, 51, 2, "distinct", "ambiguous"),
                (4, 51, 1, "tied", "one-hot"), (20, 500, 1, "tied", "ambiguous"), (7, 51, 1, "caterpillar", "one-hot"), (4, 500, 1, "caterpillar", "one-hot"),
                (20, 51, 2, "caterpillar", "ambiguous"),
                (70, 51, 1, "distinct", "one-hot")]      # (above 64 states the kernel reads its matrices from memory, not from an LDS copy)


@pytest.mark.parametrize("state_count,tip_count,sub,kind,tips", VECTOR_CASES)
def test_every_vector_and_probability_matches_the_restatement(state_count, tip_count, sub, kind, tips):
    case = Case(state_count, tip_count, sub, kind, seed=state_count * 7 + tip_count, tips=tips)
    try:
        tr = case.traversal()
        matrices = matrices_for(case.q, tr)
        logl = case.like.log_likelihood(matrices=matrices)
        for m in list(matrices)[:3]:
            assert np.array_equal(case.like.transition_matrix(m), matrices[m])
        want, partials, probabilities = case.reference(matrices)
        _probabilities.clear()
        worst = check_vectors(case, tr, partials, probabilities)
        print("S=%d T=%d sub=%d %s %s: %d operations, %d intervals, logL %.12f (restatement %.12f), worst vector error %.3f of the bound"
              % (state_count, tip_count, sub, kind, tips, len(tr.operations), len(tr.intervals) - 1, logl, want, worst))
        assert abs(logl - want) <= 1e-10 * abs(want)
        assert case.like.beagle.bastaStats()[1] >= 1 and case.like.beagle.bastaStats()[2] == 0      # one launch, not one per interval
    finally:
        case.close()


def cyclic_complex(rng):
    q = np.zeros((3, 3))
    a = rng.uniform(0.5, 2.0, size=3)
    q[0, 1], q[1, 2], q[2, 0] = a
    q[0, 2], q[1, 0], q[2, 1] = 0.05 * rng.uniform(0.5, 1.0, size=3)
    np.fill_diagonal(q, -q.sum(axis=1))
    return q


@pytest.mark.parametrize("spectrum", ["real", "complex"])
def test_log_density_through_the_transposed_eigen_system(spectrum):
    rng = np.random.default_rng(77)
    if spectrum == "complex":
        _, eig = substmodel.decompose_complex(cyclic_complex(rng))
        assert np.any(eig.evals[3:] != 0.0)
        s = 3
    else:
        s = 5
        eig, _ = substmodel.random_reversible(s, rng)
    te = basta.transpose_eigen(eig)
    tree = make_tree("distinct", 51, 3)
    sizes = rng.gamma(4.0, 0.5, size=s) + 0.05
    demes = rng.integers(0, s, size=51)
    like = basta.BastaLikelihood(tree, demes, te, sizes, rate=1.3, sub_intervals=2)
    try:
        got = like.log_likelihood()
        tr = basta.traverse(tree, 1.3, 2)
        matrices = ref.transition_matrices(te.evec, te.ievc, te.evals, tr.matrices)
        want, _, probabilities = ref.evaluate(like.tips, tr.operations, tr.intervals, tr.lengths, matrices, sizes, tr.buffer_count, tr.interval_count)
        print("%s spectrum: logL %.13f, restatement %.13f, relative difference %.3e" % (spectrum, got, want, abs(got - want) / abs(want)))
        assert abs(got - want) <= 1e-10 * abs(want)
        p = like.coalescent_probabilities()
        assert np.allclose(p[:tr.interval_count], probabilities, rtol=1e-10, atol=0.0)
    finally:
        like.close()


def test_repeat_accumulate_resize_and_flipped_sizes():
    case = Case(7, 51, 1, "distinct", seed=11)
    try:
        like, b = case.like, case.like.beagle
        tr = case.traversal()
        matrices = matrices_for(case.q, tr)
        first = like.log_likelihood(matrices=matrices)
        assert like.resizes == 1                  # the first evaluation outgrew the constructor's allocation: the tips were kept, not re-sent
        uploads = b.bastaStats()[0]
        second = like.log_likelihood(matrices=matrices)
        assert first == second                    # the same bits
        assert b.bastaStats()[0] == uploads       # an unchanged list is not sent again, by the update or by accumulate
        want, partials, _ = case.reference(matrices)
        assert abs(first - want) <= 1e-10 * abs(want)
        # accumulate ADDS
        n, m = len(tr.operations), len(tr.intervals)
        out = np.array([2.5, 7.0])
        b.accumulateBastaPartials(tr.operations, n, tr.intervals, m, tr.lengths, 0, 0, out)
        assert out[0] == 2.5 + first and out[1] == 7.0
        # a resize between evaluations keeps tips and everything else stored
        b.allocateCoalescentBuffers(5, like.max_intervals + 3, like.partials_count + 100, 0)
        for i in (0, 17, 50):
            assert np.array_equal(like.partials(i), like.tips[i])
        assert np.array_equal(like.partials(int(tr.operations[-1, 0])), partials[tr.operations[-1, 0]])      # (what the last update stored, too)
        assert like.log_likelihood(matrices=matrices) == first
        # population sizes flipped between indices 0 and 1
        other = case.sizes[::-1].copy() * 1.7
        like.set_population_sizes(other, flip=True)
        flipped = like.log_likelihood(matrices=matrices)
        assert like.sizes_index == 1
        want_flipped, _, _ = case.reference(matrices, sizes=other)
        assert abs(flipped - want_flipped) <= 1e-10 * abs(want_flipped)
        like.set_population_sizes(case.sizes, flip=True)
        assert like.log_likelihood(matrices=matrices) == first
    finally:
        case.close()


def test_a_chain_of_evaluations_with_changing_node_heights():
    case = Case(4, 51, 1, "distinct", seed=23)
    try:
        rng = np.random.default_rng(5)
        for step in range(20):
            node = int(rng.integers(case.tree.tip_count, case.tree.node_count))
            case.like.set_node_height(node, helpers.proposed_height(case.tree, node, rng))
            tr = case.traversal()
            matrices = matrices_for(case.q, tr)
            got = case.like.log_likelihood(matrices=matrices)
            want, _, _ = case.reference(matrices)
            assert abs(got - want) <= 1e-10 * abs(want), (step, got, want)
    finally:
        case.close()


def update_launches(tip_count):
    case = Case(4, tip_count, 1, "distinct", seed=tip_count)
    try:
        tr = case.traversal()
        case.like.log_likelihood(matrices=matrices_for(case.q, tr))
        b = case.like.beagle
        b.kernelTimer(1)
        b.updateBastaPartials(tr.operations, len(tr.operations), tr.intervals, len(tr.intervals), 0, 0)
        ms, launches = b.kernelTimer(0)
        return launches, len(tr.intervals) - 1, ms
    finally:
        case.close()


def test_update_launch_count_does_not_grow_with_the_interval_count():
    small, large = update_launches(51), update_launches(500)
    print("launches, intervals, ms: T=51 %s, T=500 %s" % (small, large))
    assert small[0] == large[0] and small[0] >= 1
    assert large[1] > 5 * small[1]


def test_a_list_that_is_no_forest_runs_interval_by_interval():
    """a vector read by two operations (and one overwritten in a later interval): still what the interval order says"""
    s = 3
    rng = np.random.default_rng(9)
    b = Beagle(0, 8, 0, s, 1, 2, 4, 1, 1, requirementFlags=FLAG_EIGEN_COMPLEX)
    try:
        b.allocateCoalescentBuffers(5, 4, 12, 1)
        tips = rng.dirichlet(np.ones(s), size=2)
        for i in range(2):
            b.setPartials(i, tips[i])
        sizes = np.array([0.5, 1.5, 2.5])
        b.setStateFrequencies(0, sizes)
        matrices = {m: rng.dirichlet(np.ones(s), size=s) for m in range(3)}
        for m, v in matrices.items():
            b.setTransitionMatrix(m, v)
        ops = np.array([[2, 0, 0, -1, -1, 2, -1, 0], [3, 1, 0, -1, -1, 3, -1, 0],
                        [4, 2, 1, -1, -1, 4, -1, 1], [5, 2, 1, -1, -1, 5, -1, 1],
                        [2, 4, 2, 5, 2, 6, 7, 2]], dtype=np.int32)
        intervals = np.array([0, 2, 4, 5], dtype=np.int32)
        lengths = np.array([0.1, 0.2, 0.3])
        b.updateBastaPartials(ops, 5, intervals, 4, 0, 0)
        out = np.zeros(1)
        b.accumulateBastaPartials(ops, 5, intervals, 4, lengths, 0, 0, out)
        assert b.bastaStats()[2] == 1 and b.bastaStats()[1] == 0
        want, partials, _ = ref.evaluate(tips, ops, intervals, lengths, matrices, sizes, 12, 4)
        assert abs(out[0] - want) <= 1e-12 * abs(want)
        for buffer in (2, 4, 5, 6, 7):
            assert np.allclose(b.getPartials(buffer).reshape(s), partials[buffer], rtol=1e-14, atol=0.0)
    finally:
        b.finalize()


def test_error_returns():
    import ctypes as C
    lib = bm.beagle.engine().lib
    I, D = C.POINTER(C.c_int), C.POINTER(C.c_double)
    update = lib.beagleBastaUpdatePartials
    update.argtypes = [C.c_int, I, C.c_int, I, C.c_int, C.c_int, C.c_int]
    accumulate = lib.beagleBastaAccumulatePartials
    accumulate.argtypes = [C.c_int, I, C.c_int, I, C.c_int, D, C.c_int, C.c_int, D]
    allocate = lib.beagleBastaAllocateCoalescentBuffers
    get = lib.beagleBastaGetBuffer
    get.argtypes = [C.c_int, C.c_int, D]

    def run(h, ops, intervals, sizes_index=0, probability_index=0):
        o = np.ascontiguousarray(ops, dtype=np.int32).reshape(-1)
        iv = np.ascontiguousarray(intervals, dtype=np.int32)
        return update(h, o.ctypes.data_as(I), len(o) // 8, iv.ctypes.data_as(I), len(iv), sizes_index, probability_index)

    good = [[2, 0, 0, -1, -1, 2, -1, 0], [3, 2, 1, 1, 1, 4, 5, 1]]
    b = Beagle(0, 8, 0, 3, 1, 2, 4, 1, 1, requirementFlags=FLAG_EIGEN_COMPLEX)
    wide = Beagle(0, 8, 0, 3, 5, 2, 4, 1, 1)                   # patternCount != 1
    cats = Beagle(0, 8, 0, 3, 1, 2, 4, 2, 1)                   # categoryCount != 1
    try:
        h = b.instance
        out = np.zeros(8)
        # before AllocateCoalescentBuffers
        assert run(h, good, [0, 1, 2]) == -7
        assert get(h, 0, out.ctypes.data_as(D)) == -7
        assert allocate(wide.instance, 5, 4, 8, 1, -1) == -7 and allocate(cats.instance, 5, 4, 8, 1, -1) == -7
        assert allocate(h, 5, 4, 8, 1, -1) == 0
        for i in range(2):
            b.setPartials(i, [0.2, 0.3, 0.5])
        b.setStateFrequencies(0, [1.0, 2.0, 3.0])
        for m in range(2):
            b.setTransitionMatrix(m, np.full((3, 3), 1.0 / 3))
        assert run(h, good, [0, 1, 2]) == 0
        bad = {"dest outside": (0, 8), "negative in1": (1, -1), "in1 outside": (1, 9), "matrix outside": (2, 4), "acc outside": (13, 8),
               "in2 outside": (11, 8), "interval number": (15, 4), "negative interval number": (7, -1)}
        for name, (at, value) in bad.items():
            ops = np.array(good).reshape(-1)
            ops[at] = value
            assert run(h, ops, [0, 1, 2]) == -5, name
        assert run(h, good, [0, 2, 1]) == -5                   # decreasing (and not ending at the count)
        assert run(h, good, [0, 2, 1, 2]) == -5                # decreasing
        assert run(h, good, [0, 1]) == -5                      # does not end at operationCount
        assert run(h, good, [0, 1, 3]) == -5
        assert run(h, good, [0, 1, 2], sizes_index=2) == -5 and run(h, good, [0, 1, 2], probability_index=5) == -5
        assert get(h, 5, out.ctypes.data_as(D)) == -5 and get(h, -1, out.ctypes.data_as(D)) == -5
        with pytest.raises(BeagleException):
            b.setPartials(8, [0.1, 0.2, 0.7])
        # NaN from accumulate: -8, the result untouched
        b.setStateFrequencies(0, [0.0, 2.0, 3.0])
        b.setPartials(0, [0.0, 0.0, 0.0])
        b.setPartials(1, [0.0, 0.0, 0.0])
        assert run(h, good, [0, 1, 2]) == 0
        o = np.array(good, dtype=np.int32).reshape(-1); iv = np.array([0, 1, 2], dtype=np.int32); ln = np.array([0.1, 0.2])
        res = np.array([1.25])
        assert accumulate(h, o.ctypes.data_as(I), 2, iv.ctypes.data_as(I), 3, ln.ctypes.data_as(D), 0, 0, res.ctypes.data_as(D)) == -8
        assert res[0] == 1.25
        # the gradient natives are not built
        assert lib.beagleBastaUpdatePartialsGrad(h, None, 0, None, 0, 0, 0) == -7
        assert lib.beagleBastaUpdateTransitionMatricesGrad(h, None, None, 0) == -7
        assert lib.beagleBastaAccumulatePartialsGrad(h, None, 0, None, 0, None, 0, 0, None) == -7
    finally:
        b.finalize(); wide.finalize(); cats.finalize()


def test_the_sharded_handle_has_no_basta():
    lib = bm.beagle.engine()
    gpus = len(lib.resource_list()) - 2          # [CPU placeholder, GPU 1..G, all GPUs]
    sharded = Beagle(0, 8, 0, 3, 1, 2, 4, 1, 1, resourceList=(gpus + 1,))
    try:
        assert lib.lib.beagleBastaAllocateCoalescentBuffers(sharded.instance, 5, 4, 8, 1, -1) == -7
    finally:
        sharded.finalize()


def test_an_ordinary_instance_next_to_a_basta_instance_is_unchanged():
    wl = helpers.random_workload(24, 700, 4, 4, seed=31)

    def chain(with_basta):
        rng = np.random.default_rng(2)
        tl = bm.treelikelihood.BeagleTreeLikelihood(wl)
        case = Case(4, 51, 1, "distinct", seed=3) if with_basta else None
        values = []
        try:
            for step in range(6):
                if case:
                    tr = case.traversal()
                    case.like.log_likelihood(matrices=matrices_for(case.q, tr))
                tl.makeDirty()
                values.append(tl.getLogLikelihood())
                if case:
                    node = int(rng.integers(case.tree.tip_count, case.tree.node_count))
                    case.like.set_node_height(node, helpers.proposed_height(case.tree, node, rng))
        finally:
            tl.close()
            if case:
                case.close()
        return values

    alone, together = chain(False), chain(True)
    assert alone == together


def test_the_jni_natives_give_the_c_abi_bits(tmp_path):
    g = helpers.golden("basta.json")["four_taxa"]
    s, t = g["state_count"], g["tip_count"]
    ops = np.array(g["operations"], dtype=np.int32).reshape(-1, 8)
    intervals, lengths = np.array(g["intervals"], dtype=np.int32), np.array(g["lengths"])
    matrices = {int(k): np.array(v).reshape(s, s) for k, v in g["matrices"].items()}
    tips = np.array(g["tips"]).reshape(t, s)
    n_buffers, max_intervals, n_matrices = g["buffer_count"] + 1, g["interval_count"], max(matrices) + 1
    # the C ABI route
    b = Beagle(0, n_buffers, 0, s, 1, 2, n_matrices, 1, 1, requirementFlags=FLAG_EIGEN_COMPLEX)
    try:
        b.allocateCoalescentBuffers(5, max_intervals, n_buffers, 1)
        for i in range(t):
            b.setPartials(i, tips[i])
        b.setStateFrequencies(0, g["sizes"])
        for m, v in matrices.items():
            b.setTransitionMatrix(m, v)
        b.updateBastaPartials(ops, len(ops), intervals, len(intervals), 0, 0)
        out = np.zeros(1)
        b.accumulateBastaPartials(ops, len(ops), intervals, len(intervals), lengths, 0, 0, out)
        probabilities = b.getBastaBuffer(0)
    finally:
        b.finalize()
    assert abs(out[0] - g["log_likelihood"]) <= 1e-12 * abs(g["log_likelihood"])
    exe = str(tmp_path / "fake_jvm_basta")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", os.path.join(ROOT, "tests", "native", "fake_jvm_basta.cpp"), "-ldl", "-o", exe], timeout=300)
    fixture = tmp_path / "four_taxa.txt"
    with open(fixture, "w") as fh:
        fh.write("%d %d %d %d %d %d %d\n" % (s, t, n_buffers, max_intervals, n_matrices, len(ops), len(intervals)))
        fh.write(" ".join(repr(float(x)) for x in tips.reshape(-1)) + "\n")
        fh.write(" ".join(repr(float(x)) for x in g["sizes"]) + "\n")
        fh.write("%d\n" % len(matrices))
        for m, v in matrices.items():
            fh.write("%d " % m + " ".join(repr(float(x)) for x in v.reshape(-1)) + "\n")
        fh.write(" ".join(str(int(x)) for x in ops.reshape(-1)) + "\n")
        fh.write(" ".join(str(int(x)) for x in intervals) + "\n")
        fh.write(" ".join(repr(float(x)) for x in lengths) + "\n")
    lib_dir = os.path.join(ROOT, "beast-mcmc_amd", "lib")
    run = subprocess.run([exe, os.path.join(lib_dir, "libhmsbeagle-jni.so"), os.path.join(lib_dir, "libhmsbeagle-jni-bit.so"), str(fixture)],
                         capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.returncode, run.stdout, run.stderr)
    lines = dict(line.split(" ", 1) for line in run.stdout.strip().splitlines())
    assert float.fromhex(lines["logL"].split()[0]) == out[0]
    assert lines["grad"].split() == ["-7", "-7", "-7"]
    got = [float.fromhex(x) for x in lines["probabilities"].split()[1:]]
    assert got == list(probabilities)
