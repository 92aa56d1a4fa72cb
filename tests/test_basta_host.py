"""CPU tier of the BASTA structured-coalescent likelihood: the host restatement (tests/basta_reference.py) against closed forms
and against itself in long double, the traversal of beast_mcmc_amd.basta against the restatement's, the golden fixture, and the
symbols of the two libraries."""
import os
import re
import subprocess

import numpy as np
import pytest

import basta_reference as ref
import beast_mcmc_amd as bm
import helpers
from beast_mcmc_amd import basta
from beast_mcmc_amd.inputs import substmodel, trees

ROOT = helpers.ROOT


def restated(tree, rate=1.0, sub=1):
    return ref.traverse(tree.left, tree.right, tree.height, tree.tip_count, rate, sub)


@pytest.mark.parametrize("tip_count,sub,tied", [(4, 1, 0), (51, 1, 0), (51, 2, 4), (200, 3, 0)])
def test_one_deme_is_the_kingman_coalescent(tip_count, sub, tied):
    """S = 1: every vector is (1), every matrix (1), the e, f, g, h formula collapses to L (L - 1) / 2N per unit time and every
    coalescence contributes 1 / N."""
    tree = trees.heterochronous_coalescent_tree(tip_count, np.random.default_rng(tip_count + sub), tied=tied)
    ops, intervals, lengths, mats, n_buffers, n_intervals = restated(tree, 1.0, sub)
    population = 0.37
    logl, _, _ = ref.evaluate(np.ones((tip_count, 1)), ops, intervals, lengths, {m: np.ones((1, 1)) for m, _ in mats},
                              [population], n_buffers, n_intervals)
    want = ref.kingman_log_density(tree.height, tip_count, population)
    assert abs(logl - want) <= 1e-13 * abs(want)


def test_two_tips_in_two_demes_by_hand():
    """Tips in demes 0 and 1 at heights 0 and 0.3, coalescing at 1.0; migration rates a (0 -> 1) and b (1 -> 0) backwards in
    time.  exp(Q^T t) of a two-state chain is known in closed form, and so is every term of the density."""
    a, b, n0, n1 = 0.8, 0.3, 0.6, 1.9
    tree = trees.Tree([-1, -1, 0], [-1, -1, 1], [0.0, 0.3, 1.0], 2)
    q = np.array([[-a, a], [b, -b]])

    def expm_t(t):                                   # exp(Q^T t)
        pi = np.array([b, a]) / (a + b)
        decay = np.exp(-(a + b) * t)
        p = np.array([[pi[0] + pi[1] * decay, pi[1] - pi[1] * decay], [pi[0] - pi[0] * decay, pi[1] + pi[0] * decay]])
        return p.T

    ops, intervals, lengths, mats, n_buffers, n_intervals = restated(tree)
    assert [m for m, _ in mats] == [0, 1] and np.allclose([t for _, t in mats], [0.3, 0.7])
    tips = np.eye(2)
    logl, _, probabilities = ref.evaluate(tips, ops, intervals, lengths, {0: expm_t(0.3), 1: expm_t(0.7)}, [n0, n1], n_buffers, n_intervals)
    # by hand: interval 1 (length 0.3) holds one lineage, which starts as (1, 0) and ends as u
    u = expm_t(0.3) @ np.array([1.0, 0.0])
    sizes = np.array([n0, n1])
    first = 0.0                                      # one lineage: e^2 = f and g^2 = h, and nothing coalesces
    # interval 2 (length 0.7): lineages u and (0, 1) at the start, v and w at the end; they coalesce
    v, w = expm_t(0.7) @ u, expm_t(0.7) @ np.array([0.0, 1.0])
    start, end = u + np.array([0.0, 1.0]), v + w
    second = -0.7 * np.sum((start ** 2 - (u ** 2 + np.array([0.0, 1.0])) + end ** 2 - (v ** 2 + w ** 2)) / sizes) / 4
    prob = np.sum(v * w / sizes)
    want = first + second + np.log(prob)
    assert abs(probabilities[1] - prob) <= 1e-15 * prob and probabilities[0] == 0.0
    assert abs(logl - want) <= 1e-14 * abs(want)
    # and the decomposition route gives the same matrices: transposed eigen system of Q
    w_, v_ = np.linalg.eig(q)
    te = basta.transpose_eigen(substmodel.EigenDecomposition(v_, np.linalg.inv(v_), w_))
    got = ref.transition_matrices(te.evec, te.ievc, te.evals, mats)
    assert np.allclose(got[0], expm_t(0.3), rtol=1e-13, atol=1e-15) and np.allclose(got[1], expm_t(0.7), rtol=1e-13, atol=1e-15)


def test_transposed_complex_eigen_system_gives_the_transposed_matrix():
    q = np.array([[-1.0, 1.0, 0.0], [0.0, -0.7, 0.7], [1.3, 0.0, -1.3]])
    _, eig = substmodel.decompose_complex(q)
    assert np.any(eig.evals[3:] != 0.0)
    te = basta.transpose_eigen(eig)
    plain = ref.transition_matrices(eig.evec, eig.ievc, eig.evals, [(0, 0.4)])[0]
    transposed = ref.transition_matrices(te.evec, te.ievc, te.evals, [(0, 0.4)])[0]
    assert np.allclose(transposed, plain.T, rtol=1e-12, atol=1e-15)
    assert np.allclose(plain.sum(axis=1), 1.0)


@pytest.mark.parametrize("state_count", [3, 20, 61])
def test_fp64_restatement_against_long_double(state_count):
    """Same fp64 matrices on both sides; every component within d (S + 4) 2^-53 relative (depths: basta_reference.depths).
    Random chains 2 000 deep with a renormalising coalescence every 7th step."""
    if np.finfo(np.longdouble).eps >= np.finfo(np.float64).eps:
        pytest.skip("numpy.longdouble is no wider than float64 on this platform")
    rng = np.random.default_rng(state_count)
    s, depth = state_count, 2000
    matrices = {m: rng.dirichlet(np.ones(s), size=s) for m in range(8)}
    ops, intervals, nxt, cur = [], [0], 2, 0
    for k in range(depth):
        if k % 7 == 6:
            ops.append([nxt, cur, k % 8, 1, (k + 3) % 8, nxt + 1, nxt + 2, k])
            cur, nxt = nxt, nxt + 3
        else:
            ops.append([nxt, cur, k % 8, -1, -1, nxt, -1, k])
            cur, nxt = nxt, nxt + 1
        intervals.append(len(ops))
    ops, intervals = np.array(ops, dtype=np.int32), np.array(intervals, dtype=np.int32)
    tips = rng.dirichlet(np.ones(s), size=2)
    sizes = rng.gamma(4.0, 0.5, size=s) + 0.05
    lengths = rng.uniform(0.01, 0.1, size=depth)
    _, p64, c64 = ref.evaluate(tips, ops, intervals, lengths, matrices, sizes, nxt, depth)
    _, pld, cld = ref.evaluate(tips, ops, intervals, lengths, matrices, sizes, nxt, depth, dtype=np.longdouble)
    d, per_op = ref.depths(ops, nxt)
    worst = 0.0
    for buffer in range(2, nxt):
        rel = np.abs(p64[buffer].astype(np.longdouble) - pld[buffer]) / pld[buffer]
        bound = d[buffer] * (s + 4) * 2.0 ** -53
        worst = max(worst, float(rel.max() / bound))
        assert rel.max() <= bound, (buffer, float(rel.max()), bound)
    for k, op in enumerate(ops):
        if op[3] >= 0:
            assert abs(c64[op[7]] - cld[op[7]]) <= per_op[k] * (s + 4) * 2.0 ** -53 * cld[op[7]]
    print("S = %d: the fp64 side used at most %.3f of the bound" % (s, worst))


@pytest.mark.parametrize("tip_count,sub,tied,rate", [(4, 1, 0, 1.0), (51, 2, 3, 0.7), (120, 1, 0, 2.0)])
def test_package_traversal_is_the_restated_one(tip_count, sub, tied, rate):
    tree = trees.heterochronous_coalescent_tree(tip_count, np.random.default_rng(tip_count), tied=tied)
    tr = basta.traverse(tree, rate, sub)
    ops, intervals, lengths, mats, n_buffers, n_intervals = restated(tree, rate, sub)
    assert np.array_equal(tr.operations, ops) and np.array_equal(tr.intervals, intervals) and np.array_equal(tr.lengths, lengths)
    assert tr.matrices == mats and tr.buffer_count == n_buffers and tr.interval_count == n_intervals
    # the sparse numbering of the reference: offset * nodeCount + node, accumulation buffers nodeCount + node
    n = tree.node_count
    two = tr.sparse[tr.sparse[:, 3] >= 0]
    assert np.all(two[:, 0] < n) and np.all(two[:, 5] // n == 1) and np.all(two[:, 6] // n == 1)
    assert len(two) == tip_count - 1
    one = tr.sparse[tr.sparse[:, 3] < 0]
    assert np.all(one[:, 0] == one[:, 5]) and np.all(one[:, 0] >= 2 * n) and np.all(one[:, 0] % n == one[:, 1] % n)
    # compacted: every buffer below the count, first use in increasing order
    assert tr.operations[:, [0, 1, 5]].max() < tr.buffer_count <= tr.sparse.max() + 1


@pytest.mark.parametrize("name", ["four_taxa", "fifty_one"])
def test_golden_fixture(name):
    g = helpers.golden("basta.json")[name]
    s, t = g["state_count"], g["tip_count"]
    tree = trees.Tree(g["left"], g["right"], g["height"], 2 * t - 2)
    tr = basta.traverse(tree, g["rate"], g["sub_intervals"])
    assert tr.operations.reshape(-1).tolist() == g["operations"] and tr.intervals.tolist() == g["intervals"]
    assert np.allclose(tr.lengths, g["lengths"], rtol=1e-15, atol=0.0)
    matrices = {int(k): np.array(v).reshape(s, s) for k, v in g["matrices"].items()}
    logl, _, probabilities = ref.evaluate(np.array(g["tips"]).reshape(t, s), tr.operations, tr.intervals, tr.lengths, matrices,
                                          g["sizes"], g["buffer_count"], g["interval_count"])
    assert abs(logl - g["log_likelihood"]) <= 1e-13 * abs(g["log_likelihood"])
    assert np.allclose(probabilities, g["coalescent_probabilities"], rtol=1e-13, atol=0.0)
    if name == "four_taxa":                          # unit rates: exp(Q t) = 1/3 + (2/3 or -1/3) exp(-3 t)
        for m, length in g["matrix_lengths"]:
            want = np.full((3, 3), (1.0 - np.exp(-3.0 * length)) / 3.0) + np.eye(3) * np.exp(-3.0 * length)
            assert np.allclose(matrices[m], want, rtol=1e-13, atol=0.0)


def test_every_basta_call_of_the_header_is_bound_and_exported(engine_lib):
    hdr = open(os.path.join(ROOT, "include", "beagle_mi355.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    names = sorted(set(re.findall(r"\b(beagleBasta[A-Za-z0-9]+)\s*\(", hdr)))
    assert len(names) >= 7
    for required in ("AllocateCoalescentBuffers", "UpdatePartials", "AccumulatePartials", "GetBuffer", "UpdatePartialsGrad",
                     "UpdateTransitionMatricesGrad", "AccumulatePartialsGrad"):
        assert "beagleBasta" + required in names
    assert all(n in bm.beagle.ABI_SYMBOLS for n in names)
    assert all(hasattr(engine_lib.lib, n) for n in names)


def test_the_bit_library_exports_the_seven_natives_and_nothing_else():
    lib = os.path.join(ROOT, "beast-mcmc_amd", "lib", "libhmsbeagle-jni-bit.so")
    if not os.path.exists(lib):
        __import__("importlib").import_module("beast-mcmc_amd.build").build_basta_jni()
    out = subprocess.run(["nm", "-D", "--defined-only", lib], check=True, capture_output=True, text=True).stdout
    names = sorted(line.split()[-1] for line in out.splitlines() if line.strip())
    want = sorted("Java_beagle_basta_BastaJNIWrapper_" + n for n in
                  ("allocateCoalescentBuffers", "getBastaBuffer", "updateBastaPartials", "accumulateBastaPartials", "updateBastaPartialsGrad",
                   "updateTransitionMatricesGrad", "accumulateBastaPartialsGrad"))
    assert names == want
    dyn = subprocess.run(["readelf", "-d", lib], check=True, capture_output=True, text=True).stdout
    assert "libhmsbeagle-jni.so" in dyn and "$ORIGIN" in dyn
