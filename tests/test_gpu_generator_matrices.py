"""Transition matrices straight from generators in one call (include/beagle_mi355.h beagleMi355UpdateTransitionMatricesFromGenerators;
csrc/kernels_generator.hip) against the longdouble yardstick and the numpy restatement's own error (tests/generator_matrices_reference.py,
pinned on the CPU tier), the same bits under every order, split and shard, likelihoods through generators.GeneratorModelSet against
the CPU oracle's eigen route and against the yardstick's matrices, the call's place in the engine's state, and every refusal."""
import copy
import ctypes as C
import os

import numpy as np
import pytest

import beast_mcmc_amd as bm
import generator_matrices_reference as gr
import helpers
from beast_mcmc_amd import generators
from beast_mcmc_amd.gradient import BranchGradient
from beast_mcmc_amd.inputs import substmodel

pytestmark = pytest.mark.gpu

NONE = bm.beagle.NONE
LD = np.longdouble


def category_rates(categories):
    return gr.CATEGORY_RATES if categories == 4 else (1.0,)


def instance(S, categories, slots, complex_eigen=False, resource_list=(1,), eigens=2):
    """2 tips x 16 patterns: enough to read matrices back and to turn two of them into site likelihoods."""
    b = bm.beagle.Beagle(2, 3, 2, S, 16, eigens, slots, categories, 0, resourceList=resource_list,
                         requirementFlags=bm.beagle.FLAG_EIGEN_COMPLEX if complex_eigen else 0)
    b.setCategoryRates(category_rates(categories))
    return b


def sharded_instance(S, categories, slots, shards=3):
    """(as tests/test_gpu_sharded_instance.py builds it: three shards on the one device)"""
    old = os.environ.get("BEAGLE_MI355_SHARDS")
    os.environ["BEAGLE_MI355_SHARDS"] = str(shards)
    try:
        g = len(bm.beagle.engine().resource_list()) - 2
        return instance(S, categories, slots, resource_list=(g + 1,))
    finally:
        if old is None:
            os.environ.pop("BEAGLE_MI355_SHARDS", None)
        else:
            os.environ["BEAGLE_MI355_SHARDS"] = old


def case_list(S):
    """-> (names, Q [3][S][S], generator index [21], length [21]): seven entries per generator, at the reference's lengths"""
    names = list(gr.generators(S))
    q = np.stack([gr.generators(S)[n] for n in names])
    gen = np.repeat(np.arange(len(names), dtype=np.int32), len(gr.LENGTHS))
    lengths = np.tile(np.asarray(gr.LENGTHS), len(names))
    return names, q, gen, lengths


# ---- 1. accuracy ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("categories", [1, 4])
@pytest.mark.parametrize("S", [2, 4, 5, 8, 9, 15, 16, 20, 61, 64])
def test_accuracy_against_the_longdouble_yardstick(S, categories):
    """Both kernel families (<= 8 states: a thread a matrix; 9 .. 64: a workgroup), the matrix-core threshold at 16, padded (5, 9, 15,
    61) and unpadded tiles.  Three generators in one call — dense, BSSVS-like, stiff; at 8 states the defective chain in the dense
    one's place — seven lengths each.  Every entry of every matrix: |dev - Y| <= 8 max(e_ref, (2^s + 20) eps) Y + 2^s 1e-19 with Y
    the yardstick and e_ref the restatement's own relative error against it; >= 0; the chain's zeros exact; d = 0 the identity."""
    names, q, gen, lengths = case_list(S)
    n = len(gen)
    b = instance(S, categories, n)
    b.updateTransitionMatricesFromGenerators(q, gen, None, np.arange(n), lengths)
    rates = category_rates(categories)
    worst, largest, compared = 0.0, 0, 0
    for e in range(n):
        got = b.getTransitionMatrix(e)
        assert got.shape == (categories, S, S) and np.all(np.isfinite(got)) and np.all(got >= 0.0)
        for c, rate in enumerate(rates):
            d = float(lengths[e] * rate)                                 # (the product the kernel forms)
            Y, s, e_ref = gr.reference(S, names[gen[e]], d)
            tol = gr.device_tolerance(Y, s, e_ref)
            err = np.abs(got[c].astype(LD) - Y)
            ratio = float((err / tol).max())                             # (the tolerance has a positive floor)
            worst, largest = max(worst, ratio), max(largest, s)
            assert np.all(err <= tol), (names[gen[e]], d, s, e_ref, float((err - tol).max()))
            compared += err.size
            if d == 0.0:
                assert np.array_equal(got[c], np.eye(S))
            if names[gen[e]] == "chain":
                assert np.all(got[c][np.tril_indices(S, -1)] == 0.0)
    print("S = %d, C = %d: worst error / tolerance %.3f, largest s %d" % (S, categories, worst, largest))
    assert compared == n * categories * S * S                          # no entry was left out
    assert b.generatorStats() == {"calls": 1, "matrices": n * categories, "max_squarings": largest, "refused": 0}
    b.finalize()


# ---- 2. the same bits --------------------------------------------------------------------------------------------------------------------
def evaluation_setup(b, S, categories):
    rng = np.random.default_rng(S)
    for t in range(2):
        b.setTipStates(t, rng.integers(0, S, size=16))
    b.setPatternWeights(np.ones(16))
    b.setStateFrequencies(0, np.full(S, 1.0 / S))
    b.setCategoryWeights(0, np.full(categories, 1.0 / categories))


def site_values(b, m0, m1):
    """The 16 site log-likelihoods of the two-tip tree over matrix slots m0 and m1: every shard of a sharded handle answers for its own
    patterns from its own copy of the slots."""
    b.updatePartials([2, NONE, NONE, 0, m0, 1, m1], 1, NONE)
    out = [0.0]
    b.calculateRootLogLikelihoods([2], [0], [0], [NONE], 1, out)
    return b.getSiteLogLikelihoods().copy()


@pytest.mark.parametrize("S", [4, 12, 20, 61])
def test_same_bits_whatever_the_list_the_split_and_the_shard(S, monkeypatch):
    names, q, gen, lengths = case_list(S)
    n = len(gen)
    every = np.arange(n)
    b = instance(S, 4, 2 * n)
    b.updateTransitionMatricesFromGenerators(q, gen, None, every, lengths)
    first = [b.getTransitionMatrix(int(k)).copy() for k in every]

    def check(handle, base, what):
        for k in every:
            assert np.array_equal(handle.getTransitionMatrix(int(base + k)).view(np.uint64), first[k].view(np.uint64)), (what, k)

    b.updateTransitionMatricesFromGenerators(q, gen[::-1], None, n + every[::-1], lengths[::-1])       # the list reversed
    check(b, n, "reversed")

    def scramble():                                                # (other values into the slots a variant is about to write)
        b.updateTransitionMatricesFromGenerators(q, gen, None, n + every, lengths * 0.5 + 0.01)
        assert not np.array_equal(b.getTransitionMatrix(n + 3), first[3])

    scramble()
    for k in every:                                                # one entry a call, its generator alone in the call
        b.updateTransitionMatricesFromGenerators(q[gen[k]][None], None, None, [n + k], lengths[k:k + 1])
    check(b, n, "one by one")
    scramble()
    b.updateTransitionMatricesFromGenerators(q[::-1].copy(), 2 - gen, None, n + every, lengths)      # the generators in another order
    check(b, n, "generators reversed")
    scramble()
    monkeypatch.setenv("BEAGLE_MI355_GENERATOR_CHUNK", "2")         # parts of two generators, launches of two entries
    b.updateTransitionMatricesFromGenerators(q, gen, None, n + every, lengths)
    monkeypatch.delenv("BEAGLE_MI355_GENERATOR_CHUNK")
    check(b, n, "split")
    b.updateTransitionMatricesFromGenerators(q, gen, None, every, lengths)                            # the first call again
    check(b, 0, "second call")
    many = sharded_instance(S, 4, n)
    many.updateTransitionMatricesFromGenerators(q, gen, None, every, lengths)
    check(many, 0, "sharded")
    evaluation_setup(b, S, 4); evaluation_setup(many, S, 4)
    for m0, m1 in ((1, 9), (17, 4), (12, 20)):
        assert np.array_equal(site_values(many, m0, m1), site_values(b, m0, m1)), (m0, m1)
    many.finalize(); b.finalize()


# ---- 3. / 4. likelihoods -----------------------------------------------------------------------------------------------------------------
class Evaluation(BranchGradient):
    """BranchGradient's buffer plan and post-order list with the branch matrices of ONE generator formed by `route`
    (generators.GeneratorModelSet); on an EIGEN_COMPLEX instance eigen slot 0 holds decompose_complex's system."""

    def __init__(self, wl, q, route, library=None, complex_eigen=False, **kw):
        wl = copy.copy(wl)
        if complex_eigen:
            wl.eig = substmodel.decompose_complex(q)[1]
        super().__init__(wl, library=library, requirement_flags=bm.beagle.FLAG_EIGEN_COMPLEX if complex_eigen else 0, **kw)
        self.models = generators.GeneratorModelSet(wl.state_count, 1, route=route, library=library)
        self.models.set_generator(0, q)

    def post_and_root(self):
        self.b.updatePartials(self._post_ops, len(self._post_ops) // 7, NONE)
        out = [0.0]
        self.b.calculateRootLogLikelihoods([self.post_index(self.tree.root)], [0], [0], [NONE], 1, out)
        return out[0]

    def log_likelihood(self):
        idx = self._nodes
        self.models.update_matrices(self.b, self._edge_matrix[self._set], self.branch_lengths[idx])
        return self.post_and_root()


def tree_workload(S, categories, seed=23):
    """12 taxa x 16 patterns, branch lengths uniform on [0.01, 2]"""
    wl = helpers.random_workload(12, 16, S, categories, seed=seed)
    lengths = np.random.default_rng(seed).uniform(0.01, 2.0, size=wl.tree.node_count)
    return wl, lengths


def with_lengths(ev, lengths):
    ev.branch_lengths = np.where(np.arange(ev.N) == ev.tree.root, 0.0, lengths)
    return ev


@pytest.mark.parametrize("S", [4, 7, 20, 61])
def test_dense_likelihood_matches_the_oracles_eigen_route(S, oracle_lib):
    """A dense asymmetric generator (rates uniform on [0.05, 5], normalised): route="device" on the engine against the CPU oracle fed
    decompose_complex's eigen system on an EIGEN_COMPLEX instance (route="host"), lnL and every site value to 1e-10 relative.  (For a
    dense generator at these lengths the eigen route itself is within 3e-11 of the yardstick.)"""
    categories = 4 if S == 4 else 1
    wl, lengths = tree_workload(S, categories)
    rng = np.random.default_rng(S)
    q = rng.uniform(0.05, 5.0, size=(S, S))
    np.fill_diagonal(q, 0.0)
    np.fill_diagonal(q, -q.sum(axis=1))
    q = generators.normalised(q)
    dev = with_lengths(Evaluation(wl, q, "device"), lengths)
    ref = with_lengths(Evaluation(wl, q, "host", library=oracle_lib, complex_eigen=True), lengths)
    got, want = dev.log_likelihood(), ref.log_likelihood()
    sites, ref_sites = dev.b.getSiteLogLikelihoods(), ref.b.getSiteLogLikelihoods()
    print("S = %d: lnL device route %.12f  oracle eigen route %.12f  rel %.2e  sites %.2e"
          % (S, got, want, helpers.rel_err(got, want), float(np.max(np.abs(sites - ref_sites) / np.abs(ref_sites)))))
    assert helpers.rel_err(got, want) <= 1e-10
    assert np.all(np.abs(sites - ref_sites) <= 1e-10 * np.abs(ref_sites))
    assert dev.b.generatorStats()["refused"] == 0
    dev.close(); ref.close()


def yardstick_matrices(q, lengths, rates):
    """[len(lengths)][C][S][S] doubles: the yardstick rounded"""
    return np.stack([np.stack([np.asarray(gr.yardstick(q, float(t * r)), dtype=np.float64) for r in rates]) for t in lengths])


def test_sparse_likelihood_matches_the_yardsticks_matrices():
    """The 61-state BSSVS-like generator on the same tree: the device-route lnL against the lnL of the same instance after the
    yardstick's matrices, rounded to double, were uploaded with setTransitionMatrix — 1e-10 relative.  The oracle's eigen route is no
    yardstick here: it is the route that gives negative probabilities on this generator (tests/test_generator_matrices_host.py)."""
    S = 61
    wl, lengths = tree_workload(S, 1)
    q = generators.normalised(gr.generators(S)["bssvs"])
    dev = with_lengths(Evaluation(wl, q, "device"), lengths)
    got = dev.log_likelihood()
    sites = dev.b.getSiteLogLikelihoods().copy()
    slots = dev._edge_matrix[0]
    for slot, m in zip(slots, yardstick_matrices(q, dev.branch_lengths[dev._nodes], wl.cat_rates)):
        assert np.all(dev.b.getTransitionMatrix(int(slot)) >= 0.0)
        dev.b.setTransitionMatrix(int(slot), m)
    want = dev.post_and_root()
    want_sites = dev.b.getSiteLogLikelihoods()
    print("lnL device route %.12f  yardstick matrices %.12f  rel %.2e" % (got, want, helpers.rel_err(got, want)))
    assert helpers.rel_err(got, want) <= 1e-10
    assert np.all(np.abs(sites - want_sites) <= 1e-10 * np.abs(want_sites))
    dev.close()


# ---- 5. engine state -------------------------------------------------------------------------------------------------------------------
def twin_pair(S, categories, seed=5, **kw):
    """Two instances over one workload and one dense generator: `a` is driven through the call, `b` through setTransitionMatrix with the
    bits `a` (or a scratch slot of it) produced — every later value must then agree to the bit."""
    wl, lengths = tree_workload(S, categories, seed=seed)
    q = generators.normalised(gr.generators(S)["dense"] if S in (4, 20) else gr.dense(S, np.random.default_rng(S)))
    a = with_lengths(Evaluation(wl, q, "device", **kw), lengths)
    b = with_lengths(Evaluation(wl, q, "device", **kw), lengths)
    return q, a, b


def copy_matrices(src, dst, slots):
    for s in slots:
        dst.b.setTransitionMatrix(int(s), src.b.getTransitionMatrix(int(s)))


@pytest.mark.parametrize("S", [4, 20])
def test_a_branch_move_and_its_restore_equal_the_twin_driven_by_set_transition_matrix(S):
    q, a, b = twin_pair(S, 4 if S == 4 else 1)
    slots = a._edge_matrix[0]
    first = a.log_likelihood()
    copy_matrices(a, b, slots)
    assert b.post_and_root() == first
    moved = [int(a.edges[2]), int(a.edges[7])]
    old = a.branch_lengths[moved].copy()
    a.b.updateTransitionMatricesFromGenerators(q, None, None, moved, old * 1.7 + 0.05)
    second = a.post_and_root()
    copy_matrices(a, b, moved)
    assert b.post_and_root() == second and second != first
    a.b.updateTransitionMatricesFromGenerators(q, None, None, moved, old)                    # the restore
    assert a.post_and_root() == first
    copy_matrices(a, b, moved)
    assert b.post_and_root() == first
    a.close(); b.close()


@pytest.mark.parametrize("S", [4, 20])
def test_the_call_behind_a_held_pre_order_list_leaves_the_twins_gradients(S):
    """updatePrePartials is held back until something reads its results; the call then rewrites a matrix the list reads, so the list
    runs first, over the old matrix — as it does on the twin, whose slot is rewritten by setTransitionMatrix."""
    q, a, b = twin_pair(S, 4 if S == 4 else 1, extra_matrices=1)
    slots = a._edge_matrix[0]
    a.log_likelihood()
    copy_matrices(a, b, slots)
    node = int(a.edges[3])
    new_length = a.branch_lengths[node] * 2.5 + 0.1
    a.b.updateTransitionMatricesFromGenerators(q, None, None, [a.extra_index], [new_length])
    new_matrix = a.b.getTransitionMatrix(a.extra_index).copy()
    grads = []
    for ev, rewrite in ((a, lambda: a.b.updateTransitionMatricesFromGenerators(q, None, None, [node], [new_length])),
                        (b, lambda: b.b.setTransitionMatrix(node, new_matrix))):
        lnl = ev.post_and_root()
        ev.b.setPartials(ev.pre_offset + ev.tree.root, ev._root_pre)
        ev.b.updatePrePartials(ev._pre_ops, len(ev._pre_ops) // 7, NONE)
        rewrite()
        ev.b.setDifferentialMatrix(ev.q_index, np.concatenate([(q * r).ravel() for r in ev.wl.cat_rates]))
        s1, _, _ = ev.b.calculateEdgeDifferentials(ev._edge_post[0], ev._pre_idx, ev._q1_idx, ev._w0, len(ev._nodes), want_squared=False)
        grads.append((lnl, np.asarray(s1).copy(), ev.b.getTransitionMatrix(node).copy()))
    assert grads[0][0] == grads[1][0]
    assert np.array_equal(grads[0][1], grads[1][1]) and np.all(np.isfinite(grads[0][1])) and np.any(grads[0][1] != 0.0)
    assert np.array_equal(grads[0][2], new_matrix) and np.array_equal(grads[1][2], new_matrix)
    # ... and over the old matrix: the gradients of an evaluation in which nothing was rewritten
    a.b.updateTransitionMatricesFromGenerators(q, None, None, [node], [a.branch_lengths[node]])
    a.post_and_root()
    a.b.setPartials(a.pre_offset + a.tree.root, a._root_pre)
    a.b.updatePrePartials(a._pre_ops, len(a._pre_ops) // 7, NONE)
    a.b.setDifferentialMatrix(a.q_index, np.concatenate([(q * r).ravel() for r in a.wl.cat_rates]))
    s1, _, _ = a.b.calculateEdgeDifferentials(a._edge_post[0], a._pre_idx, a._q1_idx, a._w0, len(a._nodes), want_squared=False)
    # (a list that runs on its own and one that runs with the edge sums associate the same sums differently: the project's 1e-10, not
    # the bits; a list run over the NEW matrix would move the gradients in the first digits)
    s1 = np.asarray(s1)
    print("held list: largest relative difference to the plain evaluation %.2e" % float(np.max(np.abs(s1 - grads[0][1]) / np.abs(s1))))
    assert np.all(np.abs(s1 - grads[0][1]) <= 1e-10 * np.abs(s1))
    a.close(); b.close()


@pytest.mark.parametrize("S", [4, 20])
def test_a_folded_tips_branch_matrix_rewritten_by_the_call(S):
    """Tip 0 carries an emission table with S codes (beagleMi355SetTipEmission folds it into the tip's branch matrix in front of every
    list): the fold must see the matrix the call wrote."""
    q, a, b = twin_pair(S, 4 if S == 4 else 1)
    rng = np.random.default_rng(S + 1)
    table = rng.dirichlet(np.full(S, 0.5), size=S) * 0.9 + 0.1 / S
    codes = rng.integers(0, S, size=16)
    slots = a._edge_matrix[0]
    for ev in (a, b):
        ev.b.setTipEmission(0, codes, table)
    first = a.log_likelihood()
    copy_matrices(a, b, slots)
    assert b.post_and_root() == first
    a.b.updateTransitionMatricesFromGenerators(q, None, None, [0], [a.branch_lengths[0] * 3.0 + 0.2])
    second = a.post_and_root()
    copy_matrices(a, b, [0])
    assert b.post_and_root() == second and second != first
    assert a.b.tipEmissionStats()["folded"] == b.b.tipEmissionStats()["folded"] >= 1
    a.close(); b.close()


@pytest.mark.parametrize("S", [4, 20])
def test_partitioned_instance_with_a_generator_and_a_rate_set_per_partition(S):
    """Two partitions of 8 patterns, each with its own generator, rate set and set of matrix slots, evaluated with the ...ByPartition
    calls: per-partition lnL of the call's matrices against the yardstick's uploaded with setTransitionMatrix, 1e-10 relative."""
    categories = 4 if S == 4 else 1
    wl, lengths = tree_workload(S, categories, seed=9)
    tr, T, N = wl.tree, wl.tree.tip_count, wl.tree.node_count
    qs = np.stack([generators.normalised(gr.dense(S, np.random.default_rng(10 * S + k))) for k in range(2)])
    rate_sets = [np.asarray(wl.cat_rates), np.asarray(wl.cat_rates)[::-1] * 0.7 + 0.1]
    b = bm.beagle.Beagle(T, N, T, S, 16, 2, 2 * N, categories, 0)
    for t in range(T):
        b.setTipStates(t, wl.tip_states[t])
    b.setPatternWeights(wl.weights)
    b.setPatternPartitions(2, np.repeat(np.arange(2, dtype=np.int32), 8))
    for k in range(2):
        b.setStateFrequencies(k, wl.freqs)
        b.setCategoryWeights(k, wl.cat_weights)
        b.setCategoryRatesWithIndex(k, rate_sets[k])
    edges = np.asarray([n for n in range(N) if n != tr.root], dtype=np.int32)
    slots = np.concatenate([edges + k * N for k in range(2)]).astype(np.int32)
    gen = np.repeat(np.arange(2, dtype=np.int32), len(edges))
    ops = []
    for k in range(2):
        for n in tr.postorder():
            if n >= T:
                l, r = int(tr.left[n]), int(tr.right[n])
                ops += [n, NONE, NONE, l, l + k * N, r, r + k * N, k, NONE]

    def evaluate():
        b.updatePartialsByPartition(ops, len(ops) // 9)
        by, tot = np.zeros(2), [0.0]
        b.calculateRootLogLikelihoodsByPartition([tr.root, tr.root], [0, 1], [0, 1], [NONE, NONE], [0, 1], 2, 1, by, tot)
        return by.copy(), tot[0]

    b.updateTransitionMatricesFromGenerators(qs, gen, gen, slots, np.tile(lengths[edges], 2))
    got, got_total = evaluate()
    for k in range(2):
        for slot, m in zip(edges + k * N, yardstick_matrices(qs[k], lengths[edges], rate_sets[k])):
            b.setTransitionMatrix(int(slot), m)
    want, want_total = evaluate()
    print("by partition: call %s  yardstick %s" % (got, want))
    assert np.all(np.abs(got - want) <= 1e-10 * np.abs(want)) and helpers.rel_err(got_total, want_total) <= 1e-10
    assert got[0] != got[1]
    b.finalize()


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_slots_as_they_were():
    S, n = 4, 3
    rng = np.random.default_rng(1)
    b = instance(S, 4, n)
    before = [rng.random((4, S, S)) for _ in range(n)]
    for k, m in enumerate(before):
        b.setTransitionMatrix(k, m)
    q = np.stack([gr.generators(S)["dense"], gr.generators(S)["bssvs"]])
    f = b._ext("beagleMi355UpdateTransitionMatricesFromGenerators",
               [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int])
    keep = []

    def ptr(a, dtype):
        if a is None:
            return None
        keep.append(np.ascontiguousarray(a, dtype=dtype))
        return keep[-1].ctypes.data

    def call(gens=q, gcount=2, gen=(0, 1), rate=(0, 1), slots=(0, 2), lengths=(0.1, 0.7), count=2):
        return f(b.instance, ptr(gens, np.float64), gcount, ptr(gen, np.int32), ptr(rate, np.int32), ptr(slots, np.int32),
                 ptr(lengths, np.float64), count)

    def refused(code, **change):
        assert call(**change) == code, change
        for k, want in enumerate(before):
            assert np.array_equal(b.getTransitionMatrix(k), want), change

    def with_entry(where, value):
        a = q.copy()
        a[where] = value
        return a

    refused(-5, gens=None)
    refused(-5, slots=None)
    refused(-5, lengths=None)
    refused(-5, count=-1)
    refused(-5, gcount=0)
    refused(-5, gcount=-3)
    refused(-5, slots=(0, 3))
    refused(-5, slots=(-1, 2))
    refused(-5, slots=(2, 2))                                    # a slot named twice
    refused(-5, gen=(0, 2))
    refused(-5, gen=(-1, 1))
    refused(-5, rate=(0, 2))
    refused(-5, rate=(-1, 0))
    for bad in (np.nan, np.inf, -np.inf):
        refused(-5, gens=with_entry((1, 0, 2), bad))
    refused(-5, gens=with_entry((0, 1, 3), -1e-300))             # a negative off-diagonal
    refused(-5, gens=with_entry((1, 2, 2), 1e-300))              # a positive diagonal
    refused(-5, gens=with_entry(1, 0.0))                         # mu is not > 0
    refused(-5, gens=with_entry((0, 0, 0), -np.inf))
    for bad in (-1e-300, np.nan, np.inf):
        refused(-5, lengths=(0.1, bad))
    assert call(count=0) == 0 and call(gen=None, rate=None, slots=None, lengths=None, count=0) == 0
    for k, want in enumerate(before):
        assert np.array_equal(b.getTransitionMatrix(k), want)
    assert b.generatorStats() == {"calls": 0, "matrices": 0, "max_squarings": 0, "refused": 0}
    g = b._ext("beagleMi355GeneratorStats", [C.c_int, C.c_void_p])
    assert g(b.instance, None) == -5
    assert call() == 0 and call(gen=None, rate=None) == 0        # ... and the call as it stands is accepted, NULL index lists too
    after = [b.getTransitionMatrix(k) for k in range(n)]
    assert not np.array_equal(after[0], before[0]) and np.array_equal(after[1], before[1]) and not np.array_equal(after[2], before[2])
    b.finalize()
    big = bm.beagle.Beagle(2, 3, 2, 65, 4, 1, 4, 1, 0)
    big.setTransitionMatrix(0, np.full(65 * 65, 0.25))
    with pytest.raises(bm.beagle.BeagleException) as e:
        big.updateTransitionMatricesFromGenerators(gr.dense(65, rng), None, None, [0], [0.1])
    assert e.value.code == -7
    assert np.array_equal(big.getTransitionMatrix(0).ravel(), np.full(65 * 65, 0.25))
    big.finalize()


@pytest.mark.parametrize("S", [8, 20])
def test_more_than_forty_squarings_is_nan_in_that_matrix_only(S):
    """x = mu d > 2^40: NaN in that (entry, category) only, counted, and the evaluation behind it answers -8."""
    q = gr.chain(8) if S == 8 else gr.generators(S)["dense"]
    mu = gr.max_rate(q)
    b = instance(S, 4, 3)
    evaluation_setup(b, S, 4)
    edge = 2.0 ** 39.5 / mu                                        # rates 0.1, 0.5, 1, 3: s = 37, 39, 40 and 42 — only the last is over
    b.updateTransitionMatricesFromGenerators(q, None, None, [0, 1, 2], [0.3, edge, 2.0 ** 60])
    m0, m1, m2 = (b.getTransitionMatrix(k) for k in range(3))
    assert np.all(np.isfinite(m0))
    over = [gr.squarings(mu * float(edge * r))[0] > gr.MAX_SQUARINGS for r in gr.CATEGORY_RATES]
    assert over == [False, False, False, True]
    for c in range(4):
        assert np.all(np.isnan(m1[c])) if over[c] else np.all(np.isfinite(m1[c]) & (m1[c] >= 0.0))
    assert np.all(np.isnan(m2))
    stats = b.generatorStats()
    assert stats["refused"] == 5 and stats["matrices"] == 12 and stats["max_squarings"] == 40
    root, zero, none, out = np.array([2], dtype=np.int32), np.zeros(1, dtype=np.int32), np.array([NONE], dtype=np.int32), np.zeros(1)

    def root_code():                                              # (the binding's own method tolerates -8, as BeagleJNIImpl does)
        return b._f["CalculateRootLogLikelihoods"](b.instance, bm.beagle._ip(root), bm.beagle._ip(zero), bm.beagle._ip(zero),
                                                   bm.beagle._ip(none), 1, bm.beagle._dp(out))

    b.updatePartials([2, NONE, NONE, 0, 0, 1, 1], 1, NONE)
    assert root_code() == -8
    b.updatePartials([2, NONE, NONE, 0, 0, 1, 0], 1, NONE)          # ... and the good matrix next to it serves
    assert root_code() == 0 and np.isfinite(out[0])
    b.finalize()
