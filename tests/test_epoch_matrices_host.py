"""Epoch models on the CPU tier: EpochBranchModel.mapping against hand-worked cases, the restated SubstitutionModelDelegate protocol
(beast_mcmc_amd/epochs.py route="host") on the CPU oracle at pool sizes that take every one of its paths, the reference's golden
value through it, and the longdouble yardstick (tests/epoch_matrices_reference.py) the GPU tier measures against."""
import copy
import os
import re

import numpy as np
import pytest

import beast_mcmc_amd as bm
import epoch_matrices_reference as er
import helpers
from beast_mcmc_amd import epochs
from beast_mcmc_amd.inputs import substmodel, trees

NONE = bm.beagle.NONE
SYMBOLS = ("beagleMi355UpdateTransitionMatricesWithEpochs", "beagleMi355EpochStats")


def test_the_header_declares_and_the_veneer_binds_the_call():
    hdr = open(os.path.join(helpers.ROOT, "include", "beagle_mi355.h")).read()
    for sym in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % sym, hdr)
        assert sym in bm.beagle.ABI_SYMBOLS
    assert hasattr(bm.beagle.Beagle, "updateTransitionMatricesWithEpochs") and hasattr(bm.beagle.Beagle, "epochStats")
    assert epochs.SYMBOL == SYMBOLS[0]


# ---- mapping -------------------------------------------------------------------------------------------------------------------------
MODEL = epochs.EpochBranchModel([1.0, 2.0, 3.0], 4)


@pytest.mark.parametrize("node,parent,order,weights", [
    (0.25, 0.75, [0], [0.5]),                                       # inside the first epoch
    (2.25, 2.75, [2], [0.5]),                                       # inside a middle one
    (3.5, 8.0, [3], [4.5]),                                         # above the last boundary
    (0.5, 1.25, [1, 0], [0.25, 0.5]),                               # one boundary
    (0.5, 3.5, [3, 2, 1, 0], [0.5, 1.0, 1.0, 0.5]),                 # three boundaries: node below the first, parent above the last
    (1.0, 1.5, [1], [0.5]),                                         # node height ON a boundary: it belongs to the epoch above
    (2.0, 3.25, [3, 2], [0.25, 1.0]),                               # ... and crossing one more
    (0.5, 2.0, [2, 1, 0], [0.0, 1.0, 0.5]),                         # parent height ON a boundary: a zero-weight segment at the root end
    (1.0, 2.0, [2, 1], [0.0, 1.0]),                                 # both
])
def test_mapping_hand_worked(node, parent, order, weights):
    got_order, got_weights = MODEL.mapping(node, parent)
    assert got_order == order and got_weights == weights              # (every figure above is exact in binary)
    assert sum(got_weights) == parent - node
    assert got_order == sorted(got_order, reverse=True)              # root end (the oldest epoch) first


def test_mapping_needs_one_more_model_than_times():
    with pytest.raises(ValueError):
        epochs.EpochBranchModel([1.0, 2.0], 2)
    assert epochs.EpochBranchModel([], 1).mapping(0.0, 5.0) == ([0], [5.0])


def test_segments_are_the_mappings_of_every_branch(oracle_lib):
    """The one call's packed lists against ``mapping`` and the Java expression branch by branch, to the bit — on a tree with heights
    ON boundaries (node and parent) and on the 12-tip tree — and against what the host route hands updateTransitionMatrices."""
    tree = TwoLevelTree()
    for tr, times, count in ((tree, [1.0, 2.0, 3.0], 4), (epoch_workload().tree, boundaries(epoch_workload().tree), 3)):
        etm = epochs.EpochTransitionMatrices(epochs.EpochBranchModel(times, count), tr, len(tr.height), eigen_index=lambda k: 2 * k + 1)
        branches = [n for n in range(len(tr.height)) if tr.parent[n] >= 0]
        lengths = [0.37 * (n + 1) for n in branches]
        offsets, eig, seg = etm.segments(branches, lengths)
        assert offsets.dtype == np.int32 and eig.dtype == np.int32 and seg.dtype == np.float64 and offsets[0] == 0
        for e, (b, t) in enumerate(zip(branches, lengths)):
            order, weights = etm.branch_mapping(b)
            total = 0.0
            for w in weights:
                total += w
            want = [t] if len(order) == 1 else [w * t / total for w in weights]
            assert list(eig[offsets[e]:offsets[e + 1]]) == [2 * k + 1 for k in order], b
            assert list(seg[offsets[e]:offsets[e + 1]]) == want, b
    assert etm.segments([], [])[0].tolist() == [0]


class TwoLevelTree:
    """heights chosen on and off the boundaries 1, 2, 3: tips at 0, 0.5, 1 (on), 2.5; parents at 2 (on), 3.5, 8"""
    def __init__(self):
        self.height = np.asarray([0.0, 0.5, 1.0, 2.5, 2.0, 3.5, 8.0])
        self.parent = np.asarray([4, 4, 5, 5, 6, 6, -1], dtype=np.int32)


# ---- the restated protocol on the oracle -----------------------------------------------------------------------------------------------
def epoch_workload(S=4, categories=2, tips=12, seed=7):
    wl = copy.copy(helpers.random_workload(tips, 16, S, categories, seed=seed))
    wl.tree = trees.heterochronous_coalescent_tree(tips, np.random.default_rng(seed), sampling_span=1.0)
    return wl


def boundaries(tree, fractions=(0.15, 0.25)):
    top = float(tree.height[tree.root])
    return [f * top for f in fractions]


def run_host(library, wl, systems, times, pool):
    """-> (lnL, site values, branch matrices [edges][C][S][S], the update's log, native calls, flushes by kind)"""
    tr = wl.tree
    N, T = tr.node_count, tr.tip_count
    etm = epochs.EpochTransitionMatrices(epochs.EpochBranchModel(times, len(systems)), tr, N, pool_size=pool)
    b = bm.beagle.Beagle(T, N, T, wl.state_count, wl.pattern_count, len(systems), etm.matrix_count, wl.category_count, 0, library=library)
    try:
        for t in range(T):
            b.setTipStates(t, wl.tip_states[t])
        b.setPatternWeights(wl.weights); b.setStateFrequencies(0, wl.freqs)
        b.setCategoryRates(wl.cat_rates); b.setCategoryWeights(0, wl.cat_weights)
        for k, e in enumerate(systems):
            b.setEigenDecomposition(k, e.evec, e.ievc, e.evals)
        edges = [n for n in range(N) if n != tr.root]
        etm.log = []
        etm.update(b, edges, [tr.branch_length(n) for n in edges], route="host")
        ops = []
        for n in tr.postorder():
            if n >= T:
                l, r = int(tr.left[n]), int(tr.right[n])
                ops += [n, NONE, NONE, l, l, r, r]
        b.updatePartials(ops, len(ops) // 7, NONE)
        out = [0.0]
        b.calculateRootLogLikelihoods([tr.root], [0], [0], [NONE], 1, out)
        mats = np.stack([b.getTransitionMatrix(n).copy() for n in edges])
        return out[0], b.getSiteLogLikelihoods().copy(), mats, etm.log, etm.native_calls, dict(etm.flushes)
    finally:
        b.finalize()


def test_host_route_gives_the_same_bits_at_every_pool_size(oracle_lib):
    """12 tips sampled through time, 3 eigen systems, boundaries at 0.15 and 0.25 of the root height (where most lineages coexist).
    Pool 3 (= the eigen count: every three-segment branch goes through the reserve buffer), 4, 7 (the flush in the middle of a round)
    and 100 (no flush at all)."""
    wl = epoch_workload()
    systems = er.real_systems(4)
    times = boundaries(wl.tree)
    etm = epochs.EpochTransitionMatrices(epochs.EpochBranchModel(times, 3), wl.tree, wl.tree.node_count)
    crossing = [len(etm.branch_mapping(n)[0]) for n in range(wl.tree.node_count) if n != wl.tree.root]
    assert crossing.count(3) >= 2 and crossing.count(2) >= 2 and crossing.count(1) >= 2, crossing
    runs = {pool: run_host(oracle_lib, wl, systems, times, pool) for pool in (3, 4, 7, 100)}
    lnl, sites, mats = runs[100][:3]
    assert np.isfinite(lnl) and np.all(np.abs(mats.sum(axis=-1) - 1.0) < 1e-12)
    N = wl.tree.node_count
    for pool, (l, s, m, log, calls, _) in runs.items():
        assert l == lnl and np.array_equal(s, sites) and np.array_equal(m.view(np.uint64), mats.view(np.uint64)), pool
        assert er.replay_pool(log, N) > 0                             # no pool buffer written while live, none read while empty
        used = {x for rec in log if rec[0] == "convolve" for x in rec[3]} | {x for rec in log if rec[0] == "update" for x in rec[2]}
        assert max(used) <= N + pool                                  # nothing behind the reserve buffer
        assert calls == len(log)
    reserve = lambda pool: any(rec[0] == "convolve" and N + pool in rec[3] for rec in runs[pool][3])
    assert reserve(3) and not reserve(100)
    flushes = {pool: run[5] for pool, run in runs.items()}
    print(flushes)
    assert flushes[100] == {"early": 0, "mid_round": 0, "reserve": 0}
    assert flushes[3]["reserve"] > 0 and flushes[3]["early"] > 0 and flushes[7]["mid_round"] > 0
    assert runs[100][4] < runs[7][4] < runs[3][4]                     # fewer buffers, more flushes
    # ... and the matrices are the yardstick's to rounding
    edges = [n for n in range(N) if n != wl.tree.root]
    offsets, eig, seg = etm.segments(edges, [wl.tree.branch_length(n) for n in edges])
    for e, n in enumerate(edges):
        entry = tuple((eig[j], seg[j]) for j in range(offsets[e], offsets[e + 1]))
        for c, rate in enumerate(wl.cat_rates):
            y = er.yardstick(systems, entry, rate)
            assert float(np.abs(mats[e][c].astype(er.LD) - y).max()) <= 1e-13, (n, c)


def test_golden_epoch_convolution_through_the_mapping_and_the_host_route(oracle_lib):
    """tests/TestXML/testEpochConvolutionOrder.xml: the value test_oracle_golden.py reproduces by hand, here through
    EpochBranchModel.mapping and the restated delegate; that test's own bound."""
    g = helpers.golden("epoch_convolution.json")
    lnl = golden_lnl(oracle_lib, g, "host")
    assert abs(lnl - g["lnL"]) < 1e-5, lnl


class TwoTipTree:
    def __init__(self, tip_heights, root_height):
        self.height = np.asarray(list(tip_heights) + [root_height], dtype=np.float64)
        self.parent = np.asarray([2, 2, -1], dtype=np.int32)


def golden_lnl(library, g, route, pool=8):
    pi = [0.5, 0.5]
    tree = TwoTipTree(g["tip_heights"], g["root_height"])
    etm = epochs.EpochTransitionMatrices(epochs.EpochBranchModel(g["transition_times"], len(g["epoch_rates"])), tree, 3, pool_size=pool)
    b = bm.beagle.Beagle(2, 3, 2, 2, 1, len(g["epoch_rates"]), etm.matrix_count, 1, 0, library=library)
    try:
        for k, r in enumerate(g["epoch_rates"]):
            e = substmodel.decompose_general(substmodel.asymmetric_q(r, pi), pi)
            b.setEigenDecomposition(k, e.evec, e.ievc, e.evals)
        b.setCategoryRates([1.0]); b.setCategoryWeights(0, [1.0]); b.setStateFrequencies(0, g["root_freqs"])
        b.setPatternWeights([1.0])
        etm.update(b, [0, 1], [(g["root_height"] - h) * g["clock_rate"] for h in g["tip_heights"]], route=route)
        b.setTipStates(0, [g["states"][0]]); b.setTipStates(1, [g["states"][1]])
        b.updatePartials([2, NONE, NONE, 0, 0, 1, 1], 1, NONE)
        out = [0.0]
        b.calculateRootLogLikelihoods([2], [0], [0], [NONE], 1, out)
        return out[0]
    finally:
        b.finalize()


# ---- the yardstick -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,complex_eigen", [(4, False), (20, False), (4, True), (20, True)])
def test_yardstick_against_float64_and_the_semigroup(S, complex_eigen):
    """The yardstick's segment matrix agrees with the float64 product to float64's rounding, its rows sum to 1, two segments of one
    model fold to the matrix of the summed length, and the fold is the LEFT fold in the given order."""
    systems = er.complex_systems(S) if complex_eigen else er.real_systems(S)
    for k, e in enumerate(systems):
        for d in (0.0, 1e-6, 0.3, 10.0):
            y = er.segment_matrix(e, d, complex_eigen)
            assert y.dtype == er.LD and np.all(y >= 0.0)
            assert float(np.abs(y.sum(axis=1) - 1.0).max()) < 1e-11
            if not complex_eigen:
                assert float(np.abs(y - e.transition_probabilities(d)).max()) < 1e-12
            if d == 0.0:
                assert float(np.abs(y - np.eye(S)).max()) < 1e-12
        two = er.yardstick(systems, ((k, 0.3), (k, 0.5)), 1.0, complex_eigen)
        assert float(np.abs(two - er.segment_matrix(e, 0.8, complex_eigen)).max()) < 1e-11
    a, b_, c = (er.segment_matrix(systems[k], d, complex_eigen) for k, d in enumerate((0.4, 0.5, 0.6)))
    fold = er.yardstick(systems, ((0, 0.4), (1, 0.5), (2, 0.6)), 1.0, complex_eigen)
    assert np.array_equal(fold, a.dot(b_).dot(c))
    assert float(np.abs(fold - c.dot(b_).dot(a)).max()) > 1e-6          # the order matters
    if complex_eigen:
        assert any(np.any(e.evals[S:] != 0.0) for e in systems)


def test_yardstick_clamps_per_segment():
    """A segment whose product cancels below zero is clamped before it enters the fold."""
    e = substmodel.EigenDecomposition(np.eye(2), np.array([[1.0, -1e-3], [0.0, 1.0]]), np.zeros(2))
    m = er.segment_matrix(e, 1.0)
    assert m[0, 1] == 0.0 and m[0, 0] == 1.0
    fold = er.yardstick((e, e, e), ((0, 1.0), (1, 1.0)), 1.0)
    assert np.array_equal(fold, np.eye(2))


def test_tolerance_and_entries():
    assert er.tolerance(0.0, 7, 64) == 8 * 7 * 64 * 2.0 ** -53 and er.tolerance(1e-9, 1, 4) == 8e-9
    offsets, eig, lengths = er.packed()
    n = np.diff(offsets)
    assert set(n) == {1, 2, 3, 7} and offsets[0] == 0 and len(eig) == offsets[-1] == len(lengths)
    assert lengths.min() == 0.0 and lengths[lengths > 0].min() == 1e-6 and lengths.max() == 10.0
    assert any(eig[j] == eig[j + 1] for e in range(len(n)) for j in range(offsets[e], offsets[e + 1] - 1))
