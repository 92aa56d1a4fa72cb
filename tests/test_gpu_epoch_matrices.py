"""Branch matrices of epoch models in one call (include/beagle_mi355.h beagleMi355UpdateTransitionMatricesWithEpochs;
csrc/kernels_epoch.hip): single segments against beagleUpdateTransitionMatrices to the bit, every entry against the longdouble
yardstick and the stock natives' own error (tests/epoch_matrices_reference.py, pinned on the CPU tier), the same bits under every
order, split and shard, likelihoods through epochs.EpochTransitionMatrices against the CPU oracle driven by the reference's protocol,
the golden value, the call's place in the engine's state, and every refusal."""
import copy
import ctypes as C
import functools
import os

import numpy as np
import pytest

import beast_mcmc_amd as bm
import epoch_matrices_reference as er
import helpers
from beast_mcmc_amd import epochs
from beast_mcmc_amd.gradient import BranchGradient
from beast_mcmc_amd.inputs import substmodel, trees

pytestmark = pytest.mark.gpu

NONE = bm.beagle.NONE
LD = np.longdouble


def category_rates(categories):
    if categories == 1:
        return (1.0,)
    return er.CATEGORY_RATES if categories == 4 else tuple(np.linspace(0.05, 3.0, categories))


def systems_of(S, complex_eigen):
    return er.complex_systems(S) if complex_eigen else er.real_systems(S)


def instance(S, categories, slots, complex_eigen=False, resource_list=(1,)):
    """2 tips x 16 patterns: enough to read matrices back and to turn two of them into site likelihoods; the three eigen systems set"""
    b = bm.beagle.Beagle(2, 3, 2, S, 16, er.EIGEN_SYSTEMS, slots, categories, 0, resourceList=resource_list,
                         requirementFlags=bm.beagle.FLAG_EIGEN_COMPLEX if complex_eigen else 0)
    b.setCategoryRates(category_rates(categories))
    for k, e in enumerate(systems_of(S, complex_eigen)):
        b.setEigenDecomposition(k, e.evec, e.ievc, e.evals)
    return b


def sharded_instance(S, categories, slots, shards=2):
    """(as tests/test_gpu_sharded_instance.py builds it: the shards on the one device)"""
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


@functools.lru_cache(maxsize=None)
def yardstick(S, complex_eigen, e, rate):
    """(computed once per case; the C = 1 rate is one of the C = 4 rates)"""
    return er.yardstick(systems_of(S, complex_eigen), er.ENTRIES[e], rate, complex_eigen)


def stock_fold(b, entry, result, scratch):
    """The reference's sequence for one branch through the stock natives: an updateTransitionMatrices per segment into scratch slots,
    then first x second -> result with the result as the next first (the left fold of SubstitutionModelDelegate's deque).  A single
    segment goes straight to its slot.  scratch: 2 n - 2 free slots."""
    n = len(entry)
    if n == 1:
        b.updateTransitionMatrices(entry[0][0], [result], None, None, [entry[0][1]], 1)
        return
    for j, (k, t) in enumerate(entry):
        b.updateTransitionMatrices(k, [scratch + j], None, None, [t], 1)
    acc = scratch
    for j in range(1, n):
        res = result if j == n - 1 else scratch + n + j - 1
        b.convolveTransitionMatrices([acc], [scratch + j], [res], 1)
        acc = res


# ---- 1. accuracy ---------------------------------------------------------------------------------------------------------------------
CASES = [(S, c, False) for S in (2, 4, 5, 8, 9, 15, 16, 20, 61, 64) for c in (1, 4)] + [(4, 17, False), (4, 4, True), (20, 4, True)]


@pytest.mark.parametrize("S,categories,complex_eigen", CASES)
def test_accuracy_against_update_transition_matrices_and_the_longdouble_yardstick(S, categories, complex_eigen):
    """Both kernel families (<= 8 states: a thread a matrix; 9 .. 64: a workgroup), the matrix-core threshold at 16, padded (5, 9, 15,
    61) and unpadded tiles, real and conjugate-pair eigen systems.  Entries of 1, 2, 3 and 7 segments over three eigen systems
    (epoch_matrices_reference.ENTRIES).
    (a) every single-segment entry equals, bit for bit, the slot beagleUpdateTransitionMatrices writes with the same arguments;
    (b) for every entry e_new <= 8 max(e_stock, n S eps): e_new = max |device - yardstick| over the entry's categories, e_stock the same
        for the stock natives' fold on the same instance, eps = 2^-53 (the floor: the rounding of n sums of S products of entries <= 1).
    Largest e_new / max(e_stock, n S eps) seen on an MI355X: see DESIGN.md 4.16."""
    n = len(er.ENTRIES)
    offsets, eig, lengths = er.packed()
    b = instance(S, categories, 2 * n + 13, complex_eigen)
    b.updateTransitionMatricesWithEpochs(offsets, eig, lengths, None, np.arange(n))
    rates = category_rates(categories)
    worst = 0.0
    for e, entry in enumerate(er.ENTRIES):
        stock_fold(b, entry, n + e, 2 * n)
        got, stock = b.getTransitionMatrix(e), b.getTransitionMatrix(n + e)
        assert got.shape == (categories, S, S) and np.all(np.isfinite(got))
        if len(entry) == 1:
            assert np.array_equal(got.view(np.uint64), stock.view(np.uint64)), ("single segment", e)
        e_new = e_stock = 0.0
        for c, rate in enumerate(rates):
            y = yardstick(S, complex_eigen, e, float(rate)) if categories != 17 else er.yardstick(systems_of(S, complex_eigen), entry, rate, complex_eigen)
            e_new = max(e_new, float(np.abs(got[c].astype(LD) - y).max()))
            e_stock = max(e_stock, float(np.abs(stock[c].astype(LD) - y).max()))
        floor = max(e_stock, len(entry) * S * er.EPS)
        worst = max(worst, e_new / floor)
        print("S = %d C = %d entry %d (n = %d): e_new %.3e  e_stock %.3e  ratio %.3f" % (S, categories, e, len(entry), e_new, e_stock, e_new / floor))
        assert e_new <= er.tolerance(e_stock, len(entry), S), (e, e_new, e_stock)
    print("S = %d, C = %d%s: largest e_new / max(e_stock, n S eps) %.3f" % (S, categories, ", complex" if complex_eigen else "", worst))
    assert b.epochStats() == {"calls": 1, "matrices": n * categories, "segments": int(offsets[-1]), "longest": 7}
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
    n = len(er.ENTRIES)
    every = np.arange(n)
    b = instance(S, 4, 2 * n)

    def call(handle, order, base):
        """the entries in `order`, entry k into slot base + k"""
        offsets, eig, lengths = er.packed([er.ENTRIES[k] for k in order])
        handle.updateTransitionMatricesWithEpochs(offsets, eig, lengths, None, base + np.asarray(order))

    call(b, every, 0)
    first = [b.getTransitionMatrix(int(k)).copy() for k in every]

    def check(handle, base, what):
        for k in every:
            assert np.array_equal(handle.getTransitionMatrix(int(base + k)).view(np.uint64), first[k].view(np.uint64)), (what, k)

    def scramble():                                                # (other values into the slots a variant is about to write)
        offsets, eig, lengths = er.packed()
        b.updateTransitionMatricesWithEpochs(offsets, eig, lengths * 0.5 + 0.01, None, n + every)
        assert not np.array_equal(b.getTransitionMatrix(n + 7), first[7])

    call(b, every[::-1], n)
    check(b, n, "reversed")
    scramble()
    call(b, np.random.default_rng(S).permutation(n), n)
    check(b, n, "shuffled")
    scramble()
    call(b, every[:4], n); call(b, every[4:], n)
    check(b, n, "two calls")
    scramble()
    monkeypatch.setenv("BEAGLE_MI355_EPOCH_CHUNK", "3")             # launches of three entries
    call(b, every, n)
    monkeypatch.delenv("BEAGLE_MI355_EPOCH_CHUNK")
    check(b, n, "split")
    call(b, every, 0)                                               # the first call again
    check(b, 0, "second call")
    assert b.epochStats()["calls"] == 10
    many = sharded_instance(S, 4, n)
    call(many, every, 0)
    check(many, 0, "shard 0")                                       # (a sharded handle reads matrices back from its first shard)
    evaluation_setup(b, S, 4); evaluation_setup(many, S, 4)
    for m0, m1 in ((1, 9), (10, 4), (7, 8)):                       # ... and shard 1 answers for patterns 8 .. 15 from its own copy
        assert np.array_equal(site_values(many, m0, m1), site_values(b, m0, m1)), (m0, m1)
    many.finalize(); b.finalize()


# ---- 3. likelihoods ------------------------------------------------------------------------------------------------------------------
class Evaluation(BranchGradient):
    """BranchGradient's buffer plan and post-order list with the branch matrices of an epoch model formed by `route`
    (epochs.EpochTransitionMatrices).  Behind the differential slots: `extra` spare slots (first at extra_index), then the host
    route's pool and reserve buffer."""

    def __init__(self, wl, systems, times, route, library=None, complex_eigen=False, pool=100, extra=0):
        wl = copy.copy(wl)
        wl.eig = systems[0]
        super().__init__(wl, library=library, eigen_count=len(systems), extra_matrices=extra + pool + 1,
                         requirement_flags=bm.beagle.FLAG_EIGEN_COMPLEX if complex_eigen else 0)
        for k, e in enumerate(systems):
            self.b.setEigenDecomposition(k, e.evec, e.ievc, e.evals)
        self.route = route
        self.etm = epochs.EpochTransitionMatrices(epochs.EpochBranchModel(times, len(systems)), self.tree, self.extra_index + extra,
                                                  pool_size=pool)

    def post_and_root(self):
        self.b.updatePartials(self._post_ops, len(self._post_ops) // 7, NONE)
        out = [0.0]
        self.b.calculateRootLogLikelihoods([self.post_index(self.tree.root)], [0], [0], [NONE], 1, out)
        return out[0]

    def update(self, nodes, lengths, route=None):
        self.etm.update(self.b, nodes, lengths, route=self.route if route is None else route)

    def device_call(self, node, length, slot):
        """node's branch at `length`, by the call, into `slot`"""
        offsets, eig, seg = self.etm.segments([int(node)], [float(length)])
        self.b.updateTransitionMatricesWithEpochs(offsets, eig, seg, None, [int(slot)])

    def log_likelihood(self):
        self.update(self._nodes, self.branch_lengths[self._nodes])
        return self.post_and_root()


def tree_workload(S, categories, tips=16, seed=23):
    """`tips` taxa sampled through time x 16 patterns; epoch boundaries at 0.15 and 0.25 of the root height, where most lineages
    coexist: branches of one, two and three segments"""
    wl = copy.copy(helpers.random_workload(tips, 16, S, categories, seed=seed))
    wl.tree = trees.heterochronous_coalescent_tree(tips, np.random.default_rng(seed), sampling_span=1.0)
    top = float(wl.tree.height[wl.tree.root])
    return wl, [0.15 * top, 0.25 * top]


def assert_parity(dev, ref, what):
    got, want = dev.log_likelihood(), ref.log_likelihood()
    sites, ref_sites = dev.b.getSiteLogLikelihoods(), ref.b.getSiteLogLikelihoods()
    print("%s: lnL device route %.12f  oracle host route %.12f  rel %.2e  sites %.2e"
          % (what, got, want, helpers.rel_err(got, want), float(np.max(np.abs(sites - ref_sites) / np.abs(ref_sites)))))
    assert np.isfinite(got) and helpers.rel_err(got, want) <= 1e-10
    assert np.all(np.abs(sites - ref_sites) <= 1e-10 * np.abs(ref_sites))


@pytest.mark.parametrize("S", [4, 7, 20, 61])
def test_likelihood_matches_the_oracle_driven_by_the_host_route(S, oracle_lib):
    """A three-epoch model on 16 tips sampled through time: route="device" on the engine against the CPU oracle driven by the
    reference's protocol (route="host"), lnL and every site value to the project's parity bound, 1e-10 relative."""
    categories = 4 if S == 4 else 1
    wl, times = tree_workload(S, categories)
    systems = er.real_systems(S)
    dev = Evaluation(wl, systems, times, "device")
    ref = Evaluation(wl, systems, times, "host", library=oracle_lib)
    segs = [len(dev.etm.branch_mapping(n)[0]) for n in dev._nodes]
    assert {1, 2, 3} <= set(segs), segs
    assert_parity(dev, ref, "S = %d" % S)
    stats = dev.b.epochStats()
    assert stats["calls"] == 1 and stats["matrices"] == len(segs) * categories and stats["segments"] == sum(segs) and stats["longest"] == 3
    assert dev.etm.native_calls == 1 < ref.etm.native_calls
    dev.close(); ref.close()


def test_likelihood_with_eigen_slots_written_by_the_device_just_before(oracle_lib):
    """beagleMi355SetReversibleModels queues the decomposition of the three models; the call behind it must read what it wrote.
    Against the CPU oracle driven by the host route over the host's decomposition of the same models (lnL and site values, 1e-10
    relative), and against the same engine's host route over the device-written slots."""
    S = 20
    wl, times = tree_workload(S, 1)
    rng = np.random.default_rng(77)
    rel = rng.gamma(2.0, 1.0, size=(3, S * (S - 1) // 2)) + 0.1
    pis = rng.dirichlet(np.full(S, 5.0), size=3)
    host_systems = [substmodel.decompose_reversible(substmodel.reversible_q(rel[k], pis[k]), pis[k]) for k in range(3)]
    dev = Evaluation(wl, host_systems, times, "device")
    want = dev.log_likelihood()
    want_sites = dev.b.getSiteLogLikelihoods().copy()
    for k in range(3):                                              # other systems into the slots: a call that overtook the decomposition would read these
        e = er.real_systems(S)[k]
        dev.b.setEigenDecomposition(k, e.evec, e.ievc, e.evals)
    assert dev.log_likelihood() != want
    dev.b.setReversibleModels([0, 1, 2], rel, pis)
    got = dev.log_likelihood()
    sites = dev.b.getSiteLogLikelihoods().copy()
    dev.update(dev._nodes, dev.branch_lengths[dev._nodes], route="host")
    stock = dev.post_and_root()
    ref = Evaluation(wl, host_systems, times, "host", library=oracle_lib)
    oracle = ref.log_likelihood()
    oracle_sites = ref.b.getSiteLogLikelihoods()
    print("device-written eigen slots: device route %.12f  host route %.12f  host decomposition %.12f  oracle %.12f" % (got, stock, want, oracle))
    assert helpers.rel_err(got, oracle) <= 1e-10 and np.all(np.abs(sites - oracle_sites) <= 1e-10 * np.abs(oracle_sites))
    assert helpers.rel_err(got, want) <= 1e-10 and helpers.rel_err(got, stock) <= 1e-10
    assert np.all(np.abs(sites - want_sites) <= 1e-10 * np.abs(want_sites))
    dev.close(); ref.close()


# ---- 4. the golden value -----------------------------------------------------------------------------------------------------------------
def test_golden_epoch_convolution_through_the_device_route(engine_lib):
    """tests/TestXML/testEpochConvolutionOrder.xml through EpochBranchModel.mapping and ONE call; test_golden_epoch_convolution's bound"""
    from test_epoch_matrices_host import golden_lnl
    g = helpers.golden("epoch_convolution.json")
    lnl = golden_lnl(engine_lib, g, "device")
    assert abs(lnl - g["lnL"]) < 1e-5, lnl
    assert abs(golden_lnl(engine_lib, g, "host") - lnl) < 1e-12


# ---- 5. engine state -------------------------------------------------------------------------------------------------------------------
def twin_pair(S, seed=5, **kw):
    """Two engine instances over one workload and one epoch model: `a` is driven through the call, `b` through the host route."""
    categories = 4 if S == 4 else 1
    wl, times = tree_workload(S, categories, tips=12, seed=seed)
    systems = er.real_systems(S)
    return Evaluation(wl, systems, times, "device", **kw), Evaluation(wl, systems, times, "host", **kw)


def copy_matrices(src, dst, slots):
    for s in slots:
        dst.b.setTransitionMatrix(int(s), src.b.getTransitionMatrix(int(s)))


def crossing_branches(ev, segments):
    return [int(n) for n in ev._nodes if len(ev.etm.branch_mapping(n)[0]) == segments]


@pytest.mark.parametrize("S", [4, 20])
def test_a_branch_move_and_its_restore_equal_the_twin_driven_by_the_host_route(S):
    """The twin forms the same products through beagleConvolveTransitionMatrices, which sums a product in another order than the call
    does from 16 states on: the two agree to the project's parity bound (1e-10 relative), not to the bit.  On the instance itself the
    restore gives back the first value to the bit, and a twin handed the call's matrices follows it to the bit."""
    a, b = twin_pair(S)
    first = a.log_likelihood()
    assert helpers.rel_err(first, b.log_likelihood()) <= 1e-10
    moved = [crossing_branches(a, 3)[0], crossing_branches(a, 2)[0], crossing_branches(a, 1)[0]]
    old = a.branch_lengths[moved].copy()
    for ev in (a, b):
        ev.update(moved, old * 1.7 + 0.05)
    second = a.post_and_root()
    assert second != first and helpers.rel_err(second, b.post_and_root()) <= 1e-10
    for ev in (a, b):
        ev.update(moved, old)                                      # the restore
    assert a.post_and_root() == first
    assert helpers.rel_err(first, b.post_and_root()) <= 1e-10
    copy_matrices(a, b, a._edge_matrix[0])
    assert b.post_and_root() == first
    a.close(); b.close()


@pytest.mark.parametrize("S", [4, 20])
def test_the_call_behind_a_held_pre_order_list_leaves_the_twins_gradients(S):
    """updatePrePartials is held back until something reads its results; the call then rewrites a matrix the list reads, so the list
    runs first, over the old matrix — as it does on the twin, whose slot is rewritten by setTransitionMatrix."""
    a, b = twin_pair(S, extra=1)
    q = (a.wl.eig.evec * a.wl.eig.evals[None, :]) @ a.wl.eig.ievc
    a.log_likelihood()
    copy_matrices(a, b, a._edge_matrix[0])
    node = crossing_branches(a, 3)[0]
    new_length = a.branch_lengths[node] * 2.5 + 0.1
    a.device_call(node, new_length, a.extra_index)
    new_matrix = a.b.getTransitionMatrix(a.extra_index).copy()
    grads = []
    for ev, rewrite in ((a, lambda: a.device_call(node, new_length, node)), (b, lambda: b.b.setTransitionMatrix(node, new_matrix))):
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
    a.device_call(node, a.branch_lengths[node], node)
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
    """A tip carries an emission table with S codes (beagleMi355SetTipEmission folds it into the tip's branch matrix in front of every
    list): the fold must see the product the call wrote."""
    a, b = twin_pair(S)
    rng = np.random.default_rng(S + 1)
    table = rng.dirichlet(np.full(S, 0.5), size=S) * 0.9 + 0.1 / S
    codes = rng.integers(0, S, size=16)
    tip = [n for n in crossing_branches(a, 3) + crossing_branches(a, 2) if n < a.T][0]      # a tip whose branch crosses a boundary
    for ev in (a, b):
        ev.b.setTipEmission(tip, codes, table)
    first = a.log_likelihood()
    copy_matrices(a, b, a._edge_matrix[0])
    assert b.post_and_root() == first
    a.device_call(tip, a.branch_lengths[tip] * 3.0 + 0.2, tip)
    second = a.post_and_root()
    copy_matrices(a, b, [tip])
    assert b.post_and_root() == second and second != first
    assert a.b.tipEmissionStats()["folded"] == b.b.tipEmissionStats()["folded"] >= 1
    a.close(); b.close()


@pytest.mark.parametrize("S", [4, 20])
def test_partitioned_instance_with_a_rate_set_per_partition(S):
    """Two partitions of 8 patterns, each with its own rate set and set of matrix slots, evaluated with the ...ByPartition calls:
    per-partition lnL of the call's matrices against the host route's over the stock natives on the same instance, 1e-10 relative."""
    categories = 4 if S == 4 else 1
    wl, times = tree_workload(S, categories, tips=12, seed=9)
    tr, T, N = wl.tree, wl.tree.tip_count, wl.tree.node_count
    systems = er.real_systems(S)
    rate_sets = [np.asarray(wl.cat_rates), np.asarray(wl.cat_rates)[::-1] * 0.7 + 0.1]
    model = epochs.EpochBranchModel(times, 3)
    etms = [epochs.EpochTransitionMatrices(model, tr, 2 * N, pool_size=20, matrix_index=lambda n, k=k: int(n) + k * N, category_rate_index=k)
            for k in range(2)]
    b = bm.beagle.Beagle(T, N, T, S, 16, 3, etms[0].matrix_count, categories, 0)
    for t in range(T):
        b.setTipStates(t, wl.tip_states[t])
    b.setPatternWeights(wl.weights)
    b.setPatternPartitions(2, np.repeat(np.arange(2, dtype=np.int32), 8))
    for k in range(2):
        b.setStateFrequencies(k, wl.freqs)
        b.setCategoryWeights(k, wl.cat_weights)
        b.setCategoryRatesWithIndex(k, rate_sets[k])
    for k, e in enumerate(systems):
        b.setEigenDecomposition(k, e.evec, e.ievc, e.evals)
    edges = [n for n in range(N) if n != tr.root]
    lengths = [tr.branch_length(n) for n in edges]
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

    # both partitions in ONE call: the rate set per entry
    offsets, eig, seg = etms[0].segments(edges, lengths)
    two = lambda x: list(x) + list(x)
    b.updateTransitionMatricesWithEpochs(list(offsets) + [offsets[-1] + o for o in offsets[1:]], two(eig), two(seg),
                                         [0] * len(edges) + [1] * len(edges), edges + [n + N for n in edges])
    got, got_total = evaluate()
    for k in range(2):
        etms[k].update(b, edges, lengths, route="host")
    want, want_total = evaluate()
    print("by partition: call %s  host route %s" % (got, want))
    assert np.all(np.isfinite(got)) and np.all(np.abs(got - want) <= 1e-10 * np.abs(want)) and helpers.rel_err(got_total, want_total) <= 1e-10
    assert got[0] != got[1]
    b.finalize()


def test_an_instance_with_basta_buffers():
    """The call writes matrix slots only: on an instance shaped and allocated as BASTA's (no tips, one pattern, coalescent buffers) it
    gives the bits it gives on the same shape without them."""
    S, n = 4, len(er.ENTRIES)
    offsets, eig, lengths = er.packed()
    pair = []
    for basta in (False, True):
        b = bm.beagle.Beagle(0, 8, 0, S, 1, er.EIGEN_SYSTEMS, n, 1, 1)
        if basta:
            b.allocateCoalescentBuffers(5, 4, 12, 1)
        b.setCategoryRates([1.0])
        for k, e in enumerate(er.real_systems(S)):
            b.setEigenDecomposition(k, e.evec, e.ievc, e.evals)
        b.updateTransitionMatricesWithEpochs(offsets, eig, lengths, None, np.arange(n))
        pair.append(b)
    plain, with_basta = pair
    for k in range(n):
        got = with_basta.getTransitionMatrix(k)
        assert np.array_equal(plain.getTransitionMatrix(k).view(np.uint64), got.view(np.uint64))
        assert float(np.abs(got[0].astype(LD) - yardstick(S, False, k, 1.0)).max()) <= er.tolerance(0.0, len(er.ENTRIES[k]), S)
    plain.finalize(); with_basta.finalize()


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_slots_as_they_were():
    S, n = 4, 3
    rng = np.random.default_rng(1)
    b = instance(S, 4, n)
    before = [rng.random((4, S, S)) for _ in range(n)]
    for k, m in enumerate(before):
        b.setTransitionMatrix(k, m)
    f = b._ext("beagleMi355UpdateTransitionMatricesWithEpochs",
               [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int])
    keep = []

    def ptr(a, dtype):
        if a is None:
            return None
        keep.append(np.ascontiguousarray(a, dtype=dtype))
        return keep[-1].ctypes.data

    def call(offsets=(0, 2, 3), eig=(0, 1, 2), lengths=(0.1, 0.7, 0.3), rate=(0, 1), slots=(0, 2), count=2, flags=0):
        return f(b.instance, ptr(offsets, np.int32), ptr(eig, np.int32), ptr(lengths, np.float64), ptr(rate, np.int32),
                 ptr(slots, np.int32), count, flags)

    def refused(code, **change):
        assert call(**change) == code, change
        for k, want in enumerate(before):
            assert np.array_equal(b.getTransitionMatrix(k), want), change

    refused(-5, offsets=None)
    refused(-5, eig=None)
    refused(-5, lengths=None)
    refused(-5, slots=None)
    refused(-5, count=-1)
    refused(-5, flags=1)
    refused(-5, flags=-1)
    refused(-5, offsets=(1, 2, 3))                               # does not start at 0
    refused(-5, offsets=(0, 0, 3))                               # an entry without a segment
    refused(-5, offsets=(0, 3, 3))
    refused(-5, offsets=(0, 2, 1))                               # decreasing
    refused(-5, eig=(0, 3, 2))
    refused(-5, eig=(0, 1, -1))
    refused(-5, rate=(0, 3))
    refused(-5, rate=(-1, 0))
    refused(-5, slots=(0, 3))
    refused(-5, slots=(-1, 2))
    refused(-5, slots=(2, 2))                                    # a slot named twice
    for bad in (-1e-300, np.nan, np.inf, -np.inf):
        refused(-5, lengths=(0.1, bad, 0.3))
    assert call(count=0) == 0 and call(offsets=None, eig=None, lengths=None, rate=None, slots=None, count=0) == 0
    for k, want in enumerate(before):
        assert np.array_equal(b.getTransitionMatrix(k), want)
    assert b.epochStats() == {"calls": 0, "matrices": 0, "segments": 0, "longest": 0}
    g = b._ext("beagleMi355EpochStats", [C.c_int, C.c_void_p])
    assert g(b.instance, None) == -5
    assert call() == 0                                           # ... and the call as it stands is accepted
    assert b.epochStats() == {"calls": 1, "matrices": 8, "segments": 3, "longest": 2}
    assert call(rate=None, offsets=(0, 1, 2), slots=(2, 1)) == 0  # NULL rate list; the last call's longest entry
    assert b.epochStats() == {"calls": 2, "matrices": 16, "segments": 5, "longest": 1}
    after = [b.getTransitionMatrix(k) for k in range(n)]
    assert all(not np.array_equal(after[k], before[k]) for k in range(n))
    b.finalize()
    big = bm.beagle.Beagle(2, 3, 2, 65, 4, 1, 4, 1, 0)
    big.setTransitionMatrix(0, np.full(65 * 65, 0.25))
    with pytest.raises(bm.beagle.BeagleException) as e:
        big.updateTransitionMatricesWithEpochs([0, 1], [0], [0.1], None, [0])
    assert e.value.code == -7
    assert np.array_equal(big.getTransitionMatrix(0).ravel(), np.full(65 * 65, 0.25))
    big.finalize()
