"""Degenerate and stiff inputs on every kernel family, against the plain long-double reference (which decides what is exactly zero) and
the CPU oracle (which bounds the values) — tests/degenerate_cases.py builds the cases, tests/test_degenerate_host.py pins them on the CPU.

Part A  exact zeros: matrices injected through setTransitionMatrix after a first evaluation on the model's dense ones (so whatever
        the engine derived from matrices — cherry tables, fused cherry pairs, gathered matrix streams — is stale unless it is dropped),
        the same operation list re-issued, on every pruning route; the engine's own counters say which route ran.
Part B  zero-length branches and a rate-0 category through updateTransitionMatrices: matrices, likelihoods, partials, gradients.
Part C  trees scaled far outside the simulated range and extreme gamma shapes, the short-branch regimes against the oracle's long-double mode.

Every case: at most 12 taxa and 260 patterns — but for the two sub-pattern-table routes, which need the 17 taxa from which a list is cached."""
import ctypes as C

import numpy as np
import pytest

import beast_mcmc_amd as bm
import degenerate_cases as dc
import helpers
from beast_mcmc_amd.gradient import BranchGradient
from beast_mcmc_amd.treelikelihood import BeagleTreeLikelihood, RESCALE_ALWAYS, RESCALE_DYNAMIC, RESCALE_NONE
from test_gpu_gradients import close

pytestmark = pytest.mark.gpu
REL_TOL = 1e-10
NONE = bm.beagle.NONE
# the sub-pattern tables at this size, as tests/test_gpu_repeats.py switches them on (off below 2 MiB of partials; clades of up to half the patterns)
ANY_SIZE = {"BEAGLE_MI355_REPEATS_ANY_SIZE": "1", "BEAGLE_MI355_MEM_DEF_STEPS": "8", "BEAGLE_MI355_REPEAT_MAX_FRAC": "1/2"}
# ... and on a tree of 17 taxa: the planner keeps (and so compresses) only lists of 16 operations and more (planner.cpp WalkPlanner::plan).  At 4
# states the smallest matrix entry is 0.083, so a live value stays above 0.083^32 = 3e-35: the reference's exactness argument holds as at 12 taxa.
TABLE_SHAPE = {"T": 17}


def fast(d):            # every launch on the assembly loop k_walk4_fast
    assert d["walks"] > 0 and d["fast_walks"] == d["walks"] and d["repeat_clades"] == 0, d


def fast_write(d):
    fast(d)
    assert d["scale_writes"] > 0, d


def fast_read(d):
    fast(d)
    assert d["scale_reads"] > 0 and d["scale_writes"] == 0, d


def cpp_write(d):       # k_walk4, the C++ kernel of the same walk (BEAGLE_MI355_NO_FAST_WALK=1), rescaling in write mode
    assert d["walks"] > 0 and d["fast_walks"] == 0 and d["scale_writes"] > 0, d


def table(d):           # clades evaluated once per distinct sub-pattern (k_walk4Tab) and read by the walk
    assert d["walks"] > 0 and d["repeat_clades"] > 0 and d["table_reads"] > 0, d


def walk_read(d):       # k_walkT32 / k_walkT64: a walk, not the assembly loop, nodes left unstored
    assert d["walks"] > 0 and d["fast_walks"] == 0 and d["scale_writes"] == 0 and d["stored"] < d["micro_ops"], d


def walk_write(d):      # k_walkT32W1
    assert d["walks"] > 0 and d["fast_walks"] == 0 and d["scale_writes"] > 0, d


def levels(d):          # level kernels only (k_pruneGeneral; k_pruneTiledWrite / k_pruneTiled + k_rescaleTiled)
    assert d["walks"] == 0, d


def levels_write(d):    # 21..64 states in write mode: the level kernels; the counters see the factors written
    assert d["scale_writes"] > 0 and d["stored"] == d["micro_ops"], d


#         id                    S   C  scheme          read   tips as partials  environment  which route
ROUTES = [("walk4-write",        4, 4, RESCALE_ALWAYS,  False, False, {},       fast_write),
          ("walk4-read",         4, 4, RESCALE_DYNAMIC, True,  False, {},       fast_read),
          ("walk4-unscaled",     4, 4, RESCALE_NONE,    False, False, {},       fast),
          ("walk4-table",        4, 4, RESCALE_NONE,    False, False, ANY_SIZE, table),
          ("walk4-table-read",   4, 4, RESCALE_DYNAMIC, True,  False, ANY_SIZE, table),
          ("walk4-tip-partials", 4, 4, RESCALE_ALWAYS,  False, True,  {},       fast_write),
          ("walk4-cpp-write",    4, 4, RESCALE_ALWAYS,  False, False, {"BEAGLE_MI355_NO_FAST_WALK": "1"}, cpp_write),
          ("general7-write",     7, 3, RESCALE_ALWAYS,  False, False, {},       levels),
          ("general7-unscaled",  7, 3, RESCALE_NONE,    False, False, {},       levels),
          ("t32-read",          20, 4, RESCALE_DYNAMIC, True,  False, {},       walk_read),
          ("t32-write",         20, 4, RESCALE_ALWAYS,  False, False, {},       walk_write),
          ("t32-tip-partials",  20, 4, RESCALE_ALWAYS,  False, True,  {},       walk_write),
          ("tiled20-levels",    20, 5, RESCALE_ALWAYS,  False, False, {},       levels),
          ("t64-read",          61, 2, RESCALE_DYNAMIC, True,  False, {},       walk_read),
          ("t64-write",         61, 2, RESCALE_ALWAYS,  False, False, {},       levels_write),
          ("general70-write",   70, 2, RESCALE_ALWAYS,  False, False, {},       levels),
          ("general70-unscaled", 70, 2, RESCALE_NONE,   False, False, {},       levels)]
_oracle_runs = {}


def oracle_run(cs, key, scheme, read, oracle_lib):
    """The oracle's injected evaluation, once per (case, scheme, mode): tips as states or as partials are the same numbers to it."""
    k = (key, scheme, read)
    if k not in _oracle_runs:
        _oracle_runs[k] = dc.evaluate_injected(cs, scheme, library=oracle_lib, read_mode=read)
    return _oracle_runs[k]


def run_route(route, name, oracle_lib, monkeypatch, assert_route=True, **shape):
    rid, S, Cn, scheme, read, as_partials, env, expect = route
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    if expect is table:
        shape = dict(TABLE_SHAPE, **shape)
    cs = dc.case(name, S, Cn, **shape)
    res = dc.evaluate_injected(cs, scheme, read_mode=read, as_partials=as_partials, twice=expect is table)
    d = dc.stats_delta(res)
    print("%s / %s: the injected list ran as %s" % (rid, name, d))
    if assert_route:
        expect(d)
    what = "%s / %s" % (rid, name)
    dc.check_against_reference(cs, res, what)
    dc.check_against_oracle(cs, res, oracle_run(cs, (name, S, Cn, tuple(sorted(shape.items()))), scheme, read, oracle_lib), what)
    return res


@pytest.mark.parametrize("name", ["identity", "block", "root"])
@pytest.mark.parametrize("route", ROUTES, ids=[r[0] for r in ROUTES])
def test_exact_zeros_on_every_pruning_route(route, name, oracle_lib, monkeypatch):
    """Dead patterns come back as exactly -inf beside live ones held to 1e-10, no NaN in site values, partials or factors, no -8; zero
    partial entries exactly where the reference has them; an all-zero pattern's factor is log 1; and nothing derived from the dense
    matrices of the first evaluation survives their replacement (a stale cherry table would make the dead patterns live)."""
    res = run_route(route, name, oracle_lib, monkeypatch)
    assert res.lnl == -np.inf


@pytest.mark.parametrize("route", [r for r in ROUTES if r[0] in ("walk4-write", "walk4-read", "general7-write", "t32-write", "t32-read", "t64-read",
                                                                   "tiled20-levels", "general70-unscaled")], ids=lambda r: r[0])
def test_a_category_of_weight_zero_contributes_nothing(route, oracle_lib, monkeypatch):
    res = run_route(route, "weight", oracle_lib, monkeypatch)
    assert np.isfinite(res.lnl)


@pytest.mark.parametrize("P", [67, 1])
@pytest.mark.parametrize("route", ROUTES, ids=[r[0] for r in ROUTES])
def test_every_pattern_dead_and_a_single_dead_pattern(route, P, oracle_lib, monkeypatch):
    """No live pattern at all — every maximum the write-mode kernels take is 0 — and a buffer of one pattern, which is dead.  (Which kernel a
    list of one pattern runs on is the other tests' business: tests/test_gpu_parity.py test_small_and_ragged_shapes_on_the_walks.)"""
    res = run_route(route, "identity", oracle_lib, monkeypatch, assert_route=False, P=P, kind="all")
    assert res.lnl == -np.inf and np.isneginf(res.site).all()


# ---- one partitioned instance: dead patterns in one partition only ------------------------------------------------------------------

@pytest.mark.parametrize("always_rescale", [False, True])
@pytest.mark.parametrize("own_launch", [False, True])
def test_partitioned_instance_with_dead_patterns_in_one_partition(own_launch, always_rescale, oracle_lib, monkeypatch):
    """Two 4-state partitions through the ...ByPartition calls, the block-diagonal matrices injected for both, dead patterns in partition 0
    only: its sum is -inf, partition 1's is finite and follows the oracle, and so do the site values of both.  The roots are integrated
    by the top slices of the walk's launch (the default without rescaling: the scale-factor calls of a rescaling evaluation send a held walk
    off) and by k_rootSite4WParts, a launch of its own (BEAGLE_MI355_NO_ROOT_PARTS_FUSION=1, and every rescaling evaluation)."""
    from beast_mcmc_amd.inputs import synth
    from beast_mcmc_amd.multipartition import MultiPartitionTreeLikelihood
    if own_launch:
        monkeypatch.setenv("BEAGLE_MI355_NO_ROOT_PARTS_FUSION", "1")
    parts = [dc.case("block", 4, 4, P=131), dc.case("block", 4, 4, P=70, kind="live")]
    tree = parts[0].wl.tree
    assert all(np.array_equal(c.wl.tree.height, tree.height) and np.array_equal(c.wl.tree.left, tree.left) for c in parts)
    assert parts[0].dead.any() and not parts[1].dead.any()
    pw = synth.PartitionedWorkload("dead-in-one", tree, [c.wl for c in parts])
    tl = MultiPartitionTreeLikelihood(pw, always_rescale=always_rescale)
    by_part, total = tl.calculate()                              # the models' dense matrices
    assert np.isfinite(by_part).all()
    b, K, T = tl.b, 2, tree.tip_count
    for k, c in enumerate(parts):
        for n, m in c.mats.items():
            b.setTransitionMatrix(tl.mbuf(k, n), m, 1.0)
    ops9 = tl._ops[(int(tl.flip[T]), tl.mflip)][0]
    before = b.walkLaunchInfo()["partition_roots_in_walk"]
    b.updatePartialsByPartition(ops9, len(ops9) // 9)
    cum = (T - 1) if always_rescale else NONE
    if always_rescale:
        for k in range(K):
            b.resetScaleFactorsByPartition(cum, k)
            b.accumulateScaleFactorsByPartition(tl._scale_idx, len(tl._scale_idx), cum, k)
    for k, c in enumerate(parts):
        b.setCategoryWeights(k, c.wl.cat_weights)
        b.setStateFrequencies(k, c.wl.freqs)
    out, tot = np.zeros(K), np.zeros(1)
    ia = lambda v: np.ascontiguousarray(v, dtype=np.int32)
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    roots, rng_, cums = ia([tl.pbuf(tree.root)] * K), ia(range(K)), ia([cum] * K)
    rc = b._f["CalculateRootLogLikelihoodsByPartition"](b.instance, ip(roots), ip(rng_), ip(rng_), ip(cums), ip(rng_), K, 1, dp(out), dp(tot))
    fused = b.walkLaunchInfo()["partition_roots_in_walk"] - before
    st = b.walkStats()
    site = b.getSiteLogLikelihoods().copy()
    nodes = {n: b.getPartials(tl.pbuf(n), NONE).copy() for n in range(T, tree.node_count)}
    tl.close()
    assert rc == 0 and fused == (0 if own_launch or always_rescale else 1), (rc, fused)
    assert st["walks"] > 0 and st["fast_walks"] == st["walks"], st
    assert not np.isnan(site).any() and not np.isnan(out).any() and not any(np.isnan(x).any() for x in nodes.values())
    assert out[0] == -np.inf and np.isfinite(out[1]) and tot[0] == -np.inf
    off = 0
    for k, c in enumerate(parts):
        P = c.wl.pattern_count
        s = site[off:off + P]
        ref_site, ref_nodes = c.reference()
        ora = oracle_run(c, ("block", 4, 4, P), RESCALE_ALWAYS if always_rescale else RESCALE_NONE, False, oracle_lib)
        assert np.array_equal(np.isneginf(s), c.dead) and np.array_equal(np.isneginf(ora.site), c.dead)
        live = ~c.dead
        rs = ref_site[live].astype(np.float64)
        assert np.max(np.abs(s[live] - ora.site[live]) / np.abs(ora.site[live])) <= REL_TOL
        assert np.max(np.abs(s[live] - rs) / np.abs(rs)) <= REL_TOL
        for n in nodes:
            pg, po = nodes[n][:, off:off + P, :], ora.partials[n]
            assert np.array_equal(pg == 0.0, ref_nodes[n] == 0), (k, n)
            scale = np.maximum(np.abs(po).max(axis=(0, 2), keepdims=True), 1e-300)
            assert np.max(np.abs(pg - po) / scale) <= REL_TOL, (k, n)
        off += P
    assert helpers.rel_err(out[1], oracle_run(parts[1], ("block", 4, 4, 70), RESCALE_ALWAYS if always_rescale else RESCALE_NONE, False, oracle_lib).lnl) <= REL_TOL


# ---- DYNAMIC with delayed rescaling: -inf is an answer, not an underflow that a retry cures --------------------------------------------

def test_delayed_rescaling_returns_minus_infinity_once_and_recovers(oracle_lib):
    """Identity on both branches of every cherry as a chain meets it: cherry parents at height 0 under Kimura's three-parameter model, whose
    Hadamard eigenvectors make U exp(0) U^-1 the identity exactly (both sides read back, below), the simulated tips left to differ.  The
    first evaluation is -inf, the delayed scheme retries once with rescaling and -inf stays; the counters follow the oracle's; with the
    cherry parents back at their heights the next evaluation is finite again."""
    wl, restore = dc.k3st_dead_workload()
    tree = wl.tree
    g = BeagleTreeLikelihood(wl, rescaling=RESCALE_DYNAMIC, delay_rescaling=True)
    o = BeagleTreeLikelihood(wl, library=oracle_lib, rescaling=RESCALE_DYNAMIC, delay_rescaling=True)
    a, b = g.getLogLikelihood(), o.getLogLikelihood()
    assert a == -np.inf and b == -np.inf
    rg, ro = bm.beagle.Beagle.attach(g), bm.beagle.Beagle.attach(o)
    for n in restore:
        for c in (int(tree.left[n]), int(tree.right[n])):
            for raw, t in ((rg, g), (ro, o)):
                assert np.array_equal(raw.getTransitionMatrix(t.node_matrix_index(c)), np.broadcast_to(np.eye(4), (4, 4, 4)))
    sg, so = g.getSiteLogLikelihoods(), o.getSiteLogLikelihoods()
    assert not np.isnan(sg).any() and np.array_equal(np.isneginf(sg), np.isneginf(so)) and np.isneginf(so).any() and np.isfinite(so).any()
    live = np.isfinite(so)
    assert np.max(np.abs(sg[live] - so[live]) / np.abs(so[live])) <= REL_TOL
    cg, co = g.counters(), o.counters()
    assert cg["rescale_retries"] == co["rescale_retries"] == 1 and cg["ever_underflowed"] == co["ever_underflowed"] == 1
    for t in (g, o):
        for n, h in restore.items():
            t.set_node_height(n, h)
    a, b = g.getLogLikelihood(), o.getLogLikelihood()
    assert np.isfinite(b) and helpers.rel_err(a, b) <= REL_TOL
    sg, so = g.getSiteLogLikelihoods(), o.getSiteLogLikelihoods()
    assert np.max(np.abs(sg - so) / np.abs(so)) <= REL_TOL
    g.close(); o.close()


# ---- part B ------------------------------------------------------------------------------------------------------------------------

LENGTHS = [0.0, 1e-300, 1.0]


def _transition_matrices(S, lib, complex_eigen):
    from test_oracle_golden import _cyclic_model
    from beast_mcmc_amd.inputs import substmodel
    if complex_eigen:
        _, _, eig = _cyclic_model(S, 3 + S)
    elif S == 4:
        eig = substmodel.gtr([1.1, 2.3, 0.7, 1.4, 3.1, 1.0], [0.2, 0.3, 0.15, 0.35])
    else:
        eig = substmodel.random_reversible(S, np.random.default_rng(S))[0]
    b = bm.beagle.Beagle(3, 5, 3, S, 10, 2, 6, 2, 0, requirementFlags=bm.beagle.FLAG_EIGEN_COMPLEX if complex_eigen else 0, library=lib)
    out = []
    for rates in ([0.0, 1.0], [1.0, 0.0]):                   # a new eigen system and new rates in front of every update (4 states: one fused launch)
        b.setEigenDecomposition(0, eig.evec, eig.ievc, eig.evals)
        b.setCategoryRates(rates)
        b.updateTransitionMatrices(0, [0, 1, 2], None, None, LENGTHS, 3)
        out.append((rates, [b.getTransitionMatrix(m) for m in range(3)]))
    b.finalize()
    return out


@pytest.mark.parametrize("S,complex_eigen", [(4, False), (20, False), (61, False), (100, False), (4, True), (7, True)])
def test_transition_matrices_at_length_times_rate_zero(S, complex_eigen, oracle_lib):
    """Branch lengths {0, 1e-300, 1} x category rates {0, 1}: wherever the product is zero (1e-300: far below an ulp of any eigenvalue's
    exponent) the matrix is the identity to 1e-14 with no negative entry; everything within 1e-14 of the oracle."""
    got, want = _transition_matrices(S, None, complex_eigen), _transition_matrices(S, oracle_lib, complex_eigen)
    for (rates, gm), (_, om) in zip(got, want):
        for t, a, o in zip(LENGTHS, gm, om):
            assert not np.isnan(a).any()
            assert np.max(np.abs(a - o)) <= 1e-14, (S, rates, t)
            for c, r in enumerate(rates):
                if t * r == 0.0 or t == 1e-300:
                    assert (a[c] >= 0.0).all(), (S, rates, t, c, a[c].min())
                    assert np.max(np.abs(a[c] - np.eye(S))) <= 1e-14, (S, rates, t, c)


def _every_node(tl, wl):
    raw = bm.beagle.Beagle.attach(tl)
    return {n: raw.getPartials(tl.node_buffer_index(n), NONE).copy() for n in range(wl.tip_count, wl.tree.node_count)}


def _assert_same(g, o, wl, what):
    a, b = g.getLogLikelihood(), o.getLogLikelihood()
    sa, sb = g.getSiteLogLikelihoods(), o.getSiteLogLikelihoods()
    assert np.isfinite(b) and np.isfinite(sb).all(), what        # never -inf on both sides
    assert helpers.rel_err(a, b) <= REL_TOL, (what, a, b)
    assert np.max(np.abs(sa - sb) / np.abs(sb)) <= REL_TOL, what
    pg, po = _every_node(g, wl), _every_node(o, wl)
    for n in po:
        scale = np.maximum(np.abs(po[n]).max(axis=(0, 2), keepdims=True), 1e-300)
        assert not np.isnan(pg[n]).any() and np.max(np.abs(pg[n] - po[n]) / scale) <= REL_TOL, (what, n)


@pytest.mark.parametrize("scheme", [RESCALE_ALWAYS, RESCALE_NONE])
@pytest.mark.parametrize("S", [4, 7, 20, 61, 70])
def test_zero_length_cherries_and_a_rate_zero_category(S, scheme, oracle_lib):
    wl = dc.zero_length_workload(S)
    g = BeagleTreeLikelihood(wl, rescaling=scheme, delay_rescaling=False)
    o = BeagleTreeLikelihood(wl, library=oracle_lib, rescaling=scheme, delay_rescaling=False)
    _assert_same(g, o, wl, "S=%d scheme %d" % (S, scheme))
    g.makeDirty(); o.makeDirty()
    _assert_same(g, o, wl, "S=%d scheme %d, again" % (S, scheme))
    g.close(); o.close()


@pytest.mark.parametrize("scheme", [RESCALE_ALWAYS, RESCALE_DYNAMIC])
def test_a_node_moves_onto_its_child_and_back(scheme, oracle_lib):
    """4 states, partial updates: a node with a positive branch below it is lowered onto its higher child (that branch: length zero), then
    the move is rejected (restore) — and accepted the second time, and then moved up again."""
    wl = helpers.random_workload(9, 130, 4, 4, seed=5, unknown_fraction=0.02)
    tree = wl.tree
    g = BeagleTreeLikelihood(wl, rescaling=scheme, delay_rescaling=False)
    o = BeagleTreeLikelihood(wl, library=oracle_lib, rescaling=scheme, delay_rescaling=False)
    _assert_same(g, o, wl, "start")
    base = g.getLogLikelihood()
    inner = [n for n in range(tree.tip_count, tree.node_count) if n != tree.root and max(tree.left[n], tree.right[n]) >= tree.tip_count]
    for step, node in enumerate(inner[:3]):
        child = int(tree.left[node]) if tree.height[tree.left[node]] >= tree.height[tree.right[node]] else int(tree.right[node])
        low, old = float(tree.height[child]), float(tree.height[node])
        assert low > 0.0 and old > low
        for t in (g, o):
            t.storeState(); t.set_node_height(node, low)
        _assert_same(g, o, wl, "node %d on its child" % node)
        assert g.node_branch_time(child)[0] == 0.0 and g.counters()["last_op_count"] <= tree.depth()
        if step == 0:
            for t in (g, o):
                t.restoreState(); t.restore_node_height(node, old)
            _assert_same(g, o, wl, "restored")
            assert helpers.rel_err(g.getLogLikelihood(), base) <= 1e-12
        else:
            for t in (g, o):
                t.storeState(); t.set_node_height(node, old)
            _assert_same(g, o, wl, "node %d back up" % node)
    assert helpers.rel_err(g.getLogLikelihood(), base) <= 1e-12
    g.close(); o.close()


@pytest.mark.parametrize("S", [4, 20, 61])
def test_gradients_with_zero_length_edges(S, oracle_lib):
    """Gradient, diagonal second derivatives, per-pattern derivatives and cross products, the zero-length edges' own entries included."""
    wl = dc.zero_length_workload(S)
    g, o = BranchGradient(wl), BranchGradient(wl, library=oracle_lib)
    lo, go, ho, po = o.gradient(second=True, per_pattern=True)
    co = o.cross_products()
    assert all(np.isfinite(x).all() for x in (go, ho, po, co)) and sum(1 for n in o.edges if o.branch_lengths[n] == 0.0) >= 4
    for rep in range(2):                                     # (4 states: the second evaluation answers from the held pre-order list)
        lg, gg, hg, pg = g.gradient(second=True, per_pattern=True)
        cg = g.cross_products()
        assert helpers.rel_err(lg, lo) <= REL_TOL
        close(gg, go, "gradient")
        close(hg, ho, "second derivatives")
        close(pg, po, "per-pattern derivatives")
        close(cg, co, "cross products")
    g.close(); o.close()


# ---- part C ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("S", [4, 20, 61])
@pytest.mark.parametrize("factor,alpha", [r for r in dc.STIFF_REGIMES if r[0] >= 1.0])
def test_saturated_trees_and_a_vanishing_slowest_rate(factor, alpha, S, oracle_lib):
    """Heights x 80 (every matrix at stationarity to the last bit or nearly) and gamma shape 0.02 (slowest rate 2e-42): the fp64 oracle
    is within 2e-12 of its long-double mode there (tests/test_degenerate_host.py), so the suite's 1e-10 against it leaves room."""
    wl = dc.stiff_workload(S, factor, alpha)
    for scheme in (RESCALE_DYNAMIC, RESCALE_NONE):
        lo, so = dc.site_values(wl, oracle_lib, scheme)
        lg, sg = dc.site_values(wl, None, scheme)
        assert np.isfinite(lo) and np.isfinite(so).all()
        assert helpers.rel_err(lg, lo) <= REL_TOL and np.max(np.abs(sg - so) / np.abs(so)) <= REL_TOL, (scheme, lg, lo)


# Largest relative deviation of a site log-likelihood from the oracle's long-double mode at heights x 2e-6, measured on an MI355X (the
# test prints them):        S    alpha   |engine - precise|   |oracle - precise|
#                           4    0.05    2.19e-10             6.36e-10
#                           4    0.7     2.74e-10             1.42e-10
#                          20    0.05    1.15e-10             2.00e-10
#                          20    0.7     2.41e-10             2.80e-10
#                          61    0.05    5.55e-10             1.75e-09
#                          61    0.7     1.46e-09             9.68e-10
# No fixed bound against the fp64 oracle can be derived here: U exp(t Lambda) U^-1 at t ~ 1e-7 cancels to entries of 1e-7 from terms of order
# 1e-2, and the noise varies by small factors with the order of summation.  The cap is five times the larger measured deviation per state count.
SHORT_BRANCH_CAP = {4: 5 * 6.36e-10, 20: 5 * 2.80e-10, 61: 5 * 1.75e-09}


@pytest.mark.parametrize("S", [4, 20, 61])
@pytest.mark.parametrize("alpha", [0.05, 0.7])
def test_short_branches_against_the_precise_oracle(alpha, S, oracle_lib):
    wl = dc.stiff_workload(S, 2e-6, alpha)
    _, so = dc.site_values(wl, oracle_lib)
    _, sq = dc.site_values(wl, oracle_lib, precise=True)
    _, sg = dc.site_values(wl, None)
    assert np.isfinite(so).all() and np.isfinite(sq).all()
    de = float(np.max(np.abs(sg - sq) / np.abs(sq)))
    do = float(np.max(np.abs(so - sq) / np.abs(sq)))
    print("S=%d alpha=%g heights x 2e-6: |engine - precise| %.2e, |oracle - precise| %.2e" % (S, alpha, de, do))
    assert de <= 10.0 * do + 1e-12 and do <= 10.0 * de + 1e-12, (de, do)
    assert de <= SHORT_BRANCH_CAP[S] and do <= SHORT_BRANCH_CAP[S], (de, do)
