"""Sequence simulation on the GPU (include/beagle_mi355.h beagleMi355SimulateSequences, beast-mcmc_amd/simulate.py) against the host
restatement (tests/simulate_reference.py) over the branch matrices the engine reads back: states and categories must be IDENTICAL."""
import ctypes as C
import os

import numpy as np
import pytest

import beast_mcmc_amd as bm
import helpers
import simulate_cases as sc
import simulate_reference as sr
from beast_mcmc_amd.inputs import substmodel
from beast_mcmc_amd.simulate import SequenceSimulator
from beast_mcmc_amd.tipmodels import TipErrorModel
from beast_mcmc_amd.treelikelihood import BeagleTreeLikelihood

pytestmark = pytest.mark.gpu

_IP = C.POINTER(C.c_int)


def make(wl, **kw):
    tl = BeagleTreeLikelihood(wl, **kw)
    tl.workload = wl                      # (the model arrays the caller set: the restatement's category weights and frequencies)
    return tl


def raw_call(beagle, rows, site_count, w=0, f=0, seed=1, flags=0, root=None, cats=None, node_count=None, null_nodes=False,
             null_out=False, want_cats=True):
    """The C call itself -> (return code, states [1 + max outRow][site_count], categories)."""
    fn = beagle._ext("beagleMi355SimulateSequences", [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_ulonglong, C.c_int,
                                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p])
    rows = np.ascontiguousarray(rows, dtype=np.int32).reshape(-1, 3)
    n_out = max(1, int(rows[:, 0].max()) + 1)
    states = np.full((n_out, max(1, site_count)), 255, dtype=np.uint8)
    out_cats = np.full(max(1, site_count), -1, dtype=np.int32)
    root = None if root is None else np.ascontiguousarray(root, dtype=np.uint8)
    cats = None if cats is None else np.ascontiguousarray(cats, dtype=np.int32)
    rc = fn(beagle.instance, None if null_nodes else rows.ctypes.data, len(rows) if node_count is None else node_count, site_count, w, f,
            seed, flags, None if root is None else root.ctypes.data, None if cats is None else cats.ctypes.data,
            None if null_out else states.ctypes.data, out_cats.ctypes.data if want_cats else None)
    return rc, states, out_cats


def check_identical(beagle, rows, weights, freqs, site_count, seed, root=None, cats=None):
    """One call against the restatement: every wanted row and the categories, byte for byte; rows nobody wanted are left alone."""
    rc, states, out_cats = raw_call(beagle, rows, site_count, seed=seed, root=root, cats=cats)
    assert rc == 0
    ref, ref_cats, bad = sr.simulate_from_engine(beagle, rows, weights, freqs, seed, site_count, root_states=root, rate_categories=cats)
    assert not bad
    assert np.array_equal(out_cats, ref_cats)
    rows = np.asarray(rows).reshape(-1, 3)
    wanted = set()
    for r in range(len(rows)):
        if rows[r, 0] >= 0:
            wanted.add(int(rows[r, 0]))
            assert np.array_equal(states[rows[r, 0]], ref[r]), (r, np.flatnonzero(states[rows[r, 0]] != ref[r])[:5])
    for o in range(states.shape[0]):
        assert o in wanted or np.all(states[o] == 255)
    return states, out_cats


def all_variants(beagle, sim, wl, site_count, seed):
    """Tips only / every node, with and without the caller's root states and rate categories."""
    rng = np.random.default_rng(seed)
    root = rng.integers(0, wl.state_count, size=site_count).astype(np.uint8)
    cats = rng.integers(0, wl.category_count, size=site_count).astype(np.int32)
    out = None
    for ancestral in (False, True):
        rows, _ = sim.node_list(ancestral)
        for r, c in ((None, None), (root, None), (None, cats), (root, cats)):
            got = check_identical(beagle, rows, wl.cat_weights, wl.freqs, site_count, seed, root=r, cats=c)
            if ancestral and r is None and c is None:
                out = got
    return out


@pytest.mark.parametrize("S,C,T,sites,P", [
    (4, 4, 9, 257, 257),         # one more site than a multiple of four
    (4, 1, 40, 1000, 1000),      # deeper tree, one category
    (2, 2, 6, 1, 8),             # a single site: one thread, three of its four sites padding
    (7, 2, 6, 50, 50),           # up to 16 states: every table entry is compared
    (20, 2, 8, 100, 100),        # above: binary search
    (61, 1, 6, 70, 70),
    (4, 4, 9, 1027, 50),         # the site count has nothing to do with the instance's patterns
])
def test_states_equal_the_restatement(S, C, T, sites, P):
    wl = helpers.random_workload(T, P, S, C, seed=300 + S + T)
    tl = make(wl)
    tl.getLogLikelihood()                                   # (the caller's updateTransitionMatrices for every branch)
    sim = SequenceSimulator(tl)
    states, cats = all_variants(sim.beagle, sim, wl, sites, 4000 + S)
    assert states.max() < S
    if sites >= 50:
        assert len(np.unique(states)) > 1 and (C == 1 or len(np.unique(cats)) > 1)
    # the class returns the same bytes by tip and by node number
    tips, internal, c2 = sim.simulate(sites, 4000 + S, ancestral=True)
    assert np.array_equal(np.vstack([tips, internal]), states) and np.array_equal(c2, cats)
    tips2, none, _ = sim.simulate(sites, 4000 + S)
    assert none is None and np.array_equal(tips2, tips)
    tl.close()


def test_caterpillar_of_2000_tips():
    wl = helpers.random_workload(2000, 300, 4, 2, seed=77, tree_kind="caterpillar", root_to_tip=2.0)
    tl = make(wl)
    assert np.isfinite(tl.getLogLikelihood())
    sim = SequenceSimulator(tl)
    check_identical(sim.beagle, sim.node_list(True)[0], wl.cat_weights, wl.freqs, 300, 5)
    check_identical(sim.beagle, sim.node_list(False)[0], wl.cat_weights, wl.freqs, 300, 5)
    tl.close()


def tree_rows(tree, matrix_of_node=None):
    """{outRow = node, matrix = node (or the given map), parentRow} in pre-order for a bare instance whose matrix n is node n's branch."""
    order, stack = [], [tree.root]
    while stack:
        n = stack.pop()
        order.append(n)
        if n >= tree.tip_count:
            stack.append(int(tree.right[n])); stack.append(int(tree.left[n]))
    row_of = {n: r for r, n in enumerate(order)}
    rows = []
    for n in order:
        p = int(tree.parent[n])
        m = n if matrix_of_node is None else matrix_of_node.get(n, n)
        rows.append([n, 0 if p < 0 else m, -1 if p < 0 else row_of[p]])
    return np.asarray(rows, dtype=np.int32)


def bare_instance(wl, eig, freqs, flags=0, extra_matrices=0):
    """An instance on which nothing but the model setters and updateTransitionMatrices is ever called (Partition's use of BEAGLE)."""
    tree, S, Cn = wl.tree, len(freqs), wl.category_count
    b = bm.beagle.Beagle(tree.tip_count, tree.node_count, tree.tip_count, S, 16, 1, tree.node_count + extra_matrices, Cn, 0,
                         requirementFlags=flags)
    b.setEigenDecomposition(0, eig.evec, eig.ievc, eig.evals)
    b.setStateFrequencies(0, freqs)
    b.setCategoryRates(wl.cat_rates)
    b.setCategoryWeights(0, wl.cat_weights)
    nodes = [n for n in range(tree.node_count) if n != tree.root]
    b.updateTransitionMatrices(0, nodes, None, None, [tree.branch_length(n) for n in nodes], len(nodes))
    return b


def test_instance_that_only_ever_updated_its_matrices():
    wl = helpers.random_workload(12, 16, 4, 4, seed=12)
    b = bare_instance(wl, wl.eig, wl.freqs)
    rows = tree_rows(wl.tree)
    check_identical(b, rows, wl.cat_weights, wl.freqs, 777, 9)
    tips_only = rows.copy(); tips_only[rows[:, 0] >= wl.tree.tip_count, 0] = -1
    check_identical(b, tips_only, wl.cat_weights, wl.freqs, 777, 9)
    b.finalize()


@pytest.mark.parametrize("S", [4, 7])
def test_complex_eigen_model_and_convolved_matrices(S):
    rng = np.random.default_rng(40 + S)
    q = substmodel.complex_q(rng.uniform(0.02, 0.1, size=S * (S - 1)), S)
    for i in range(S):
        q[i, (i + 1) % S] += 2.0                           # a directed cycle: complex-conjugate eigenvalue pairs
    np.fill_diagonal(q, 0.0); np.fill_diagonal(q, -q.sum(axis=1))
    pi, eig = substmodel.decompose_complex(q)
    assert np.count_nonzero(eig.evals[S:]) >= 2
    wl = helpers.random_workload(7, 16, 4, 2, seed=5)       # (its tree and site model only)
    b = bare_instance(wl, eig, pi, flags=bm.beagle.FLAG_EIGEN_COMPLEX, extra_matrices=2)
    assert b.details.flags & bm.beagle.FLAG_EIGEN_COMPLEX
    n = wl.tree.node_count
    # an epoch branch: two nodes' branches take the product of two other matrices instead of their own
    b.convolveTransitionMatrices([0, 2], [1, 3], [n, n + 1], 2)
    rows = tree_rows(wl.tree, {4: n, 5: n + 1})
    M = b.getTransitionMatrix(n)
    assert not np.allclose(M[0], M[0].T, atol=1e-3) and np.allclose(M.sum(axis=2), 1.0, atol=1e-9)
    states, _ = check_identical(b, rows, wl.cat_weights, pi, 2000, 3)
    assert len(np.unique(states)) == S
    b.finalize()


def test_chunks_do_not_change_the_bytes(monkeypatch):
    wl = helpers.random_workload(9, 50, 4, 4, seed=313)
    tl = make(wl)
    tl.getLogLikelihood()
    sim = SequenceSimulator(tl)
    rows = sim.node_list(True)[0]
    rng = np.random.default_rng(1)
    root, cats = rng.integers(0, 4, size=1027).astype(np.uint8), rng.integers(0, 4, size=1027).astype(np.int32)
    whole = [raw_call(sim.beagle, rows, 1027, seed=8), raw_call(sim.beagle, rows, 1027, seed=8, root=root, cats=cats)]
    for chunk in ("64", "62", "1000"):                      # (62: rounded up to whole packed words)
        monkeypatch.setenv("BEAGLE_MI355_SIM_CHUNK_SITES", chunk)
        parts = [raw_call(sim.beagle, rows, 1027, seed=8), raw_call(sim.beagle, rows, 1027, seed=8, root=root, cats=cats)]
        for (rc0, s0, c0), (rc1, s1, c1) in zip(whole, parts):
            assert rc0 == 0 and rc1 == 0 and np.array_equal(s0, s1) and np.array_equal(c0, c1)
    monkeypatch.delenv("BEAGLE_MI355_SIM_CHUNK_SITES")
    tl.close()


def test_seeds():
    wl = helpers.random_workload(20, 64, 4, 4, seed=8)
    tl = make(wl)
    tl.getLogLikelihood()
    sim = SequenceSimulator(tl)
    a, _, ca = sim.simulate(500, 1)
    b, _, cb = sim.simulate(500, 1)
    c, _, cc = sim.simulate(500, 2)
    assert np.array_equal(a, b) and np.array_equal(ca, cb)
    assert not np.array_equal(a, c) and not np.array_equal(ca, cc)
    tl.close()


@pytest.fixture
def shards(request):
    n = getattr(request, "param", 0)
    old = os.environ.get("BEAGLE_MI355_SHARDS")
    if n:
        os.environ["BEAGLE_MI355_SHARDS"] = str(n)
    yield n
    if old is None:
        os.environ.pop("BEAGLE_MI355_SHARDS", None)
    else:
        os.environ["BEAGLE_MI355_SHARDS"] = old


@pytest.mark.parametrize("shards", [0, 3], indirect=True)
def test_sharded_handle_draws_what_one_instance_draws(shards):
    g = len(bm.beagle.engine().resource_list()) - 2
    wl = helpers.random_workload(40, 200, 4, 4, seed=901)
    single = make(wl)
    multi = make(wl, resource_list=(g + 1,))
    assert single.getLogLikelihood() == pytest.approx(multi.getLogLikelihood(), rel=1e-12)
    s1, s2 = SequenceSimulator(single), SequenceSimulator(multi)
    rng = np.random.default_rng(2)
    root, cats = rng.integers(0, 4, size=3001).astype(np.uint8), rng.integers(0, 4, size=3001).astype(np.int32)
    for kw in ({}, {"root_states": root, "rate_categories": cats}):
        a, ia, ca = s1.simulate(3001, 31, ancestral=True, **kw)
        b, ib, cb = s2.simulate(3001, 31, ancestral=True, **kw)
        assert np.array_equal(a, b) and np.array_equal(ia, ib) and np.array_equal(ca, cb)
    single.close(); multi.close()


def test_distribution_on_the_device():
    """The tree, seed and site count of tests/test_simulate_host.py against the engine's own site likelihoods of the 256 patterns."""
    tl = sc.tree_likelihood()
    assert np.isfinite(tl.getLogLikelihood())
    prob = np.exp(tl.getSiteLogLikelihoods())
    tips, _, cats = SequenceSimulator(tl).simulate(sc.N_SITES, sc.SEED)
    sc.check_distribution(tips, cats, prob)
    tl.close()


def test_the_instance_is_left_as_it_was():
    wl = helpers.random_workload(20, 500, 4, 4, seed=55)
    tl = make(wl)
    sim = SequenceSimulator(tl)
    before = tl.getLogLikelihood()
    tips, _, cats = sim.simulate(900, 17)
    assert tl.getLogLikelihood() == before
    tl.makeDirty()
    assert tl.getLogLikelihood() == before                  # bitwise
    # every tip gets a folded emission table: the caller's matrices, not the shadow slots the fold writes, are what is drawn from
    model = TipErrorModel(tl, wl.tip_states, base_rate=0.03)
    folded = tl.getLogLikelihood()
    assert folded != before
    st0 = model.raw.tipEmissionStats()
    assert st0["folded"] == wl.tip_count and st0["expanded"] == 0
    tips2, _, cats2 = sim.simulate(900, 17)
    assert np.array_equal(tips, tips2) and np.array_equal(cats, cats2)
    st1 = model.raw.tipEmissionStats()
    assert st1["folded"] == wl.tip_count and st1["expanded"] == 0 and st1["demotions"] == 0, st1
    tl.makeDirty()
    assert tl.getLogLikelihood() == folded
    st2 = model.raw.tipEmissionStats()
    assert st2["folded"] == wl.tip_count and st2["demotions"] == 0 and st2["fold_launches"] > st1["fold_launches"], st2
    # pattern partitions change nothing either
    sim.beagle.setPatternPartitions(2, (np.arange(wl.pattern_count) >= wl.pattern_count // 2).astype(np.int32))
    tips3, _, cats3 = sim.simulate(900, 17)
    assert np.array_equal(tips, tips3) and np.array_equal(cats, cats3)
    tl.close()


def test_round_trip_into_a_new_tree_likelihood():
    wl = helpers.random_workload(8, 100, 4, 4, seed=64)
    tl = make(wl)
    tl.getLogLikelihood()
    sim = SequenceSimulator(tl)
    tips, _, _ = sim.simulate(5000, 2027)
    pats, weights = sim.to_patterns(tips)
    assert pats.shape[0] == 8 and 1 < pats.shape[1] < 5000 and weights.sum() == 5000
    kw = dict(tree=wl.tree, tip_states=pats, weights=weights, eig=wl.eig, freqs=wl.freqs, cat_rates=wl.cat_rates,
              cat_weights=wl.cat_weights, state_count=4)
    again = BeagleTreeLikelihood(**kw)
    oracle = BeagleTreeLikelihood(library=helpers.oracle_library(), **kw)
    assert helpers.rel_err(again.getLogLikelihood(), oracle.getLogLikelihood()) <= 1e-10
    for t in (tl, again, oracle):
        t.close()


def test_error_codes():
    wl = helpers.random_workload(12, 64, 4, 2, seed=21)
    tl = make(wl)
    tl.getLogLikelihood()
    sim = SequenceSimulator(tl)
    b = sim.beagle
    rows, order = sim.node_list(True)
    n = 200
    assert raw_call(b, rows, n)[0] == 0
    assert raw_call(b, rows, n, want_cats=False)[0] == 0                # categories may be NULL
    assert raw_call(b, rows, n, null_nodes=True)[0] == -5
    assert raw_call(b, rows, n, null_out=True)[0] == -5
    assert raw_call(b, rows, n, node_count=0)[0] == -5
    assert raw_call(b, rows, 0)[0] == -5 and raw_call(b, rows, -3)[0] == -5
    assert raw_call(b, rows, n, w=7)[0] == -5 and raw_call(b, rows, n, w=-1)[0] == -5
    assert raw_call(b, rows, n, f=7)[0] == -5 and raw_call(b, rows, n, f=-1)[0] == -5
    bad = rows.copy(); bad[4, 1] = -1
    assert raw_call(b, bad, n)[0] == -5                                 # matrix
    bad = rows.copy(); bad[4, 1] = 10 ** 6
    assert raw_call(b, bad, n)[0] == -5
    bad = rows.copy(); bad[3, 2] = 5
    assert raw_call(b, bad, n)[0] == -5                                 # parent after its child
    bad = rows.copy(); bad[2, 2] = 2
    assert raw_call(b, bad, n)[0] == -5                                 # parent = itself
    bad = rows.copy(); bad[5, 2] = -1
    assert raw_call(b, bad, n)[0] == -5                                 # a second root
    bad = rows.copy(); bad[6, 0] = bad[2, 0]
    assert raw_call(b, bad, n)[0] == -5                                 # an outRow twice
    bad = rows.copy(); bad[6, 0] = -2
    assert raw_call(b, bad, n)[0] == -5
    assert raw_call(b, rows, n, flags=1)[0] == -5
    root = np.zeros(n, dtype=np.uint8); root[n - 1] = 4
    assert raw_call(b, rows, n, root=root)[0] == -5                     # an input state >= S
    cats = np.zeros(n, dtype=np.int32); cats[n - 1] = 2
    assert raw_call(b, rows, n, cats=cats)[0] == -5                     # an input category >= C
    cats[n - 1] = -1
    assert raw_call(b, rows, n, cats=cats)[0] == -5
    # -8: a row of zeros that is reached — those draws are 0, every other site keeps its bytes
    rc, clean, clean_cats = raw_call(b, rows, n, seed=17)
    assert rc == 0
    r = 3
    m, parent_out = int(rows[r, 1]), int(rows[rows[r, 2], 0])
    M = b.getTransitionMatrix(m).copy()
    M[:, 2, :] = 0.0
    b.setTransitionMatrix(m, M)
    rc, states, cats = raw_call(b, rows, n, seed=17)
    assert rc == -8
    ref, ref_cats, any_bad = sr.simulate_from_engine(b, rows, wl.cat_weights, wl.freqs, 17, n)
    assert any_bad and np.array_equal(cats, ref_cats)
    for k in range(len(rows)):
        assert np.array_equal(states[rows[k, 0]], ref[k])
    hit = clean[parent_out] == 2
    assert hit.any() and not hit.all()
    assert np.all(states[rows[r, 0]][hit] == 0)
    assert np.array_equal(states[:, ~hit], clean[:, ~hit]) and np.array_equal(cats, clean_cats)
    with pytest.raises(bm.beagle.BeagleException) as e:
        b.simulateSequences(rows, n, 0, 0, 17)
    assert e.value.code == -8
    tl.close()
