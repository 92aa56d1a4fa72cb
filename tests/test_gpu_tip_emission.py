"""Tip error models folded into the tip branch matrices on the device (include/beagle_mi355.h beagleMi355SetTipEmission).
A tip whose partials are the lookup E[code][state] is, with K <= S codes, a compact tip whose branch matrix is M E^T: the engine writes
those products into shadow matrix slots in front of every operation list (k_foldTipEmission) and everything behind that sees an ordinary
compact tip.  With K > S, and for every caller that needs a tip's partials as data, the device writes the partials buffer out
(k_expandTipEmission).  Checked against the CPU oracle on the stock route (setTipPartials of the expanded tables) at the project's
parity bound, 1e-10 relative, and bit for bit against the engine's own compact-tip and uploaded-partials paths.
Shapes, codes and tables: tests/tip_emission_cases.py."""
import ctypes as C

import numpy as np
import pytest

import beast_mcmc_amd as bm
import helpers
import tip_emission_cases as cases
from beast_mcmc_amd import tipmodels
from beast_mcmc_amd.ancestral import AncestralStateSampler
from beast_mcmc_amd.gradient import BranchGradient
from beast_mcmc_amd.treelikelihood import BeagleTreeLikelihood, RESCALE_NONE

pytestmark = pytest.mark.gpu
NONE = bm.beagle.NONE
REL_TOL = 1e-10          # tests/test_gpu_parity.py REL_TOL
Beagle, BeagleException = bm.beagle.Beagle, bm.beagle.BeagleException
_DP = C.POINTER(C.c_double)
S4, S20 = cases.SHAPES[0], cases.SHAPES[1]


def site_err(a, b):
    return float(np.max(np.abs(a - b) / np.abs(b)))


def oracle_tips(o, codes, tabs):
    """The stock route on the host driver: every tip's expanded partials, every node dirty."""
    for t in range(len(tabs)):
        p = np.ascontiguousarray(tipmodels.expand(codes[t], tabs[t]))
        assert o.h.btlSetTipPartials(o.ptr, t, p.ctypes.data_as(_DP)) == 0
    o.makeDirty()


def evaluate(g, fix=None, ops=None, matrices=True):
    """One evaluation on a BranchGradient's raw instance: matrices, (``fix``: the caller's own matrices), the list, the root."""
    if matrices:
        idx = g._nodes
        g.b.updateTransitionMatrices(0, g._edge_matrix[0], None, None, g.branch_lengths[idx], len(idx))
    if fix is not None:
        fix(g.b)
    ops = g._post_ops if ops is None else np.asarray(ops, dtype=np.int32)
    g.b.updatePartials(ops, len(ops) // 7, NONE)
    out = [0.0]
    g.b.calculateRootLogLikelihoods([g.tree.root], [0], [0], [NONE], 1, out)
    return out[0], g.b.getSiteLogLikelihoods().copy()


def same_bits(a, b, what):
    print(what, a[0], b[0], "largest site difference", float(np.max(np.abs(a[1] - b[1]))))
    assert a[0] == b[0], (what, a[0], b[0])
    assert np.array_equal(a[1], b[1]), what


# ---- 1. parity with the oracle on the stock route -------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", cases.SHAPES)
def test_parity_with_the_oracle_given_the_expanded_partials(shape, oracle_lib):
    wl, codes, _ = cases.workload(shape)
    T = shape[1]
    tl = BeagleTreeLikelihood(wl)
    raw = Beagle.attach(tl)
    o = BeagleTreeLikelihood(wl, library=oracle_lib)
    try:
        for step in range(3):
            if step == 0:                                    # codes and tables
                tabs = cases.tables(shape, 0.02)
                for t in range(T):
                    raw.setTipEmission(t, codes[t], tabs[t])
                tl.makeDirty()
                oracle_tips(o, codes, tabs)
            elif step == 1:                                  # a table-only update: a new base rate, the same operation list
                tabs = cases.tables(shape, 0.07)
                for t in range(T):
                    raw.setTipEmission(t, None, tabs[t])
                tl.makeDirty()
                oracle_tips(o, codes, tabs)
            else:                                            # new matrices under the same tables and the same list
                for x in (tl, o):
                    x.set_branch_rates(np.full(wl.tree.node_count, 1.07))
                    x.makeDirty()
            a, b = tl.getLogLikelihood(), o.getLogLikelihood()
            sa, sb = tl.getSiteLogLikelihoods(), o.getSiteLogLikelihoods()
            print(shape, "step", step, "lnL", a, b, "rel", helpers.rel_err(a, b), "site rel", site_err(sa, sb))
            assert helpers.rel_err(a, b) <= REL_TOL, (step, a, b)
            assert site_err(sa, sb) <= REL_TOL, step
        st = raw.tipEmissionStats()
        assert st["folded"] == T and st["expanded"] == 0 and st["demotions"] == 0 and st["fold_launches"] >= 3, st
        assert np.array_equal(raw.getTipStates(0), np.where(codes[0] < shape[0], codes[0], shape[0]))
    finally:
        tl.close()
        o.close()


def test_the_model_object_sends_tables_only_and_marks_the_tips(oracle_lib):
    """tipmodels.TipErrorModel on the 4-state shape: an error-rate move re-sends every tip's table, an indicator flip one tip's, and the
    evaluation behind each matches the oracle given the model's partials."""
    wl, codes, ages = cases.workload(S4)
    tl = BeagleTreeLikelihood(wl)
    o = BeagleTreeLikelihood(wl, library=oracle_lib)
    try:
        model = tipmodels.TipErrorModel(tl, codes, tipmodels.ALL_SUBSTITUTIONS, base_rate=0.02, age_rate=0.3, tip_ages=ages,
                                        excluded=[t == 1 for t in range(S4[1])])

        def check(what):
            for t in range(S4[1]):
                p = np.ascontiguousarray(model.partials(t))
                assert o.h.btlSetTipPartials(o.ptr, t, p.ctypes.data_as(_DP)) == 0
            o.makeDirty()
            a, b = tl.getLogLikelihood(), o.getLogLikelihood()
            assert helpers.rel_err(a, b) <= REL_TOL, (what, a, b)
            assert site_err(tl.getSiteLogLikelihoods(), o.getSiteLogLikelihoods()) <= REL_TOL, what
        check("first")
        model.set_rates(base_rate=0.06)
        check("base rate")
        assert tl.counters()["last_op_count"] == S4[1] - 1
        model.set_indicator(3, False)
        check("indicator")
        assert 0 < tl.counters()["last_op_count"] < S4[1] - 1          # the tip's path to the root only
        assert model.raw.tipEmissionStats()["folded"] == S4[1]
    finally:
        tl.close()
        o.close()


# ---- 2. the fold, bit for bit ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [S4, S20])
def test_fold_equals_compact_tips_on_host_folded_matrices_bit_for_bit(shape):
    wl, codes, _ = cases.workload(shape)
    T = shape[1]
    tabs = cases.tables(shape, 0.03)
    x, y = BranchGradient(wl), BranchGradient(wl)            # (y: plain compact tips, the codes as states)
    try:
        for t in range(T):
            x.b.setTipEmission(t, codes[t], tabs[t])

        def host_fold(b):
            for t in range(T):
                b.setTransitionMatrix(t, tipmodels.fold(b.getTransitionMatrix(t), tabs[t]))
        for k in range(3):                                   # a first list, then replays of the cached plan
            same_bits(evaluate(x), evaluate(y, fix=host_fold), ("fold", shape, k))
        assert x.b.tipEmissionStats()["fold_launches"] == 3
    finally:
        x.close()
        y.close()


# ---- 3. the expansion, bit for bit -------------------------------------------------------------------------------------------------
def test_more_codes_than_states_are_expanded_bit_for_bit():
    wl, codes, _ = cases.workload(S4)
    T, P = S4[1], S4[2]
    rng = np.random.default_rng(77)
    states = np.where(codes < 4, codes, 16)                                          # alignment coding: 16 = unknown
    states[(rng.random(states.shape) < 0.1) & (states == 0)] = tipmodels.HYPERMUTANT_CONTEXT_STATE
    c5 = np.stack([tipmodels.hypermutant_codes(states[t]) for t in range(T)])
    assert (c5 == 4).any() and (c5 < 0).any()
    tabs = [tipmodels.hypermutant_emission(0.3 + 0.01 * t, t % 2 == 0) for t in range(T)]
    x, y = BranchGradient(wl), BranchGradient(wl)
    try:
        for t in range(T):
            x.b.setTipEmission(t, c5[t], tabs[t])
            y.b.setTipPartials(t, tipmodels.expand(c5[t], tabs[t]))
        for k in range(2):
            same_bits(evaluate(x), evaluate(y), ("expand", k))
        st = x.b.tipEmissionStats()
        assert st == {"folded": 0, "expanded": T, "fold_launches": 0, "demotions": 0}, st
        assert np.array_equal(x.b.getPartials(2), np.broadcast_to(tipmodels.expand(c5[2], tabs[2]), (S4[3], P, 4)))
        tabs[2] = tipmodels.hypermutant_emission(0.9, True)                         # a table-only update of an expanded tip
        x.b.setTipEmission(2, None, tabs[2])
        y.b.setTipPartials(2, tipmodels.expand(c5[2], tabs[2]))
        same_bits(evaluate(x), evaluate(y), "expand, new table")
    finally:
        x.close()
        y.close()


# ---- 4. the fast path is kept ------------------------------------------------------------------------------------------------------
def test_folded_tips_keep_the_compact_tip_programs(monkeypatch):
    """4 states, every tip folded, against plain compact tips on the same alignment and lists: the same micro-operations, stored nodes, tip
    and memory reads, the same clades served from class tables, and one fold launch per updatePartials call."""
    monkeypatch.setenv("BEAGLE_MI355_REPEATS_ANY_SIZE", "1")      # (the class tables are off at this size otherwise)
    monkeypatch.setenv("BEAGLE_MI355_MEM_DEF_STEPS", "8")
    wl = helpers.random_workload(24, 300, 4, 4, seed=424, unknown_fraction=0.1, root_to_tip=0.15)
    T = 24
    tabs = [cases.table(4, 0.02, 0.1 * t) for t in range(T)]
    x, y = BeagleTreeLikelihood(wl, rescaling=RESCALE_NONE), BeagleTreeLikelihood(wl, rescaling=RESCALE_NONE)
    try:
        rx, ry = Beagle.attach(x), Beagle.attach(y)
        for t in range(T):
            rx.setTipEmission(t, wl.tip_states[t], tabs[t])
        stats = []
        for tl, raw in ((x, rx), (y, ry)):
            for k in range(4):
                tl.makeDirty(); tl.getLogLikelihood()
            raw.kernelTimer(True)
            launches0 = raw.tipEmissionStats()["fold_launches"]
            for k in range(3):
                tl.makeDirty(); tl.getLogLikelihood()
            stats.append((raw.walkStats(), raw.repeatStats(), raw.tipEmissionStats()["fold_launches"] - launches0))
            raw.kernelTimer(False)
        (wx, repx, fx), (wy, repy, fy) = stats
        print("walk", wx, wy, "repeats", repx, repy)
        for key in ("micro_ops", "stored", "tip_reads", "mem_reads", "walks", "fast_walks"):
            assert wx[key] == wy[key], (key, wx, wy)
        for key in ("table_rows", "table_reads", "repeat_clades", "two_table_nodes"):
            assert repx[key] == repy[key], (key, repx, repy)
        assert repy["repeat_clades"] > 0 and wy["tip_reads"] > 0
        assert fx == 3 and fy == 0
    finally:
        x.close()
        y.close()


# ---- 5. a partial update -----------------------------------------------------------------------------------------------------------
def test_one_table_changes_and_only_its_path_is_recomputed():
    shape = cases.SHAPES[4]
    wl, codes, _ = cases.workload(shape)
    T, tree = shape[1], wl.tree
    tabs = cases.tables(shape, 0.02)
    tip = 2
    new = cases.table(4, 0.2, 1.1)
    path, n = set(), int(tree.parent[tip])
    while n >= 0:
        path.add(n); n = int(tree.parent[n])
    x, z = BranchGradient(wl), BranchGradient(wl)
    try:
        for t in range(T):
            x.b.setTipEmission(t, codes[t], tabs[t])
            z.b.setTipEmission(t, codes[t], new if t == tip else tabs[t])
        evaluate(x)
        x.b.setTipEmission(tip, None, new)
        ops = x._post_ops.reshape(-1, 7)
        ops = ops[[int(r[0]) in path for r in ops]]
        assert 0 < len(ops) < T - 1 or T - 1 == len(path)
        same_bits(evaluate(x, ops=ops.ravel(), matrices=False), evaluate(z), "partial update")
    finally:
        x.close()
        z.close()


# ---- 6. callers that need the tips' partials as data -------------------------------------------------------------------------------
def test_a_gradient_pass_demotes_the_tips_and_matches_the_uploaded_partials(oracle_lib):
    wl, codes, _ = cases.workload(S4)
    T, P, Cn = S4[1], S4[2], S4[3]
    tabs = cases.tables(S4, 0.04)
    x, y = BranchGradient(wl), BranchGradient(wl)
    o = BeagleTreeLikelihood(wl, library=oracle_lib, rescaling=RESCALE_NONE)
    try:
        for t in range(T):
            x.b.setTipEmission(t, codes[t], tabs[t])
            y.b.setTipPartials(t, tipmodels.expand(codes[t], tabs[t]))
        assert x.b.tipEmissionStats()["folded"] == T
        lx, gx = x.gradient()
        ly, gy = y.gradient()
        st = x.b.tipEmissionStats()
        assert st["demotions"] == T and st["folded"] == 0 and st["expanded"] == T, st
        scale = max(1.0, float(np.max(np.abs(gy))))          # tests/test_gpu_gradients.py close()
        print("lnL", lx, ly, "gradient error", float(np.max(np.abs(gx - gy))) / scale)
        assert helpers.rel_err(lx, ly) <= REL_TOL
        assert float(np.max(np.abs(gx - gy))) / scale <= REL_TOL
        oracle_tips(o, codes, tabs)
        expect = o.getLogLikelihood()
        assert helpers.rel_err(x.log_likelihood(), expect) <= REL_TOL       # the next likelihood, on the expanded tips
        for t in (0, T - 1):
            assert np.array_equal(x.b.getPartials(t), np.broadcast_to(tipmodels.expand(codes[t], tabs[t]), (Cn, P, 4)))
        tabs2 = cases.tables(S4, 0.09)                       # a demoted tip is written out again when its table changes
        for t in range(T):
            x.b.setTipEmission(t, None, tabs2[t])
        oracle_tips(o, codes, tabs2)
        assert helpers.rel_err(x.log_likelihood(), o.getLogLikelihood()) <= REL_TOL
        assert x.b.tipEmissionStats()["expanded"] == T
        x.b.setTipEmission(0, codes[0], tabs2[0])            # ... until a call with codes chooses the route again
        assert x.b.tipEmissionStats()["folded"] == 1
        assert helpers.rel_err(x.log_likelihood(), o.getLogLikelihood()) <= REL_TOL
    finally:
        x.close()
        y.close()
        o.close()


@pytest.mark.parametrize("shape", [S4, S20])
def test_get_partials_and_the_ancestral_sampler_demote(shape, oracle_lib):
    wl, codes, _ = cases.workload(shape)
    S, T, P, Cn = shape
    tabs = cases.tables(shape, 0.04)
    tl = BeagleTreeLikelihood(wl)
    o = BeagleTreeLikelihood(wl, library=oracle_lib)
    try:
        raw = Beagle.attach(tl)
        for t in range(T):
            raw.setTipEmission(t, codes[t], tabs[t])
        tl.makeDirty()
        tl.getLogLikelihood()
        assert np.array_equal(raw.getPartials(1), np.broadcast_to(tipmodels.expand(codes[1], tabs[1]), (Cn, P, S)))
        st = raw.tipEmissionStats()
        assert st["demotions"] == 1 and st["folded"] == T - 1, st
        states, cats = AncestralStateSampler(tl).sample(seed=5)
        assert states.shape == (wl.tree.node_count, P) and int(states.max()) < S
        st = raw.tipEmissionStats()
        assert st["demotions"] == T and st["folded"] == 0 and st["expanded"] == T, st
        oracle_tips(o, codes, tabs)
        tl.makeDirty()
        a, b = tl.getLogLikelihood(), o.getLogLikelihood()
        assert helpers.rel_err(a, b) <= REL_TOL, (a, b)
        assert site_err(tl.getSiteLogLikelihoods(), o.getSiteLogLikelihoods()) <= REL_TOL
    finally:
        tl.close()
        o.close()


# ---- 7. one matrix index for two folded tips ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [S4, cases.SHAPES[3]])
def test_a_list_that_shares_a_matrix_between_two_folded_tips(shape):
    wl, codes, _ = cases.workload(shape)
    T, tree = shape[1], wl.tree
    tabs = cases.tables(shape, 0.04)
    x, y = BranchGradient(wl), BranchGradient(wl)
    try:
        for t in range(T):
            x.b.setTipEmission(t, codes[t], tabs[t])
            y.b.setTipPartials(t, tipmodels.expand(codes[t], tabs[t]))
        ops = x._post_ops.reshape(-1, 7).copy()
        row = next(r for r in ops if r[3] < T and r[5] < T)          # a node over two tips: both branches read the first one's matrix
        a, b = int(row[3]), int(row[5])
        row[6] = row[4]
        lx, sx = evaluate(x, ops=ops.ravel())
        ly, sy = evaluate(y, ops=ops.ravel())
        print("shared matrix", shape, lx, ly)
        assert helpers.rel_err(lx, ly) <= REL_TOL and site_err(sx, sy) <= REL_TOL
        st = x.b.tipEmissionStats()
        assert st["demotions"] == 2 and st["folded"] == T - 2 and st["expanded"] == 2, st
        other = next(r for r in ops if (r[3] < T) != (r[5] < T) and int(r[3] if r[3] < T else r[5]) not in (a, b))
        if other[3] < T:                                     # ... and a folded tip sharing its matrix with an internal child
            other[4] = other[6]
        else:
            other[6] = other[4]
        lx, sx = evaluate(x, ops=ops.ravel())
        ly, sy = evaluate(y, ops=ops.ravel())
        assert helpers.rel_err(lx, ly) <= REL_TOL and site_err(sx, sy) <= REL_TOL
        assert x.b.tipEmissionStats()["demotions"] == 3
    finally:
        x.close()
        y.close()


# ---- 8. a partitioned instance, plain and sharded ----------------------------------------------------------------------------------
def _partitioned(tree, wls, tabs, route, resource_list):
    T, K = tree.tip_count, len(wls)
    P = sum(w.pattern_count for w in wls)
    nodes = 2 * T - 1
    b = Beagle(T, T + (T - 1), T, 4, P, K, K * nodes, 4, 0, resourceList=resource_list)
    try:
        for t in range(T):
            c = np.concatenate([w.tip_states[t] for w in wls])
            if route == "emission":
                b.setTipEmission(t, c, tabs[t])
            else:
                b.setTipPartials(t, tipmodels.expand(c, tabs[t]))
        b.setPatternWeights(np.concatenate([w.weights for w in wls]))
        b.setPatternPartitions(K, np.concatenate([np.full(w.pattern_count, k, dtype=np.int32) for k, w in enumerate(wls)]))
        eig_idx, rate_idx, mat_idx, lens = [], [], [], []
        for k, w in enumerate(wls):
            b.setEigenDecomposition(k, w.eig.evec, w.eig.ievc, w.eig.evals)
            b.setCategoryRatesWithIndex(k, w.cat_rates)
            b.setCategoryWeights(k, w.cat_weights)
            b.setStateFrequencies(k, w.freqs)
            for n in range(nodes):
                if n != tree.root:
                    eig_idx.append(k); rate_idx.append(k); mat_idx.append(k * nodes + n); lens.append(tree.branch_length(n))
        ops = []
        for n in tree.postorder():
            if n >= T:
                l, r = int(tree.left[n]), int(tree.right[n])
                for k in range(K):
                    ops += [n, NONE, NONE, l, k * nodes + l, r, k * nodes + r, k, NONE]
        out = []
        for rep in range(2):
            b.updateTransitionMatricesWithMultipleModels(eig_idx, rate_idx, mat_idx, None, None, lens, len(lens))
            b.updatePartialsByPartition(ops, len(ops) // 9)
            by_part, total = np.zeros(K), [0.0]
            b.calculateRootLogLikelihoodsByPartition([tree.root] * K, list(range(K)), list(range(K)), [NONE] * K, list(range(K)), K, 1,
                                                     by_part, total)
            out.append((by_part.copy(), total[0], b.getSiteLogLikelihoods().copy()))
        stats = b.tipEmissionStats()
    finally:
        b.finalize()
    return out, stats


@pytest.mark.parametrize("shards", [0, 3])
def test_partitioned_instance_by_partition_tuples(shards, monkeypatch):
    tree, wls = helpers.two_partitions(4, 9, [150, 77], seed=44)
    T = tree.tip_count
    rng = np.random.default_rng(6)
    for w in wls:
        w.tip_states[rng.random(w.tip_states.shape) < 0.1] = 4
    tabs = [cases.table(4, 0.03, 0.2 * t) for t in range(T)]
    rl = [1]
    if shards:
        monkeypatch.setenv("BEAGLE_MI355_SHARDS", str(shards))
        rl = [len(bm.beagle.engine().resource_list()) - 1]               # the sharded handle
    got, st = _partitioned(tree, wls, tabs, "emission", rl)
    expect, _ = _partitioned(tree, wls, tabs, "partials", [1])
    assert st["folded"] == T and st["fold_launches"] == 2 and st["demotions"] == 0, st
    for (pa, ta, sa), (pb, tb, sb) in zip(got, expect):
        print("partitioned, shards", shards, ta, tb)
        assert helpers.rel_err(ta, tb) <= REL_TOL
        assert np.max(np.abs(pa - pb) / np.abs(pb)) <= REL_TOL and site_err(sa, sb) <= REL_TOL


# ---- 9. errors ---------------------------------------------------------------------------------------------------------------------
def test_errors_and_dropping_an_emission():
    wl, codes, _ = cases.workload(cases.SHAPES[4])
    T = cases.SHAPES[4][1]
    g = BranchGradient(wl)
    try:
        e = np.eye(4)
        with pytest.raises(BeagleException) as err:
            g.b.setTipEmission(0, None, e)                   # no codes yet
        assert err.value.code == -5
        f = g.b._ext("beagleMi355SetTipEmission", [C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int, _DP])
        big = np.ones((256, 4))
        c = np.ascontiguousarray(codes[0], dtype=np.int32)
        for K in (0, 256):
            assert f(g.b.instance, 0, c.ctypes.data_as(C.POINTER(C.c_int)), K, big.ctypes.data_as(_DP)) == -5
        for tip in (-1, T):
            assert f(g.b.instance, tip, c.ctypes.data_as(C.POINTER(C.c_int)), 4, big.ctypes.data_as(_DP)) == -5
        assert g.b.tipEmissionStats() == {"folded": 0, "expanded": 0, "fold_launches": 0, "demotions": 0}
        g.b.setTipEmission(0, codes[0], e)
        g.b.setTipEmission(1, codes[1], np.ones((255, 4)))               # the largest table: expanded
        assert g.b.tipEmissionStats()["folded"] == 1 and g.b.tipEmissionStats()["expanded"] == 1
        with pytest.raises(BeagleException) as err:
            g.b.setTipEmission(0, None, np.ones((3, 4)))     # another size than the codes came with
        assert err.value.code == -5
        g.b.setTipStates(0, codes[0])                        # the tip is the caller's again
        g.b.setTipPartials(1, np.ones((cases.SHAPES[4][2], 4)))
        assert g.b.tipEmissionStats()["folded"] == 0 and g.b.tipEmissionStats()["expanded"] == 0
        with pytest.raises(BeagleException) as err:
            g.b.setTipEmission(0, None, e)
        assert err.value.code == -5
    finally:
        g.close()
    b = Beagle(4, 8, 4, 3, 1, 1, 8, 1, 0)
    try:
        b.allocateCoalescentBuffers(5, 8, 8, 1)
        with pytest.raises(BeagleException) as err:
            b.setTipEmission(0, [0], np.eye(3))
        assert err.value.code == -7
    finally:
        b.finalize()
