"""Every kernel family at 9, 16, 17 and 32 rate categories (tests/category_cases.py), on the HIP engine against the CPU oracle driven by
the same calls, and for the one-call entry points against the restatement each family's own GPU file uses, under that file's rule.

The engine picks kernels by category count: the 4-state walk's templates end at 4, 8 and 16 categories, the hold slots drop from three
to two above 8, and above 16 no instance is a walk instance (engine_create.cpp in->walk, in->walkT) — 4 states then run on
k_pruneGeneral over plain [C][P][4] buffers, 16..64 states on the level kernels.  Each likelihood and gradient test asserts the route
its instance took from the counters that exist (walkStats, walkLaunchInfo, gradientStats).

Every deviation a test measures is printed before it is asserted, as "category-deviation <family> C=<n> <value> (bound <b>)".
The checkers are the ones tests/test_category_counts_host.py runs on the oracle against an oracle with rolled category weights."""

import numpy as np
import pytest

import beast_mcmc_amd as bm
import category_cases as cc
import helpers
from beast_mcmc_amd.gradient import BranchGradient
from beast_mcmc_amd.treelikelihood import RESCALE_ALWAYS, RESCALE_DYNAMIC, RESCALE_NONE, BeagleTreeLikelihood

pytestmark = pytest.mark.gpu

NONE = bm.beagle.NONE
SCHEMES = {"none": RESCALE_NONE, "dynamic": RESCALE_DYNAMIC, "always": RESCALE_ALWAYS}


def report(family, C, worst, bound=cc.REL_TOL):
    for key in sorted(worst):
        print("category-deviation %s/%s C=%d %.3e (bound %.0e)" % (family, key, C, worst[key], bound))


def assert_route(S, C, stats, what, scheme="none"):
    """Which kernels answered, over a whole sequence.  4 states: the one-launch walk (walkLaunchInfo ticket_walks + flag_walks) up to 16
    categories, none above; 16..64 states: the T32 / T64 pattern walk (walkStats walks) up to 16 categories, the level kernels above —
    except that a list which rescales in write mode stays on that walk only up to 4 categories and 20 states (engine_levels.cpp:
    `!writes || in->walkTWrite`, kernels.h WALK_T32_WRITE_MAX_CATEGORIES), so under RESCALE_ALWAYS, where every list does, no walk runs
    at any count used here, and under RESCALE_DYNAMIC the walk serves the read-mode evaluations behind the first.  7 and 80 states run
    the general level kernel at every category count: no counter separates anything there, and the assertion is that no walk ran."""
    one_launch = stats["ticket_walks"] + stats["flag_walks"]
    if S == 4:
        assert (one_launch > 0) == (C <= 16), (what, stats)
        assert (stats["walks"] > 0) == (C <= 16), (what, stats)
    elif 16 <= S <= 64:
        assert (stats["walks"] > 0) == (C <= 16 and scheme != "always"), (what, stats)
        assert one_launch == 0, (what, stats)
    else:
        assert stats["walks"] == 0 and one_launch == 0, (what, stats)


# ---- 1. likelihood -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("scheme", sorted(SCHEMES))
@pytest.mark.parametrize("case", cc.likelihood_cases(), ids=cc.case_id)
def test_likelihood_sequence_matches_the_oracle(case, scheme, oracle_lib):
    """A full evaluation, two branch moves each followed by a restore, and a model move: after each of them lnL, every site value, every
    internal node's partials (per pattern, relative to its largest entry) and every scale buffer against the oracle at 1e-10; for one
    scheme per shape the site values against the long-double pruning reference over the matrices the engine itself reads back."""
    S, T, P, C = case
    wl = cc.workload(*case)
    what = "%s %s" % (cc.case_id(case), scheme)
    with_prune = sorted(SCHEMES)[cc.SHAPES.index((S, T, P)) % 3] == scheme
    stats = {}
    got = cc.run_sequence(wl, SCHEMES[scheme], matrices=with_prune, stats=stats)
    want = cc.run_sequence(wl, SCHEMES[scheme], library=oracle_lib)
    worst = {}
    try:
        cc.check_sequences(got, want, what, worst=worst)
        if with_prune:
            cc.check_against_prune(wl, got, what, worst=worst)
    finally:
        report("likelihood", C, worst)
    assert_route(S, C, stats, what, scheme)


@pytest.mark.parametrize("S,T,P", [(20, 8, 33), (61, 6, 37)])
def test_sixteen_and_seventeen_categories_take_different_kernels(S, T, P, oracle_lib):
    """The last count on the walks and the first off them, on the same shape: both match the oracle, and the walk counters are positive at
    16 and zero at 17.  (4 states: the likelihood cases above hold both counts and assert the same of each.)"""
    seen = {}
    for C in cc.CONTRAST:
        wl = cc.workload(S, T, P, C)
        stats = {}
        got = cc.run_sequence(wl, RESCALE_NONE, stats=stats)
        want = cc.run_sequence(wl, RESCALE_NONE, library=oracle_lib)
        worst = {}
        try:
            cc.check_sequences(got, want, "S=%d C=%d" % (S, C), worst=worst)
        finally:
            report("likelihood", C, worst)
        assert_route(S, C, stats, "S=%d C=%d" % (S, C))
        seen[C] = stats
    assert seen[16]["walks"] > 0 and seen[17]["walks"] == 0, seen


# ---- 2. transition matrices ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("S,C,cx", cc.matrix_cases(), ids=lambda v: str(v))
def test_transition_matrices_match_the_matrix_exponential(S, C, cx):
    """updateTransitionMatrices and updateTransitionMatricesWithMultipleModels (two eigen systems, two rate sets): every category's matrix
    within 1e-12 of scipy's expm(Q t r_c), and bit for bit the matrix of a call that names that branch alone."""
    models, rates, out = cc.run_matrices(S, C, cx)
    worst = {}
    try:
        cc.check_matrices(models, rates, out, "S=%d C=%d complex=%s" % (S, C, cx), worst=worst)
    finally:
        report("transition", C, worst, cc.MATRIX_TOL)


@pytest.mark.parametrize("C", [16, 17, 32])
@pytest.mark.parametrize("S,cx", [(4, False), (4, True)])
def test_matrices_right_behind_new_category_rates_use_the_new_rates(S, cx, C):
    """setCategoryRates and then updateTransitionMatrices with no call in between: the matrices are those of the new rates.  On a 4-state
    instance the launch may take its rates straight from the upload still queued in the host's staging ring (engine_abi.cpp:471-505);
    k_transition4Fused copies them from that source into LDS up to 16 categories and reads them from that source directly, in global
    memory, above 16.  No existing counter tells whether a call took the queued upload as its source or found it flushed already, so
    the route is not asserted: what is held is the result on either route.  Several times over, so that the ring's slots turn over."""
    import scipy.linalg
    (q, eig), _ = cc.matrix_models(S, cx)
    b = cc.matrix_instance(S, C, cx)
    try:
        b.setEigenDecomposition(0, eig.evec, eig.ievc, eig.evals)
        b.setCategoryRates(cc.transition_rates(C, 0))
        b.updateTransitionMatrices(0, [0], None, None, [0.4], 1)
        worst = 0.0
        for k in range(1, 5):
            rates = cc.transition_rates(C, k)
            b.setCategoryRates(rates)
            b.updateTransitionMatrices(0, [1, 2], None, None, [0.3, 1.1], 2)
            for m, t in ((1, 0.3), (2, 1.1)):
                got = b.getTransitionMatrix(m)
                for c in range(C):
                    worst = max(worst, float(np.max(np.abs(got[c] - scipy.linalg.expm(q * (t * rates[c]))))))
        print("category-deviation transition/queued-rates C=%d %.3e (bound %.0e)" % (C, worst, cc.MATRIX_TOL))
        assert worst <= cc.MATRIX_TOL
    finally:
        b.finalize()


# ---- 3. gradients --------------------------------------------------------------------------------------------------------------------

def expected_gradient_stats(S, C):
    """gradientStats() after the first evaluation, the second, the read of every pre-order partial, and the third (which asks for the
    per-pattern derivatives), as the code has them.
    4 states hold the list back at every category count (engine_preorder.cpp:196 in runPreOperations: S == 4, not tiled, no scale index
    -> holdPreList, :306; by_operation, statPreLists at :209, is behind that return).
      C <= 16: the first evaluation runs the list with the derivatives (fused), the second is answered by the pre-order walk and leaves
        the list held (walked), the read runs it (late), the third asks for per-pattern derivatives, which run the list first (late).
      C > 16: walkedGradient returns 1 at once (engine_preorder.cpp:513: `!in->walk || ... || in->C > 16`), so edgeDifferentials (:697-698)
        goes on to fusedGradient (:489, statFusedGradients at :506): every sums-only evaluation is fused and has run its list, so the
        read finds nothing held; the third asks for per-pattern derivatives (:695 `outDerivatives ? 1`), which run the list first
        (:699 executeHeldPre, statLateLists at :466): late.
    Other state counts go operation by operation: one list per evaluation."""
    zero = {"fused": 0, "by_operation": 0, "walked": 0, "late": 0}
    if S != 4:
        return [dict(zero, by_operation=n) for n in (1, 2, 2, 3)]
    if C <= 16:
        return [dict(zero, fused=1), dict(zero, fused=1, walked=1), dict(zero, fused=1, walked=1, late=1), dict(zero, fused=1, walked=1, late=2)]
    return [dict(zero, fused=1), dict(zero, fused=2), dict(zero, fused=2), dict(zero, fused=2, late=1)]


@pytest.mark.parametrize("rescale", [False, True], ids=["plain", "rescaled"])
@pytest.mark.parametrize("case", cc.GRADIENT_CASES, ids=cc.case_id)
def test_branch_gradient_matches_the_oracle(case, rescale, oracle_lib):
    """First and second derivatives, per-pattern derivatives, cross products (and their exact scaling direction) and every pre-order
    partial, over three evaluations, against the oracle at 1e-10; gradientStats() after each; log_likelihood() afterwards bit for bit what
    it was before them (with rescaling in the post-order pass: what it was before the last of them, category_cases.check_gradients)."""
    S, T, P, C = case
    wl = cc.gradient_workload(*case)
    g = BranchGradient(wl, rescale=rescale)
    o = BranchGradient(wl, rescale=rescale, library=oracle_lib)
    worst = {}
    try:
        stats = []
        got = cc.record_gradient(g, stats_after=stats)
        want = cc.record_gradient(o)
        try:
            cc.check_gradients(wl, got, want, cc.case_id(case), worst=worst, rescale=rescale)
        finally:
            report("gradient", C, worst)
        assert stats == expected_gradient_stats(S, C), stats
        launch = g.b.walkLaunchInfo()
        assert (launch["ticket_walks"] + launch["flag_walks"] > 0) == (S == 4 and C <= 16), launch
    finally:
        g.close(); o.close()


@pytest.mark.parametrize("case", cc.NODE_HEIGHT_CASES, ids=cc.case_id)
def test_node_height_derivatives_match_the_restatement_on_the_oracle(case, oracle_lib):
    """beagleMi355NodeHeightDerivatives against tests/node_height_reference.py on what the oracle reads back, as tests/test_gpu_node_height.py."""
    import node_height_reference as nr
    from beast_mcmc_amd.nodeheight import NodeHeightGradient
    S, T, P, C = case
    wl = cc.gradient_workload(*case)
    rates = np.random.default_rng(11 + T).uniform(0.5, 2.0, size=2 * T - 1)
    g, o = NodeHeightGradient(wl, rates=rates), NodeHeightGradient(wl, rates=rates, library=oracle_lib)
    try:
        lnl, first, second = g.derivatives()
        lo = o.prepare()
        fo, so = nr.from_plan(o)
        worst = {}
        try:
            cc.check_node_heights((lnl, first, second), (lo, fo, so), T, cc.case_id(case), worst=worst)
        finally:
            report("node-height", C, worst)
        rows, r = g.node_rows()
        again = g.b.nodeHeightDerivatives(rows, r, 0)
        assert np.array_equal(again[0], first) and np.array_equal(again[1], second)
        assert g.log_likelihood() == lnl
    finally:
        g.close(); o.close()


# ---- 4. one-call entry points ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("C", cc.COUNTS)
@pytest.mark.parametrize("S,T,P", cc.SAMPLER_SHAPES)
def test_ancestral_draws_equal_the_restatement(S, T, P, C):
    """sampleAncestralStates: the category draw over C weights, then the states — byte for byte (tests/test_gpu_ancestral.py)."""
    import test_gpu_ancestral as ta
    from beast_mcmc_amd.ancestral import AncestralStateSampler
    wl = cc.gradient_workload(S, T, P, C)                            # (uneven category weights)
    tl = ta.make(wl, rescaling=RESCALE_DYNAMIC, delay_rescaling=True)
    try:
        tl.getLogLikelihood()
        sampler = AncestralStateSampler(tl)
        for use_map in (False, True):
            states, cats = ta.check_identical(tl, sampler, 2024 + S + C, use_map)
        assert np.array_equal(states[:T][wl.tip_states < S], wl.tip_states[wl.tip_states < S])
        assert 0 <= cats.min() and cats.max() < C and len(np.unique(cats)) > 1
        assert C < 32 or cats.max() >= 16                            # the draw reaches past the sixteenth weight
    finally:
        tl.close()


@pytest.mark.parametrize("C", cc.COUNTS)
@pytest.mark.parametrize("S,T,P", cc.JUMP_SHAPES)
def test_markov_jumps_equal_the_restatement(S, T, P, C):
    """sampleMarkovJumps, integrated: the rule of tests/test_gpu_markov_jumps.py (1e-12 relative plus the row's floor)."""
    import test_gpu_markov_jumps as tm
    from beast_mcmc_amd.markovjumps import MarkovJumpsSampler
    wl = cc.gradient_workload(S, T, P, C)
    tl = tm.make(wl, branch_rate_seed=S, rescaling=RESCALE_DYNAMIC, delay_rescaling=True)
    try:
        s = tm.three_registers(MarkovJumpsSampler(tl), S, seed=S)
        for use_map in (False, True):
            res = tm.check_against_restatement(tl, s, 77 + S + C, use_map)
        assert np.all(res["jumps"][:, 0] == 0.0) and res["jumps"][0].sum() > 0.0
    finally:
        tl.close()


@pytest.mark.parametrize("C", cc.COUNTS)
@pytest.mark.parametrize("S,T,P", cc.JUMP_SHAPES)
def test_uniformized_jumps_equal_the_restatement(S, T, P, C):
    """sampleMarkovJumps with uniformization, one simulant and its history: the rule of tests/test_gpu_uniformized_jumps.py."""
    import test_gpu_uniformized_jumps as tu
    from beast_mcmc_amd.markovjumps import MarkovJumpsSampler
    wl = cc.gradient_workload(S, T, P, C)
    tl = tu.make(wl, branch_rate_seed=S, rescaling=RESCALE_DYNAMIC, delay_rescaling=True)
    try:
        s = tu.registers(MarkovJumpsSampler(tl), S, seed=S)
        res, ref = tu.check(tl, s, 77 + S + C, 1, True)
        assert np.all(res["jumps"][:, 0] == 0.0) and res["jumps"][0].sum() > 0.0
    finally:
        tl.close()


@pytest.mark.parametrize("C", cc.COUNTS)
@pytest.mark.parametrize("S,T", cc.SIMULATE_SHAPES)
def test_simulated_sequences_equal_the_restatement(S, T, C):
    """simulateSequences at 5 and 259 sites, tips only and every node, with and without the caller's root states and categories: bytes equal."""
    import test_gpu_simulate as ts
    from beast_mcmc_amd.simulate import SequenceSimulator
    wl = cc.gradient_workload(S, T, {4: 130, 61: 37}[S], C)
    tl = ts.make(wl)
    try:
        tl.getLogLikelihood()
        sim = SequenceSimulator(tl)
        for sites in cc.SIMULATE_SITES:
            states, cats = ts.all_variants(sim.beagle, sim, wl, sites, 4000 + S + C)
            assert states.max() < S and 0 <= cats.min() and cats.max() < C
        assert len(np.unique(cats)) > C // 2
    finally:
        tl.close()


@pytest.mark.parametrize("C", cc.COUNTS)
@pytest.mark.parametrize("S,T", cc.HISTORY_SHAPES)
def test_complete_histories_equal_the_restatement(S, T, C):
    """simulateCompleteHistories at 130 sites: states, categories, event counts, events' states and count registers exact, rewards and
    heights within the bound tests/test_gpu_complete_history.py derives."""
    import test_gpu_complete_history as th
    c, res = cc.history_case(S, T, C)
    b = th.instance_for(c)
    try:
        out = th.call(b, c)
        fr, fh = th.check_equal(out, res, c)
        print("category-deviation history/rewards C=%d %.3f of the bound; heights %.3f" % (C, fr, fh))
        assert len(np.unique(out["categories"])) > C // 2
    finally:
        b.finalize()


@pytest.mark.parametrize("C", cc.COUNTS)
@pytest.mark.parametrize("S", cc.DIFFERENTIAL_STATES)
def test_differential_matrices_match_the_restatement(S, C):
    """updateDifferentialMatrices, exact and first-order: the float64-loss ratio of tests/test_gpu_differential_matrices.py."""
    import test_gpu_differential_matrices as td
    case = td.reversible_case(S, C)
    try:
        case.guard()
        td.check_case(case, 1, False, td.EXACT)
        td.check_case(case, 7, True, td.EXACT)
        td.check_case(case, 3, True, td.FIRST_ORDER)
    finally:
        case.close()


@pytest.mark.parametrize("C", cc.COUNTS)
@pytest.mark.parametrize("S,T,P", cc.EMISSION_SHAPES)
def test_tip_emission_folds_bit_for_bit_and_matches_the_oracle(S, T, P, C, oracle_lib):
    """setTipEmission: bit for bit against compact tips on host-folded matrices, 1e-10 against the oracle given the expanded partials —
    the two checks of tests/test_gpu_tip_emission.py on its own builders at this shape."""
    import test_gpu_tip_emission as te
    shape = (S, T, P, C)
    te.test_fold_equals_compact_tips_on_host_folded_matrices_bit_for_bit(shape)
    te.test_parity_with_the_oracle_given_the_expanded_partials(shape, oracle_lib)


@pytest.mark.parametrize("use_map", [False, True], ids=["draw", "map"])
def test_robust_counts_at_seventeen_categories(use_map):
    """robustCounts over three 4-state instances, 10 tips, 64 sites, 17 categories: tests/test_gpu_robust_counts.py's 1e-12 + floor."""
    import test_gpu_robust_counts as tr
    case = tr.Case(10, 64, 17, seed=3)
    try:
        tr.check_against_restatement(case, use_map)
        for tl in case.tls:
            assert tl.category_count == 17
    finally:
        case.close()


# ---- 5. partitioned and sharded instances ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("S,K", [(4, 2), (4, 9), (20, 3), (61, 2)])
def test_partitioned_instance_at_seventeen_categories(S, K, oracle_lib):
    """One by-partition evaluation and one whole-range evaluation against the per-partition oracles at 1e-10."""
    from test_gpu_partition_sequences import Case
    c = Case(S, K, oracle_lib, C=17)
    try:
        assert all(len(w.cat_rates) == 17 for w in c.wls)
        c.update_by_partition()
        by, tot = c.root_by_partition()
        c.check_by_partition(by, tot, list(range(K)), c.eng.getSiteLogLikelihoods(), "by partition")
        c.matrices(1.07)
        c.update_by_partition()
        v = [0.0]
        c.eng.calculateRootLogLikelihoods([c.root()], [0], [0], [NONE], 1, v)
        c.check_whole(v[0], c.eng.getSiteLogLikelihoods(), "whole range")
        launch = c.eng.walkLaunchInfo()
        assert launch["ticket_walks"] + launch["flag_walks"] == 0 and c.eng.walkStats()["walks"] == 0       # off the walks
    finally:
        c.close()


@pytest.mark.parametrize("S,T,P", [(4, 12, 257), (20, 10, 130)])
def test_sharded_handle_at_seventeen_categories(S, T, P, oracle_lib, monkeypatch):
    """BEAGLE_MI355_SHARDS=3: the likelihood (1e-12, site values bit for bit) and one branch gradient (1e-10) equal a single instance's, the
    rules of tests/test_gpu_sharded_instance.py."""
    monkeypatch.setenv("BEAGLE_MI355_SHARDS", "3")
    rl = bm.beagle.engine().resource_list()
    g = len(rl) - 2
    assert "sharded" in rl[g + 1][0]                                 # resource g + 1 is the all-GPUs one (test_gpu_sharded_instance.py)
    wl = cc.gradient_workload(S, T, P, 17)
    single = BeagleTreeLikelihood(wl, rescaling=RESCALE_DYNAMIC, delay_rescaling=False)
    multi = BeagleTreeLikelihood(wl, rescaling=RESCALE_DYNAMIC, delay_rescaling=False, resource_list=(g + 1,))
    try:
        # the handle is the routing layer's, not an engine instance: setStream is a call only that layer refuses (engine_stats.cpp:20).
        # No existing counter reports how many shards it made.
        with pytest.raises(bm.beagle.BeagleException):
            bm.beagle.Beagle.attach(multi).setStream(None)
        bm.beagle.Beagle.attach(single).setStream(None)
        for step in range(2):
            a, b = single.getLogLikelihood(), multi.getLogLikelihood()
            assert helpers.rel_err(b, a) <= 1e-12, (step, a, b)
            assert np.array_equal(single.getSiteLogLikelihoods(), multi.getSiteLogLikelihoods())
            single.makeDirty(); multi.makeDirty()
    finally:
        single.close(); multi.close()
    one, many, o = BranchGradient(wl), BranchGradient(wl, resource_list=(g + 1,)), BranchGradient(wl, library=oracle_lib)
    try:
        r1, rm, ro = one.gradient(second=True), many.gradient(second=True), o.gradient(second=True)
        assert helpers.rel_err(rm[0], r1[0]) <= 1e-12 and helpers.rel_err(rm[0], ro[0]) <= 1e-10
        for a, b, c in zip(rm[1:], r1[1:], ro[1:]):
            assert np.max(np.abs(a - b)) <= 1e-10 * max(1.0, np.max(np.abs(b)))
            assert np.max(np.abs(a - c)) <= 1e-10 * max(1.0, np.max(np.abs(c)))
    finally:
        one.close(); many.close(); o.close()
