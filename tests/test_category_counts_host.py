"""CPU tier of the rate-category counts 9, 16, 17 and 32 (tests/category_cases.py): the CPU oracle against the long-double pruning
reference at every shape and count of the GPU file, its gradients against finite differences of its own log-likelihood, the builders'
outputs, and the checkers of the GPU file that category_cases.py holds — the likelihood sequence, the pruning reference, the transition
matrices, the gradients, the node-height derivatives — run on an oracle evaluation whose category weights (for the transition matrices,
which read no weights: whose category rates) are rolled by one position: each must then fail, so a checker that looks at nothing shows
without a GPU.  Category weights reach neither partials nor scale buffers, so each comparison of the likelihood checker is also shown to
fire on its own, on a copy of the oracle's record with that one quantity moved by 1e-9.
Not perturbed here: the one-call entry points (their checkers are their own GPU files', and the oracle has none of those calls), the
partitioned and the sharded tests."""
import copy

import numpy as np
import pytest

import category_cases as cc
from beast_mcmc_amd.gradient import BranchGradient
from beast_mcmc_amd.treelikelihood import RESCALE_ALWAYS, RESCALE_NONE


@pytest.mark.parametrize("case", cc.likelihood_cases(), ids=cc.case_id)
def test_oracle_agrees_with_the_long_double_pruning_reference(case, oracle_lib):
    """Site values of every step of the recorded sequence (first evaluation, two branch moves with their restores, a model move) to 1e-12
    relative, the bound of tests/test_degenerate_host.py."""
    wl = cc.workload(*case)
    steps = cc.run_sequence(wl, RESCALE_NONE, library=oracle_lib, matrices=True)
    worst = cc.check_against_prune(wl, steps, cc.case_id(case), tol=cc.ORACLE_TOL)
    print("%s: oracle against reference_prune %.2e" % (cc.case_id(case), worst["prune"]))


@pytest.mark.parametrize("S,T,P,C", [(4, 10, 130, 17), (4, 10, 130, 32), (20, 8, 33, 17), (20, 8, 33, 32)])
def test_oracle_gradient_matches_finite_differences(S, T, P, C, oracle_lib):
    """The rule of test_gpu_gradients.test_gradient_matches_finite_differences_on_the_engine: central differences at h = 1e-4 t, within
    1e-5 max(1, |g|) plus the rounding noise of the two log-likelihoods."""
    wl = cc.gradient_workload(S, T, P, C)
    g = BranchGradient(wl, library=oracle_lib)
    lnl, grad = g.gradient()
    for n in g.edges[:6]:
        t = g.branch_lengths[n]
        h = 1e-4 * t
        g.set_branch_length(n, t + h); up = g.log_likelihood()
        g.set_branch_length(n, t - h); dn = g.log_likelihood()
        g.set_branch_length(n, t)
        noise = 50 * np.finfo(float).eps * abs(lnl) / h
        assert abs((up - dn) / (2 * h) - grad[n]) <= 1e-5 * max(1.0, abs(grad[n])) + noise, n
    g.close()


def test_builders_stay_inside_the_listed_shapes_and_counts():
    shapes = set(cc.SHAPES)
    assert len(shapes) == 8 and set(cc.COUNTS) | set(cc.CONTRAST) == {9, 16, 17, 32}
    cases = cc.likelihood_cases()
    assert len(cases) == 6 * 3 + 2 * 4
    for S, T, P, C in cases + cc.GRADIENT_CASES + cc.NODE_HEIGHT_CASES:
        assert (S, T, P) in shapes and C in (9, 16, 17, 32)
        assert C != 16 or S == 4
    for case in cases:
        wl = cc.workload(*case)
        S, T, P, C = case
        assert (wl.state_count, wl.tip_count, wl.pattern_count, wl.category_count) == case
        assert wl.tip_states.shape == (T, P) and 0.0 < (wl.tip_states >= S).mean() < 0.15      # some unknown states, not many
        for rates, weights in ((wl.cat_rates, wl.cat_weights), cc.second_model(wl)[2:]):
            assert len(rates) == len(weights) == C
            assert abs(float(np.sum(weights)) - 1.0) <= 1e-12 and (np.asarray(weights) > 0).all()
            assert (np.asarray(rates) > 0).all() and np.isfinite(rates).all()
    for C in (9, 16, 17, 32):
        w = cc.uneven_weights(C)
        assert abs(w.sum() - 1.0) <= 1e-12 and (w > 0).all() and not np.allclose(w, np.roll(w, 1))
        for which in (0, 1):
            r = cc.transition_rates(C, which)
            assert (r > 0).all() and (np.diff(r) > 0).all() and abs(r.mean() - 1.0) <= 1e-12
        assert not np.allclose(cc.transition_rates(C, 0), cc.transition_rates(C, 1))
    for S, C, cx in cc.matrix_cases():
        assert S in (4, 7, 20, 61, 100) and C in (9, 16, 17, 32) and (C > 16 or S == 4) and (not cx or S in (4, 7))
    assert len(cc.matrix_cases()) == 4 * 2 + 2 * 2 + 3 * 2
    for S, T, P, C in cc.GRADIENT_CASES:
        wl = cc.gradient_workload(S, T, P, C)
        assert abs(wl.cat_weights.sum() - 1.0) <= 1e-12 and not np.allclose(wl.cat_weights, cc.rolled(wl).cat_weights)


# ---- the checkers see a perturbed answer ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", [(4, 10, 130, 17), (20, 8, 33, 32), (61, 6, 37, 9)], ids=cc.case_id)
@pytest.mark.parametrize("scheme", [RESCALE_NONE, RESCALE_ALWAYS])
def test_likelihood_checkers_pass_on_the_oracle_and_fail_on_rolled_weights(case, scheme, oracle_lib):
    """On a workload whose category weights differ from one another, so that the rolled copy differs at every step: the first thing to
    go wrong is then the first step's lnL, and the pruning reference's first step's site values."""
    wl = cc.gradient_workload(*case)
    good = cc.run_sequence(wl, scheme, library=oracle_lib, matrices=True)
    again = cc.run_sequence(wl, scheme, library=oracle_lib, matrices=True)
    cc.check_sequences(again, good, "oracle twice")
    cc.check_against_prune(wl, good, "oracle")
    bad = cc.run_sequence(wl, scheme, library=oracle_lib, matrices=True, roll_weights=True)
    assert all(abs(b.lnl - g.lnl) > 1e-8 * abs(g.lnl) for b, g in zip(bad, good))        # every step is perturbed
    with pytest.raises(AssertionError, match="lnL.*first"):
        cc.check_sequences(bad, good, "rolled weights")
    with pytest.raises(AssertionError, match="first"):
        cc.check_against_prune(wl, bad, "rolled weights")


@pytest.mark.parametrize("step", [0, 3, 5])
@pytest.mark.parametrize("quantity", ["lnL", "site values", "partials", "scale factors", "cumulative buffer"])
def test_every_comparison_of_the_likelihood_checker_fires_on_its_own(quantity, step, oracle_lib):
    """The oracle's record with ONE quantity of ONE step moved by 1e-9 (relative; absolute on the logarithms of the scale buffers), ten
    times the bound: the checker fails, and with the assertion that names that quantity and that step."""
    wl = cc.workload(20, 8, 33, 17)
    good = cc.run_sequence(wl, RESCALE_ALWAYS, library=oracle_lib)
    bad = copy.deepcopy(good)
    s = bad[step]
    last = max(s.partials)
    if quantity == "lnL":
        s.lnl *= 1.0 + 1e-9
    elif quantity == "site values":
        s.site[-1] *= 1.0 + 1e-9
    elif quantity == "partials":
        c, p, k = np.unravel_index(np.argmax(s.partials[last]), s.partials[last].shape)
        s.partials[last][c, p, k] *= 1.0 + 1e-9
    elif quantity == "scale factors":
        s.factors[last][-1] += 1e-9
    else:
        s.cumulative[-1] += 1e-9
    cc.check_sequences(copy.deepcopy(good), good, "a copy")
    with pytest.raises(AssertionError, match="%s.*%s" % (quantity, cc.STEPS[step])):
        cc.check_sequences(bad, good, "one quantity moved")


@pytest.mark.parametrize("S,C,cx", cc.matrix_cases(), ids=lambda v: str(v))
def test_matrix_checker_holds_the_oracle_to_the_matrix_exponential(S, C, cx, oracle_lib):
    """The oracle's updateTransitionMatrices and updateTransitionMatricesWithMultipleModels within 1e-12 of scipy's expm for every
    category, at every case of the GPU file: the bound the engine is held to is one the eigen route reaches."""
    models, rates, out = cc.run_matrices(S, C, cx, library=oracle_lib)
    worst = cc.check_matrices(models, rates, out, "oracle S=%d C=%d" % (S, C))
    print("S=%d C=%d complex=%s: oracle against expm %.2e" % (S, C, cx, worst["matrices"]))


@pytest.mark.parametrize("S,C,cx", [(4, 17, False), (7, 32, True), (20, 17, False)])
def test_matrix_checker_fails_on_rolled_rates(S, C, cx, oracle_lib):
    models, rates, out = cc.run_matrices(S, C, cx, library=oracle_lib, roll_rates=True)
    with pytest.raises(AssertionError):
        cc.check_matrices(models, rates, out, "rolled rates")


@pytest.mark.parametrize("S,T,P,C", [(4, 10, 130, 17), (20, 8, 33, 17)])
@pytest.mark.parametrize("rescale", [False, True])
def test_gradient_checker_passes_on_the_oracle_and_fails_on_rolled_weights(S, T, P, C, rescale, oracle_lib):
    wl = cc.gradient_workload(S, T, P, C)
    records = []
    for w in (wl, wl, cc.rolled(wl)):
        g = BranchGradient(w, rescale=rescale, library=oracle_lib)
        records.append(cc.record_gradient(g))
        g.close()
    cc.check_gradients(wl, records[1], records[0], "oracle twice")
    with pytest.raises(AssertionError):
        cc.check_gradients(wl, records[2], records[0], "rolled weights")


@pytest.mark.parametrize("C", cc.COUNTS)
@pytest.mark.parametrize("S,T", cc.HISTORY_SHAPES)
def test_no_history_of_the_gpu_cases_is_near_its_end_or_cut(S, T, C):
    """What the exact comparison of the complete histories rests on (tests/test_complete_history_host.py holds the same for its own cases):
    no event time within 1e-12 relative of its branch's end, none cut; and the draw reaches most of the categories."""
    c, res = cc.history_case(S, T, C)
    assert res["near"].sum() == 0 and not res["cut"].any() and not res["bad"]
    assert res["counts"].sum() == len(res["event_site"]) > 0
    assert abs(c.cat_weights.sum() - 1.0) <= 1e-12 and (c.cat_rates > 0).all() and len(c.cat_rates) == C
    assert len(np.unique(res["categories"])) > C // 2


@pytest.mark.parametrize("case", cc.NODE_HEIGHT_CASES, ids=cc.case_id)
def test_node_height_checker_passes_on_the_oracle_and_fails_on_rolled_weights(case, oracle_lib):
    import node_height_reference as nr
    from beast_mcmc_amd.nodeheight import NodeHeightGradient
    S, T, P, C = case
    wl = cc.gradient_workload(*case)
    rates = np.random.default_rng(11 + T).uniform(0.5, 2.0, size=2 * T - 1)
    out = []
    for w in (wl, wl, cc.rolled(wl)):
        o = NodeHeightGradient(w, rates=rates, library=oracle_lib)
        lnl = o.prepare()
        out.append((lnl,) + tuple(nr.from_plan(o)))
        o.close()
    cc.check_node_heights(out[1], out[0], T, "oracle twice")
    with pytest.raises(AssertionError):
        cc.check_node_heights(out[2], out[0], T, "rolled weights")
