"""Markov jumps, CPU tier: the C ABI symbol, the host restatement of MarkovJumpsCore against the R package's numbers and against
Van Loan's block exponential, the exact two-tip expectation of MarkovJumpsTest, and the host driver's branch times."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest
import scipy.linalg

import beast_mcmc_amd as bm
import helpers
import markov_jumps_reference as mr
from beast_mcmc_amd.inputs import substmodel
from beast_mcmc_amd.markovjumps import MarkovJumpsSampler
from beast_mcmc_amd.treelikelihood import BeagleTreeLikelihood

SYMBOL = "beagleMi355SampleMarkovJumps"
GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "markov_jumps.json")))
R_ORDER = [0, 2, 1, 3]                      # A,C,G,T -> the R package's A,G,C,T (makeComparableToRPackage)


def test_library_exports_and_header_declares_the_call(engine_lib):
    assert hasattr(engine_lib.lib, SYMBOL)
    hdr = open(os.path.join(helpers.ROOT, "include", "beagle_mi355.h")).read()
    assert re.search(r"\bint\s+%s\s*\(" % SYMBOL, hdr)
    assert re.search(r"#define\s+BEAGLE_MI355_JUMPS_REWARDS\s+1\b", hdr)
    assert re.search(r"#define\s+BEAGLE_MI355_JUMPS_SCALE_BY_TIME\s+2\b", hdr)
    assert SYMBOL in bm.beagle.ABI_SYMBOLS
    assert hasattr(bm.beagle.Beagle, "sampleMarkovJumps")


def _eig(model):
    return model.evec, model.ievc, model.evals


def test_restatement_gives_the_r_package_values():
    g = GOLDEN["hky_r"]
    U, Ui, lam = _eig(substmodel.hky(g["kappa"], g["frequencies_acgt"]))
    R = np.zeros((4, 4))
    R[tuple(g["register_from_to_acgt"])] = 1.0
    t = g["time"]
    P = (U * np.exp(lam * t)) @ Ui
    rate_reg = mr.rate_registration(U, Ui, lam, R, "counts")
    J = mr.joint_precompute(U, Ui, lam, mr.precompute(U, Ui, rate_reg), t)
    assert np.allclose(J, mr.joint(U, Ui, lam, rate_reg, t), rtol=0, atol=1e-15)
    tol = g["tolerance"]
    np.testing.assert_allclose(J[np.ix_(R_ORDER, R_ORDER)].ravel(), g["rMarkovJumpsJ"], rtol=0, atol=tol)
    np.testing.assert_allclose((J / P)[np.ix_(R_ORDER, R_ORDER)].ravel(), g["rMarkovJumpsC"], rtol=0, atol=tol)
    rew = mr.rate_registration(U, Ui, lam, np.diag(g["rewards"]), "rewards")
    Jr = mr.joint_precompute(U, Ui, lam, mr.precompute(U, Ui, rew), t)
    np.testing.assert_allclose(Jr[np.ix_(R_ORDER, R_ORDER)].ravel(), g["rMarkovRewardsJ"], rtol=0, atol=tol)
    np.testing.assert_allclose((Jr / P)[np.ix_(R_ORDER, R_ORDER)].ravel(), g["rMarkovRewardsC"], rtol=0, atol=tol)
    assert mr.marginal_rate(rate_reg, g["frequencies_acgt"]) == pytest.approx(g["rMarkovMarginalRate"], abs=tol)
    every = np.ones((4, 4))
    assert mr.marginal_rate(mr.rate_registration(U, Ui, lam, every, "counts"), g["frequencies_acgt"]) == pytest.approx(1.0, abs=1e-12)


def _models():
    rng = np.random.default_rng(12)
    return [("gtr", substmodel.gtr([1.3, 4.1, 0.7, 1.1, 3.9, 1.0], [0.35, 0.15, 0.2, 0.3])),
            ("jc69", substmodel.jc69()),
            ("hky", substmodel.hky(2.0, [0.3, 0.2, 0.25, 0.25])),
            ("random20", substmodel.random_reversible(20, rng)[0])]


@pytest.mark.parametrize("name,model", _models(), ids=lambda x: x if isinstance(x, str) else "")
@pytest.mark.parametrize("t", [1e-4, 0.01, 0.3, 1.0, 5.0])
def test_joint_matrix_is_van_loans_block(name, model, t):
    """J = the top-right block of expm(t [[Q, rateReg], [0, Q]]) for an all-counts, a one-pair count and a reward register."""
    U, Ui, lam = _eig(model)
    S = U.shape[0]
    Q = (U * lam) @ Ui
    rng = np.random.default_rng(S)
    one = np.zeros((S, S)); one[0, S - 1] = 1.0
    for R, kind in [(np.ones((S, S)), "counts"), (one, "counts"), (np.diag(rng.uniform(0.0, 2.0, S)), "rewards")]:
        rate_reg = mr.rate_registration(U, Ui, lam, R, kind)
        J = mr.joint_precompute(U, Ui, lam, mr.precompute(U, Ui, rate_reg), t)
        big = np.zeros((2 * S, 2 * S))
        big[:S, :S] = Q; big[S:, S:] = Q; big[:S, S:] = rate_reg
        vl = scipy.linalg.expm(t * big)[:S, S:]
        np.testing.assert_allclose(J, vl, rtol=0, atol=1e-10 * max(1.0, np.abs(vl).max()))


def _two_tip_expectations():
    """MarkovJumpsTest's two-tip tree by exact enumeration of the root state: E[sum over both branches of V(root, A)]."""
    g = GOLDEN["two_tips"]
    U, Ui, lam = _eig(substmodel.hky(g["kappa"], g["frequencies_acgt"]))
    pi = np.asarray(g["frequencies_acgt"])
    mu, a = g["mu"], g["tip_state_acgt"]
    times = np.array([0.0, 1.0, 1.0])
    P = (U * np.exp(lam * mu)) @ Ui
    post = pi * P[:, a] * P[:, a]
    post = post / post.sum()
    regs = [np.asarray(r).reshape(4, 4) if len(r) == 16 else np.diag(r) for r in g["registers"]]
    cond = mr.tables(U, Ui, lam, regs, g["kinds"], g["scale_by_time"], times, None, [mu], np.stack([P[None]] * 3))
    return np.array([2.0 * np.sum(post * cond[k, 1, 0, :, a]) for k in range(3)]), cond, post


def test_two_tip_tree_gives_the_values_from_r():
    expect, _, _ = _two_tip_expectations()
    np.testing.assert_allclose(expect, GOLDEN["two_tips"]["valuesFromR"], rtol=0, atol=GOLDEN["two_tips"]["tolerance"])


def test_zero_rate_category_rule():
    U, Ui, lam = _eig(substmodel.hky(3.0, [0.25, 0.25, 0.25, 0.25]))
    P = np.stack([np.stack([(U * np.exp(lam * 0.4 * r)) @ Ui for r in (0.0, 2.0)])] * 2)
    regs = [np.ones((4, 4)), np.diag([1.0, 2.0, 0.0, 1.0]), np.diag([1.0, 2.0, 0.0, 1.0])]
    cond = mr.tables(U, Ui, lam, regs, ["counts", "rewards", "rewards"], [False, False, True], [0.0, 0.4], [1.0, 1.0], [0.0, 2.0], P)
    assert np.all(cond[:, 0] == 0.0)
    assert np.all(cond[0, 1, 0] == 0.0) and np.all(cond[1, 1, 0] == 0.0)
    assert np.array_equal(cond[2, 1, 0], 0.4 * np.eye(4))
    assert np.all(np.isfinite(cond[:, 1, 1]))


def test_site_values_and_totals():
    rng = np.random.default_rng(3)
    K, n, C, S, P = 2, 5, 2, 4, 50
    cond = rng.uniform(size=(K, n, C, S, S))
    states = rng.integers(0, S, size=(n, P)).astype(np.uint8)
    parents = np.array([-1, 0, 0, 1, 1])
    cats = rng.integers(0, C, size=P)
    vals, tot, rows = mr.site_values(cond, states, parents, cats)
    assert np.all(vals[:, 0] == 0.0)
    assert vals[1, 3, 7] == cond[1, 3, cats[7], states[1, 7], states[3, 7]]
    np.testing.assert_allclose(tot, vals.sum(axis=1), rtol=1e-15)
    np.testing.assert_allclose(rows, vals.sum(axis=2), rtol=1e-15)


def test_branch_time_product_is_the_edge_length():
    """btlNodeBranchTime's two operands multiply to the edge length the host driver passed to updateTransitionMatrices."""
    wl = helpers.random_workload(12, 40, 4, 2, seed=5)
    tl = BeagleTreeLikelihood(wl, library=helpers.oracle_library())
    rng = np.random.default_rng(1)
    branch_rates = rng.uniform(0.5, 2.0, wl.tree.node_count)
    tl.set_branch_rates(branch_rates)
    tl.getLogLikelihood()
    height = np.array(wl.tree.height, dtype=np.float64)
    node = next(n for n in range(wl.tree.tip_count, wl.tree.node_count) if wl.tree.parent[n] >= 0)
    lo = max(height[wl.tree.left[node]], height[wl.tree.right[node]])
    height[node] = lo + 0.37 * (height[wl.tree.parent[node]] - lo)
    tl.set_node_height(node, float(height[node]))          # (the Python tree's heights stay as they were)
    tl.getLogLikelihood()
    lengths = {}
    raw = helpers.raw_binding(tl)
    sampler = MarkovJumpsSampler(tl)
    for n in range(wl.tree.node_count):
        if wl.tree.parent[n] < 0:
            with pytest.raises(bm.beagle.BeagleException):
                tl.node_branch_time(n)
            continue
        t, r = tl.node_branch_time(n)
        lengths[n] = t * r
        # runTraversal's edge length: branchRate[node] * (height[parent] - height[node]), bit for bit
        assert lengths[n] == branch_rates[n] * (height[wl.tree.parent[n]] - height[n])
        m = raw.getTransitionMatrix(tl.node_matrix_index(n)).reshape(len(wl.cat_rates), 4, 4)
        # the oracle builds row n's matrix from exactly this edge length: the same function of it gives the same bits
        eig = wl.eig
        for c, rate in enumerate(wl.cat_rates):
            expect = np.maximum(0.0, (eig.evec * np.exp(lengths[n] * rate * eig.evals)) @ eig.ievc)
            np.testing.assert_allclose(m[c], expect, rtol=1e-12, atol=1e-15)
    assert np.isclose(sampler.expected_tree_length(), sum(lengths.values()), rtol=1e-15)
    tl.close()
