"""Uniformized Markov jumps without a GPU: the ABI surface of beagleMi355SampleMarkovJumpsUniformized, and the host restatement
(tests/uniformized_reference.py) against the reference's R-package numbers (UniformizedStateHistoryTest), the integrated
expectations (Van Loan's block exponential) and its own event lists."""
import json
import math
import os
import re

import numpy as np
import pytest

import beast_mcmc_amd as bm
import helpers
import uniformized_reference as ur
from beast_mcmc_amd.inputs import substmodel

GOLDEN = json.load(open(os.path.join(helpers.ROOT, "tests", "golden", "uniformized_jumps.json")))
PERM = [0, 2, 1, 3]                                   # R's A,G,C,T <-> A,C,G,T


def hky_q():
    eig = substmodel.hky(GOLDEN["kappa"], GOLDEN["frequencies_acgt"])
    return (eig.evec * eig.evals[None, :]) @ eig.ievc, eig


def test_the_call_is_exported_declared_and_bound():
    name = "beagleMi355SampleMarkovJumpsUniformized"
    lib = bm.beagle.EngineLibrary()
    assert hasattr(lib.lib, name)
    hdr = open(os.path.join(helpers.ROOT, "include", "beagle_mi355.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"\b%s\s*\(" % name, hdr[:hdr.index("typedef struct BeagleApi")])
    assert name in bm.beagle.ABI_SYMBOLS
    assert callable(getattr(bm.beagle.Beagle, "sampleMarkovJumpsUniformized", None))
    from beast_mcmc_amd.markovjumps import MarkovJumpsSampler
    assert "uniformization" in MarkovJumpsSampler.sample.__code__.co_varnames
    assert hasattr(bm.treelikelihood.BeagleTreeLikelihood, "node_height")


def test_chain_powers_and_next_state_pdf_match_the_r_package():
    Q, _ = hky_q()
    mu, R = ur.chain(Q)
    T = ur.powers(R, 5)
    tol = GOLDEN["tolerance"]
    np.testing.assert_allclose(T[1][np.ix_(PERM, PERM)].ravel(), GOLDEN["r_one_step"], atol=tol)
    np.testing.assert_allclose(T[3][np.ix_(PERM, PERM)].ravel(), GOLDEN["r_three_step"], atol=tol)
    g = GOLDEN["next_state"]
    pdf = ur.next_state_pdf(T, g["start"], g["end"], g["n"], g["i"])
    np.testing.assert_allclose((pdf / pdf.sum())[PERM], g["pdf_r"], atol=tol)
    assert mu == max(-np.diag(Q))


def test_poisson_draw_cutoffs():
    Q, eig = hky_q()
    mu, R = ur.chain(Q)
    T = ur.powers(R, 20)
    for case in GOLDEN["poisson_draws"]:
        i, j, t = case["start"], case["end"], case["time"]
        P = ((eig.evec * np.exp(eig.evals * t)) @ eig.ievc)[i, j]
        with np.errstate(divide="ignore"):                  # computePDFDirectly (log 0 = -inf)
            pdf = [float(np.exp(-mu * t + n * (math.log(mu) + math.log(t)) - math.lgamma(n + 1) + np.log(T[n][i, j]) - math.log(P)))
                   for n in range(10)]
        for terms, offset, expect in case["cases"]:
            n, near = ur.draw_n(np.array([sum(pdf[:terms]) + offset]), [i], [j], [t], [P], mu, T, 1000)
            assert n[0] == expect and not near[0]


def conditional_expectation(Q, W, t, i, j):
    """Van Loan: expm([[Q, W], [0, Q]] t) -> (int_0^t e^(Qs) W e^(Q(t-s)) ds)[i, j] / P[i, j]"""
    import scipy.linalg
    S = Q.shape[0]
    B = np.zeros((2 * S, 2 * S))
    B[:S, :S] = Q; B[S:, S:] = Q; B[:S, S:] = W
    E = scipy.linalg.expm(B * t)
    return E[:S, S:][i, j] / E[:S, :S][i, j], E[:S, :S][i, j]


def cyclic_q(S, seed):
    rng = np.random.default_rng(seed)
    q = substmodel.complex_q(rng.uniform(0.02, 0.1, size=S * (S - 1)), S)
    for a in range(S):
        q[a, (a + 1) % S] += 2.0
    np.fill_diagonal(q, 0.0); np.fill_diagonal(q, -q.sum(axis=1))
    assert np.iscomplex(np.linalg.eigvals(q)).any()
    return q


@pytest.mark.parametrize("model,i,j,t", [("hky", 1, 3, 2.0), ("hky", 0, 0, 0.3), ("cycle", 0, 2, 0.8), ("cycle", 1, 1, 1.5)])
def test_restated_means_match_the_integrated_expectations(model, i, j, t):
    Q = hky_q()[0] if model == "hky" else cyclic_q(4, 17)
    S = Q.shape[0]
    regs = [np.ones((S, S)) - np.eye(S), np.zeros((S, S)), np.diag([1.0, 0.0, 0.0, 1.0])]
    regs[1][2, 1] = 1.0
    flags = [0, 0, 1]
    H = 200000
    mu, R = ur.chain(Q)
    N = ur.table_length(mu, [0.0, t], None, [1.0])
    T = ur.powers(R, N)
    exact, P = zip(*[conditional_expectation(Q, Q * r if f == 0 else r, t, i, j) for r, f in zip(regs, flags)])
    z = ur.stream(2024, np.arange(H))
    sim = ur.simulate(z, np.full(H, i), np.full(H, j), np.full(H, t), np.full(H, P[0]), mu, T, N)
    vals = ur.register_values(sim, np.full(H, i), np.full(H, t), regs, flags)
    assert not sim["bad"].any() and not (sim["n"] == N).any()
    mean, se = vals.mean(axis=1), vals.std(axis=1) / np.sqrt(H)
    assert np.all(np.abs(mean - np.array(exact)) <= 5 * se + 1e-12), (mean, exact, se)


def test_jump_fractions_are_uniform_order_statistics():
    H = 100000
    z = ur.stream(5, np.arange(H))
    for n in (2, 5):
        E = np.stack([ur.spacing(z, q) for q in range(1, n + 2)])
        f = np.cumsum(E, axis=0)[:n] / E.sum(axis=0)
        mean, se = f.mean(axis=1), f.std(axis=1) / np.sqrt(H)
        expect = np.arange(1, n + 1) / (n + 1)
        assert np.all(np.abs(mean - expect) <= 5 * se), (mean, expect)


def test_values_recomputed_from_the_event_list():
    """A small tree: counts and rewards recomputed from the restated events equal the restated values exactly."""
    rng = np.random.default_rng(3)
    S, n, P, C = 4, 7, 400, 2
    Q, eig = hky_q()
    parents = np.array([-1, 0, 0, 1, 1, 2, 2])
    times = np.r_[0.0, rng.uniform(0.05, 0.8, n - 1)]
    heights = np.zeros(n)
    for r in range(1, n):
        heights[r] = heights[parents[r]] - times[r]
    cat_rates = [0.5, 1.5]
    mats = np.zeros((n, C, S, S))
    for r in range(1, n):
        for c in range(C):
            mats[r, c] = (eig.evec * np.exp(eig.evals * times[r] * cat_rates[c])) @ eig.ievc
    states = rng.integers(0, S, size=(n, P)).astype(np.uint8)
    cats = rng.integers(0, C, size=P)
    regs = [np.ones((S, S)), np.zeros((S, S)), np.diag([1.0, 0.0, 0.0, 1.0])]
    regs[1][0, 3] = 1.0
    res = ur.restate(parents, times, None, heights, states, cats, cat_rates, mats, Q, regs, [0, 0, 1], 1, 99)
    assert res["event_counts"].sum() == len(res["event_heights"]) > 0
    assert np.array_equal(res["values"][0], res["event_counts"])            # all-jumps = the real changes
    for r in range(1, n):
        for p in range(0, P, 37):
            sel = (res["event_rows"] == r) & (res["event_patterns"] == p)
            tau = times[r] * cat_rates[cats[p]]
            cnt, rew, prev, cur = 0.0, 0.0, 0.0, int(states[parents[r], p])
            for f, (a, b) in zip(res["event_f"][sel], res["event_states"][sel]):
                assert a == cur and a != b
                cnt = cnt + regs[1][a, b]
                rew = rew + regs[2][a, a] * (f * tau - prev)
                prev, cur = f * tau, int(b)
            assert cur == states[r, p]
            rew = rew + regs[2][cur, cur] * (tau - prev)
            assert res["values"][1, r, p] == cnt and res["values"][2, r, p] == rew
            hp = heights[parents[r]]
            np.testing.assert_array_equal(res["event_heights"][sel], hp + res["event_f"][sel] * (heights[r] - hp))
    key = res["event_patterns"] * n + res["event_rows"]
    assert np.all(np.diff(key) >= 0)                                        # (pattern, row, time) order


def test_history_strings_follow_the_reference_layout():
    s = ur.history_strings([1, 1, 2], [0, 0, 3], [0.5, 0.25, 1e-5], np.array([[0, 2], [2, 3], [1, 0]]), [5, 6, 7], 8, 4, "ACGT",
                           compact=True)
    assert s[6][0] == "{{1,0.5,A,G},{1,0.25,G,T}}" and s[7][3] == "{{4,1.0E-5,C,A}}" and s[6][1] == "{}"
