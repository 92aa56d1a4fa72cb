"""Sequence simulation, CPU tier: the C ABI symbol, the draw rules of the host restatement (tests/simulate_reference.py) on hand-made
vectors, and the restatement alone against the exact pattern distribution — with the seed, tree and site count the GPU test uses, so
that the rule itself is shown to stay within the bounds here."""
import os
import re

import numpy as np
import pytest

import beast_mcmc_amd as bm
import helpers
import simulate_cases as sc
import simulate_reference as sr
from beast_mcmc_amd.simulate import SequenceSimulator

SYMBOL = "beagleMi355SimulateSequences"
U_MAX = 1.0 - 2.0 ** -53                                   # the largest uniform the generator returns


def test_library_exports_and_header_declares_the_simulator(engine_lib):
    assert hasattr(engine_lib.lib, SYMBOL)
    hdr = open(os.path.join(helpers.ROOT, "include", "beagle_mi355.h")).read()
    assert re.search(r"\bint\s+%s\s*\(" % SYMBOL, hdr)
    assert "largest index" in hdr.lower()                  # the fall-through rule is part of the header comment
    assert SYMBOL in bm.beagle.ABI_SYMBOLS
    assert hasattr(bm.beagle.Beagle, "simulateSequences")


def _one(p, u):
    cum, last, bad = sr.cumulative(np.asarray(p, dtype=np.float64)[None, :])
    s, b = sr.draw(cum, last, bad, np.array([u]))
    return int(s[0]), bool(b[0])


def test_draw_rules_on_hand_made_vectors():
    # a row whose sum is 1 - 2^-53 (the additions are exact), u just below 1: nothing is above u -> the largest positive index
    p = [0.5, 0.25, 0.25 - 2.0 ** -53]
    assert 0.5 + 0.25 + (0.25 - 2.0 ** -53) == U_MAX
    assert _one(p, U_MAX) == (2, False)
    assert _one([0.5, 0.5 - 2.0 ** -53, 0.0], U_MAX) == (1, False)          # ... which skips a trailing zero
    assert _one(p, np.nextafter(U_MAX, 0.0)) == (2, False)                  # u < cum_2 as usual
    # u < cum is strict: u equal to a cumulative sum goes to the next index
    t = [0.25, 0.5, 0.0, 0.0]
    assert _one(t, 0.0) == (0, False) and _one(t, np.nextafter(0.25, 0.0)) == (0, False)
    assert _one(t, 0.25) == (1, False) and _one(t, 0.7499) == (1, False)
    assert _one(t, 0.75) == (1, False) and _one(t, U_MAX) == (1, False)     # trailing zeros are never drawn
    assert _one([0.0, 0.0, 1.0, 0.0], 0.0) == (2, False)                    # nor are leading ones
    # totals that are not finite and > 0: flagged, the draw is 0
    for z in ([0.0, 0.0, 0.0, 0.0], [0.5, np.nan, 0.5, 0.0], [0.5, np.inf, 0.0, 0.0], [0.5, -0.75, 0.0, 0.25]):
        assert _one(z, 0.3) == (0, True)


def _scalar(p, u):
    """The rule once more, one site at a time in plain Python."""
    cum, total = 0.0, 0.0
    for x in p:
        total = total + x
    if not (total > 0.0 and total <= np.finfo(float).max):
        return 0
    for i, x in enumerate(p):
        cum = cum + x
        if u < cum:
            return i
    return max(i for i, x in enumerate(p) if x > 0.0)


@pytest.mark.parametrize("weights,freqs", [
    ([0.3, 0.7, 0.0], [0.1, 0.2, 0.3, 0.4, 0.0]),
    ([1.0], [0.25, 0.25, 0.25, 0.25 - 2.0 ** -53]),
    ([0.0, 1.0 - 2.0 ** -53], [0.0, 0.0, 1.0]),
])
def test_categories_and_root_states_follow_the_rules(weights, freqs):
    n, seed = 4000, 77
    states, cats, bad = sr.simulate([[0, 0, -1]], None, weights, freqs, seed, n)
    assert not bad and states.shape == (1, n)
    uc, us = sr.uniforms(seed, 0, np.arange(n), n, 1), sr.uniforms(seed, 0, np.arange(n), n, 0)
    want_c = [_scalar(weights, u) if len(weights) > 1 else 0 for u in uc]
    assert cats.tolist() == want_c
    assert states[0].tolist() == [_scalar(freqs, u) for u in us]
    assert all(weights[c] > 0.0 for c in np.unique(cats)) and all(freqs[s] > 0.0 for s in np.unique(states))
    # given categories and root states are taken as they are
    given_c = (np.arange(n) % len(weights)).astype(np.int32)
    given_s = (np.arange(n) % len(freqs)).astype(np.uint8)
    s2, c2, bad = sr.simulate([[0, 0, -1]], None, weights, freqs, seed, n, root_states=given_s, rate_categories=given_c)
    assert not bad and np.array_equal(s2[0], given_s) and np.array_equal(c2, given_c)


def test_a_zero_row_that_is_reached_is_flagged_and_gives_zero():
    M = np.array([[[0.9, 0.1], [0.0, 0.0]]])                # parent state 1 has nothing to draw from
    rows = [[0, 0, -1], [1, 0, 0]]
    n = 1000
    states, _, bad = sr.simulate(rows, lambda m: M, [1.0], [0.5, 0.5], 3, n)
    assert bad and (states[0] == 1).any()
    assert np.all(states[1][states[0] == 1] == 0)
    # ... and is not flagged where no site reaches it
    _, _, bad = sr.simulate(rows, lambda m: M, [1.0], [1.0, 0.0], 3, n)
    assert not bad
    # zero category weights are flagged only where they are drawn from
    _, cats, bad = sr.simulate(rows[:1], None, [0.0, 0.0], [1.0, 0.0], 3, n)
    assert bad and not cats.any()
    _, _, bad = sr.simulate(rows[:1], None, [0.0, 0.0], [1.0, 0.0], 3, n, rate_categories=np.ones(n, dtype=np.int32))
    assert not bad


@pytest.fixture(scope="module")
def exact_case():
    """The oracle's exact pattern probabilities and branch matrices of the distribution case, and the simulator's row list."""
    tl = sc.tree_likelihood(library=helpers.oracle_library())
    lnl = tl.getLogLikelihood()
    assert np.isfinite(lnl)
    prob = np.exp(tl.getSiteLogLikelihoods())
    sim = SequenceSimulator(tl)
    rows, order = sim.node_list()
    mats = {int(m): sim.beagle.getTransitionMatrix(int(m)).copy() for m in rows[1:, 1]}
    tl.close()
    return prob, rows, order, mats


def _tips(states, rows):
    out = np.zeros((4, states.shape[1]), dtype=np.uint8)
    for r in range(len(rows)):
        if rows[r, 0] >= 0:
            out[rows[r, 0]] = states[r]
    return out


def test_restatement_draws_the_exact_pattern_distribution(exact_case):
    prob, rows, order, mats = exact_case
    assert not np.allclose(mats[int(rows[1, 1])][0], mats[int(rows[1, 1])][0].T, atol=1e-3)      # P != P^T
    states, cats, bad = sr.simulate(rows, lambda m: mats[m], sc.CAT_WEIGHTS, sc.FREQS, sc.SEED, sc.N_SITES)
    assert not bad
    sc.check_distribution(_tips(states, rows), cats, prob)


def test_a_transposed_restatement_exceeds_the_bound(exact_case):
    prob, rows, order, mats = exact_case
    states, _, _ = sr.simulate(rows, lambda m: np.ascontiguousarray(np.swapaxes(mats[m], 1, 2)), sc.CAT_WEIGHTS, sc.FREQS, sc.SEED,
                               sc.N_SITES)
    stat = sc.chi_square(_tips(states, rows), prob)
    print("transposed: chi2 = %.1f (bound %.2f)" % (stat, sc.CHI2_BOUND))
    assert stat > sc.CHI2_BOUND
