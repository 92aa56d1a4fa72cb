"""Node-height derivatives, CPU tier: the C ABI symbol, the caller's tables, and the numpy restatement of
DiscreteTraitNodeHeightDelegate.getNodeDerivatives (tests/node_height_reference.py) — driven by the CPU oracle — against finite
differences of the oracle's own log-likelihood in a node's height."""
import os
import re

import numpy as np
import pytest

import beast_mcmc_amd as bm
import helpers
import node_height_reference as nr
from beast_mcmc_amd.nodeheight import NodeHeightGradient

SYMBOL = "beagleMi355NodeHeightDerivatives"
EPS = np.finfo(float).eps
STEP = 3e-3             # the height step, as a fraction of the node's room (see the finite-difference test)
ALLOW_SECOND = 2e-5     # truncation allowances, relative to max(1, |derivative|)
ALLOW_FIRST = 5e-4


def test_library_exports_and_header_declares_the_call(engine_lib):
    assert hasattr(engine_lib.lib, SYMBOL)
    hdr = open(os.path.join(helpers.ROOT, "include", "beagle_mi355.h")).read()
    assert re.search(r"\bint\s+%s\s*\(" % SYMBOL, hdr)
    assert SYMBOL in bm.beagle.ABI_SYMBOLS
    assert hasattr(bm.beagle.Beagle, "nodeHeightDerivatives")


def _plan(S, C, T, P, seed, **kw):
    wl = helpers.random_workload(T, P, S, C, seed=seed)
    rates = np.random.default_rng(seed).uniform(0.5, 2.0, size=2 * T - 1)        # non-unit clock rates on every branch
    return wl, NodeHeightGradient(wl, rates=rates, library=helpers.oracle_library(), **kw)


def test_tables_follow_the_buffer_plan():
    wl, g = _plan(4, 2, 7, 20, seed=4, double_buffer=True)
    tr = wl.tree
    for flip in range(2):
        g.log_likelihood()                                   # flips the buffer set
        rows, rates = g.node_rows()
        assert rows.shape == (g.T - 1, 8) and rates.shape == (g.T - 1, 3)
        for r, i in enumerate(range(g.T, g.N)):
            j, k = int(tr.left[i]), int(tr.right[i])
            assert rows[r, 0] == g.pre_offset + i
            assert list(rows[r, [1, 4]]) == [g.post_index(j), g.post_index(k)]
            assert list(rows[r, [2, 5]]) == [g.matrix_index(j), g.matrix_index(k)]
            assert list(rows[r, [3, 6]]) == [g.q_index, g.q_index]
            assert rows[r, 7] == (-1 if i == tr.root else g.q_index)
            assert list(rates[r, :2]) == [g.rates[j], g.rates[k]] and rates[r, 2] == (0.0 if i == tr.root else g.rates[i])
    # branch length = rate x height difference
    n = g.edges[0]
    assert g.branch_lengths[n] == g.rates[n] * (g.heights[tr.parent[n]] - g.heights[n])
    g.close()


def test_first_is_the_chain_rule_over_the_branch_gradient():
    """DiscreteTraitNodeHeightDelegate.java:69-85: first[i] = sum over children of rate x d lnL / d t - the same for i's own branch,
    with d lnL / d t from calculateEdgeDifferentials."""
    wl, g = _plan(4, 3, 11, 150, seed=8)
    g.prepare()
    first, _ = nr.from_plan(g, second=False)
    _, grad = g.gradient()
    expect = g.first_from_branch_gradient(grad)
    assert np.max(np.abs(first - expect)) <= 1e-10 * max(1.0, float(np.max(np.abs(expect))))
    g.close()


@pytest.mark.parametrize("S,C,T,P,seed", [(4, 3, 9, 70, 1), (7, 2, 6, 50, 3)])
def test_row_restatement_equals_the_tree_restatement_on_one_evaluation(S, C, T, P, seed):
    """``row_derivatives`` reads only what the call's rows name (the form the generated call sequences need, where buffers may belong
    to different evaluations); on the buffers of ONE evaluation it is the restatement that is pinned against finite differences
    below, to rounding: 1e-12 of max(1, largest value)."""
    wl, g = _plan(S, C, T, P, seed)
    g.prepare()
    first, second = nr.from_plan(g)
    rows, rates = g.node_rows()
    compact = set(range(g.T))

    def post_of(buf):
        if buf in compact:
            return nr.expand_states(wl.tip_states[buf], S, C)
        return g.b.getPartials(buf, -1).reshape(C, P, S)

    f, s = nr.row_derivatives(rows, rates, post_of, lambda buf: g.b.getPartials(buf, -1).reshape(C, P, S),
                              lambda m: g.b.getTransitionMatrix(m).reshape(C, S, S), wl.cat_weights, wl.weights)
    for got, want in ((f, first), (s, second)):
        assert np.max(np.abs(got - want)) <= 1e-12 * max(1.0, float(np.max(np.abs(want))))
    only, none = nr.row_derivatives(rows, rates, post_of, lambda buf: g.b.getPartials(buf, -1).reshape(C, P, S),
                                    lambda m: g.b.getTransitionMatrix(m).reshape(C, S, S), wl.cat_weights, wl.weights, second=False)
    assert none is None and np.array_equal(only, f)
    g.close()


@pytest.mark.parametrize("S,C,T,P,seed", [(4, 4, 9, 300, 1), (4, 2, 12, 200, 2), (7, 2, 6, 50, 3)])
def test_restatement_matches_finite_differences_of_the_oracle(S, C, T, P, seed):
    """Central differences of the oracle's lnL in the height h of node i — moving h by d changes the two child branches by
    +r_j d, +r_k d and the node's own branch by -r_i d — against the restatement:
        |(L(h+d) - 2 L(h) + L(h-d)) / d^2 - second| <= ALLOW_SECOND max(1, |second|) + 4 * 50 eps |lnL| / d^2
        |(L(h+d) - L(h-d)) / (2 d)      - first|  <= ALLOW_FIRST  max(1, |first|)  +     50 eps |lnL| / d
    The rounding terms are those of test_gradient_matches_finite_differences_on_the_engine (50 eps |lnL| per evaluated lnL, four
    evaluations' worth in the second difference).  The truncation error of both differences is O(d^2 f''''), and f'''' grows as the
    branches around the node shorten, so d is STEP = 3e-3 of the node's room (the distance to its higher child, and to its parent
    below the root).  Calibration on these three workloads (clock rates uniform on [0.5, 2]): with d = 1e-2 of the room the second
    difference is off by 5.0e-5 .. 5.8e-5 of |second|, with 3e-3 by 4.3e-6 .. 5.3e-6 (the d^2 law), with 1e-3 rounding takes over;
    the first difference is off by 2.3e-5 .. 1.4e-4 of |first| at 3e-3.  The allowances are four times the observed errors at 3e-3.
    Nodes with little room have a tiny d and a rounding term larger than the allowance: they are checked too, but at least three
    nodes per workload — one of them below the root — must be checked with the rounding term under half the allowance."""
    wl, g = _plan(S, C, T, P, seed)
    lnl = g.prepare()
    first, second = nr.from_plan(g)
    tr = wl.tree
    sharp = []
    for r, i in enumerate(g.internal):
        h0 = g.heights[i]
        room = h0 - max(g.heights[tr.left[i]], g.heights[tr.right[i]])
        if i != tr.root:
            room = min(room, g.heights[tr.parent[i]] - h0)
        d = STEP * room
        g.set_height(i, h0 + d); up = g.log_likelihood()
        g.set_height(i, h0 - d); dn = g.log_likelihood()
        g.set_height(i, h0)
        noise2, noise1 = 4 * 50 * EPS * abs(lnl) / d ** 2, 50 * EPS * abs(lnl) / d
        err2 = abs((up - 2 * lnl + dn) / d ** 2 - second[r])
        err1 = abs((up - dn) / (2 * d) - first[r])
        print("node %d: d = %.3e  second = %.6g  error = %.3e  (rounding %.3e)   first = %.6g  error = %.3e  (rounding %.3e)"
              % (i, d, second[r], err2, noise2, first[r], err1, noise1))
        assert err2 <= ALLOW_SECOND * max(1.0, abs(second[r])) + noise2, i
        assert err1 <= ALLOW_FIRST * max(1.0, abs(first[r])) + noise1, i
        if noise2 <= 0.5 * ALLOW_SECOND * max(1.0, abs(second[r])):
            sharp.append(int(i))
    assert len(sharp) >= 3 and any(i != tr.root for i in sharp), sharp
    assert g.log_likelihood() == lnl
    g.close()
