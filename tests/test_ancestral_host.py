"""Ancestral-state draws, CPU tier: the C ABI symbol, the random numbers, the host restatement of the sampler against the exact
posterior, and the pre-order node list AncestralStateSampler builds from a caller's tree and buffer indices."""
import itertools
import os
import re

import numpy as np
import pytest

import ancestral_reference as ar
import beast_mcmc_amd as bm
import helpers
from beast_mcmc_amd.ancestral import AncestralStateSampler
from beast_mcmc_amd.inputs import substmodel, trees
from beast_mcmc_amd.treelikelihood import BeagleTreeLikelihood

SYMBOL = "beagleMi355SampleAncestralStates"


def test_library_exports_and_header_declares_the_sampler(engine_lib):
    assert hasattr(engine_lib.lib, SYMBOL)
    hdr = open(os.path.join(helpers.ROOT, "include", "beagle_mi355.h")).read()
    assert re.search(r"\bint\s+%s\s*\(" % SYMBOL, hdr)
    assert re.search(r"#define\s+BEAGLE_MI355_ANCESTRAL_MAP\s+1\b", hdr)
    assert SYMBOL in bm.beagle.ABI_SYMBOLS
    assert hasattr(bm.beagle.Beagle, "sampleAncestralStates")


def test_random_numbers_are_splitmix64():
    assert int(ar.splitmix64(0, 0)) == 0xE220A8397B1DCDAF           # the first SplitMix64 output from state 0
    # scalar loop restatement of the same formula, against the vectorised one over rows x patterns
    M = (1 << 64) - 1

    def one(seed, ctr):
        z = (seed + (ctr + 1) * ar.GOLDEN) & M
        z = ((z ^ (z >> 30)) * ar.MIX1) & M
        z = ((z ^ (z >> 27)) * ar.MIX2) & M
        return z ^ (z >> 31)

    seed, P = 0xDEADBEEF12345678, 1000
    u = ar.uniforms(seed, np.arange(7)[:, None], np.arange(P)[None, :], P, 0)
    assert u.shape == (7, P)
    for r, p in [(0, 0), (3, 17), (6, 999)]:
        z = one(seed, (r * P + p) * 2)
        assert u[r, p] == (z >> 11) * 2.0 ** -53
    uc = ar.uniforms(seed, 0, np.arange(P), P, 1)
    assert uc[5] == (one(seed, 5 * 2 + 1) >> 11) * 2.0 ** -53
    assert np.all((u >= 0.0) & (u < 1.0)) and abs(float(u.mean()) - 0.5) < 0.01


def test_draw_choice_rules():
    w = [np.array([1.0, 0.0, 2.0, 0.0]), np.array([3.0, 0.0, 2.0, np.nan]), np.array([0.0, 0.0, 1.0, 1.0])]
    s, bad = ar.draw_choice(w, np.array([0.5, 0.5, 0.0, 0.5]), True)
    assert list(s) == [1, 0, 0, 0] and list(bad) == [False, True, False, True]    # MAP: first index of the strict maximum
    s, bad = ar.draw_choice(w, np.array([0.2, 0.5, 0.0, 0.5]), False)
    assert list(s) == [0, 0, 0, 0]
    s, _ = ar.draw_choice(w, np.array([0.26, 0.5, 0.9999, 0.5]), False)
    assert list(s[[0, 2]]) == [1, 2]


def _pruned_three_tips(C, seed):
    """((0, 1)3, 2)4 with compact tips, its partials per category and matrices — the engine's quantities in numpy."""
    rng = np.random.default_rng(seed)
    pi = np.full(4, 0.25) if C > 1 else rng.dirichlet(np.full(4, 5.0))
    eig = substmodel.gtr(rng.gamma(2.0, 1.0, size=6) + 0.1, pi)
    rates = np.array([0.2, 0.7, 1.3, 1.8])[:C] if C > 1 else np.array([1.0])
    cw = np.array([0.1, 0.2, 0.3, 0.4])[:C] if C > 1 else np.array([1.0])
    lengths = {0: 0.3, 1: 0.5, 2: 0.6, 3: 0.25}
    mats = {n: np.stack([eig.transition_probabilities(lengths[n] * r) for r in rates]) for n in lengths}
    tips = {0: 0, 1: 2, 2: 1}
    leaf = {t: np.eye(4)[s] for t, s in tips.items()}
    p3 = np.stack([(mats[0][c] @ leaf[0]) * (mats[1][c] @ leaf[1]) for c in range(C)])        # [C][S]
    p4 = np.stack([(mats[3][c] @ p3[c]) * (mats[2][c] @ leaf[2]) for c in range(C)])
    return pi, cw, mats, tips, p3, p4


@pytest.mark.parametrize("C", [1, 4])
def test_restated_sampler_matches_the_exact_joint_posterior(C):
    pi, cw, mats, tips, p3, p4 = _pruned_three_tips(C, seed=7 + C)
    P = 20000                                                  # identical patterns: independent draws
    part = {4: np.repeat(p4[:, None, :], P, axis=1), 3: np.repeat(p3[:, None, :], P, axis=1)}
    rows = [[4, 0, -1], [3, 3, 0], [0, 0, 1], [1, 1, 1], [2, 2, 0]]     # buffers = node numbers, matrix n = branch above node n
    states, cats, bad = ar.sample(rows, lambda b: part[b], lambda m: mats[m], lambda b: np.full(P, tips[b]), lambda b: b < 3,
                                  cw, pi, seed=12345)
    assert not bad
    assert np.all(states[2] == tips[0]) and np.all(states[3] == tips[1]) and np.all(states[4] == tips[2])
    # exact joint posterior of (root, node 3) by enumeration: sum over categories of w_c pi(x4) P_c(x4, x3) L_c3(x3) P_c(x4 -> tip 2)
    post = np.zeros((4, 4))
    for c, x4, x3 in itertools.product(range(C), range(4), range(4)):
        post[x4, x3] += cw[c] * pi[x4] * mats[3][c][x4, x3] * p3[c][x3] * mats[2][c][x4, tips[2]]
    post /= post.sum()
    emp = np.zeros((4, 4))
    np.add.at(emp, (states[0].astype(int), states[1].astype(int)), 1.0)
    emp /= P
    tv = 0.5 * float(np.abs(emp - post).sum())
    assert tv <= 0.02, (tv, post, emp)
    if C > 1:
        assert len(np.unique(cats)) == C
    # MAP: one answer for every identical pattern, the argmax of the first conditional at each step
    ms, mc, _ = ar.sample(rows, lambda b: part[b], lambda m: mats[m], lambda b: np.full(P, tips[b]), lambda b: b < 3,
                          cw, pi, seed=1, use_map=True)
    assert all(len(np.unique(ms[r])) == 1 for r in range(len(rows)))
    c0 = int(np.argmax([cw[c] * p4[c].sum() for c in range(C)])) if C > 1 else 0
    assert mc[0] == c0 and ms[0, 0] == int(np.argmax(p4[c0] * pi))


def test_unknown_tip_is_drawn_from_the_matrix_row():
    rng = np.random.default_rng(3)
    S, P = 4, 20000
    M = rng.dirichlet(np.ones(S), size=S)[None]                # [1][S][S]
    root = np.tile(np.array([0.0, 1.0, 0.0, 0.0]), (1, P, 1))   # root state 1 with certainty
    rows = [[9, 0, -1], [0, 0, 0], [1, 0, 0]]
    tips = {0: np.full(P, S), 1: np.where(np.arange(P) % 2 == 0, 3, S + 1)}
    st, _, bad = ar.sample(rows, lambda b: root, lambda m: M, lambda b: tips[b], lambda b: b < 2, [1.0], np.full(S, 0.25), seed=9)
    assert not bad and np.all(st[0] == 1) and np.all(st[2][::2] == 3)
    freq = np.bincount(st[1], minlength=S) / P
    assert 0.5 * np.abs(freq - M[0, 1]).sum() <= 0.02


def _tree_likelihood(tree, P=8, C=2):
    """A caller over the CPU oracle: only its tree and buffer bookkeeping are used here."""
    rng = np.random.default_rng(5)
    pi = np.full(4, 0.25)
    eig = substmodel.hky(2.0, pi)
    tips = rng.integers(0, 4, size=(tree.tip_count, P)).astype(np.int32)
    return BeagleTreeLikelihood(tree=tree, tip_states=tips, weights=np.ones(P), eig=eig, freqs=pi, cat_rates=[0.5, 1.5][:C],
                                cat_weights=[0.5, 0.5][:C], state_count=4, library=helpers.oracle_library())


def _check_node_list(sampler, tl, tree):
    rows, order = sampler.node_list()
    assert sorted(order.tolist()) == list(range(tree.node_count))              # every node once
    assert order[0] == tree.root and rows[0, 2] == -1
    for r in range(1, len(rows)):
        n = int(order[r])
        assert 0 <= rows[r, 2] < r and order[rows[r, 2]] == tree.parent[n]      # parent first
        assert rows[r, 0] == tl.node_buffer_index(n) and rows[r, 1] == tl.node_matrix_index(n)
    assert rows[0, 0] == tl.root_buffer_index()
    return rows


@pytest.mark.parametrize("kind", ["coalescent", "yule", "caterpillar"])
def test_node_list_is_preorder_and_follows_double_buffering(kind):
    rng = np.random.default_rng(11)
    if kind == "coalescent":
        tree = trees.coalescent_tree(23, rng, root_height=0.5)
    elif kind == "yule":
        tree = trees.yule_tree(23, rng, root_height=0.5)
    else:
        tree = trees.caterpillar_tree(23, root_height=0.5)
    tl = _tree_likelihood(tree)
    sampler = AncestralStateSampler(tl)
    tl.getLogLikelihood()
    before = _check_node_list(sampler, tl, tree)
    assert np.all(before[before[:, 0] < tree.tip_count, 0] == np.asarray(sampler.preorder())[before[:, 0] < tree.tip_count])
    # a height move flips the moved node's and its children's buffers (BufferIndexHelper): the list follows
    tl.storeState()
    node = [n for n in range(tree.tip_count, tree.node_count) if n != tree.root][0]
    tl.set_node_height(node, helpers.proposed_height(tree, node, rng))
    tl.getLogLikelihood()
    after = _check_node_list(sampler, tl, tree)
    assert not np.array_equal(before[:, :2], after[:, :2])
    tl.restoreState()
    assert np.array_equal(_check_node_list(sampler, tl, tree), before)
    tl.close()
