"""CPU tier of the marginal node state posteriors (include/beagle_mi355.h beagleMi355NodePosteriors): the numpy restatement the GPU
tests compare the device with (tests/node_posteriors_reference.py) against the definition — the sum over every assignment of states to
the internal nodes — on trees small enough to enumerate."""
import os
import subprocess

import numpy as np
import pytest

import beast_mcmc_amd as bm
import helpers
import node_posteriors_reference as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("beagleMi355NodePosteriors", "beagleMi355NodePosteriorStats")

EPS = np.finfo(np.float64).eps
# A 6-taxon, 4-state, 4-category posterior takes under 200 roundings from the branch matrices to the quotient (two S-term dot products
# per branch on the way up, two on the way down, ten branches, then C products and sums and S sums), so its first-order bound is
# under 200 eps = 4.4e-14: 1e-12 is more than 20 times that.
ENUMERATION_REL = 1e-12

SHAPES = [(4, 2, 1), (5, 3, 4), (6, 4, 4), (6, 4, 1), (5, 2, 4), (4, 3, 1)]       # (taxa, states, categories)


@pytest.fixture(scope="module")
def cases():
    out = {}
    for T, S, C in SHAPES:
        wl = helpers.random_workload(T, 4, S, C, seed=900 + 10 * T + S + C, unknown_fraction=0.15)
        post, pre_s, post_s = pr.restatement(wl)
        out[(T, S, C)] = (wl, post, pre_s, post_s)
    return out


@pytest.mark.parametrize("shape", SHAPES)
def test_restatement_is_the_enumerated_marginal(cases, shape):
    wl, post, _, _ = cases[shape]
    exact = pr.enumerate_marginals(wl)
    assert post.shape == exact.shape == (wl.tree.node_count, 4, shape[1])
    err = np.max(np.abs(post - exact) / np.maximum(np.abs(exact), np.finfo(float).tiny))
    print(shape, "largest relative difference to the enumeration", float(err))
    # entries that are exactly 0 in the definition (a state a tip excludes) are exactly 0 in the restatement
    assert np.array_equal(exact == 0, post == 0)
    assert err <= ENUMERATION_REL


@pytest.mark.parametrize("shape", SHAPES)
def test_rows_sum_to_one_and_the_longdouble_twin_agrees(cases, shape):
    wl, post, pre_s, post_s = cases[shape]
    S, C = shape[1], shape[2]
    total = np.zeros(post.shape[:2])
    for s in range(S):
        total = total + post[:, :, s]
    assert np.max(np.abs(total - 1.0)) <= (S + 1) * EPS
    twin = pr.posteriors(pre_s, post_s, wl.cat_weights, dtype=np.longdouble)[0]
    # the same partials in, so only the call's own C S + C + S roundings separate the two
    assert np.max(np.abs(post - twin)) <= 2 * (C * S + C + 5) * EPS
    states, probs = pr.map_states(post)
    assert np.array_equal(probs, post.max(axis=2)) and np.array_equal(states, post.argmax(axis=2))


@pytest.mark.parametrize("shape", SHAPES)
def test_category_posteriors_do_not_depend_on_the_node(cases, shape):
    """sum_s pre_c post_c is the category's likelihood of the pattern at every node, so the normalised measure formed at the root
    equals the one formed at any other node within the bound of the rows' sums, (S + 1) eps, absolute on values that are at most 1."""
    wl, _, pre_s, post_s = cases[shape]
    S, C = shape[1], shape[2]
    root = wl.tree.root
    at_root = pr.category_posteriors(pre_s[root], post_s[root], wl.cat_weights)
    assert np.max(np.abs(at_root.sum(axis=1) - 1.0)) <= (S + 1) * EPS
    worst = 0.0
    for n in range(wl.tree.node_count):
        here = pr.category_posteriors(pre_s[n], post_s[n], wl.cat_weights)
        worst = max(worst, float(np.max(np.abs(here - at_root))))
        assert np.max(np.abs(here - at_root)) <= (S + 1) * EPS, n
    print(shape, "largest difference between a node's category posteriors and the root's, in eps:", worst / EPS)
    if shape[2] == 1:
        # AncestralStateBeagleTreeLikelihood.java:434-455 at the root: (sum_k partials[r][j][k]) * proportion[r], normalised by drawChoice —
        # with one category the measure has one entry and normalises to exactly 1
        measure = post_s[root].sum(axis=2) * np.asarray(wl.cat_weights)[:, None]
        assert np.array_equal(at_root, (measure / measure.sum(axis=0)[None, :]).T)
        assert np.all(at_root == 1.0)


def test_totals_in_device_order_are_the_plain_sum(cases):
    wl, post, _, _ = cases[(6, 4, 4)]
    rng = np.random.default_rng(4)
    wide = np.concatenate([post] * 40, axis=1)[:, :131]                      # three blocks of 64, the last ragged
    w = rng.integers(1, 9, size=131).astype(float)
    got = pr.state_totals_in_device_order(wide, w)
    want = pr.state_totals(wide, w)
    assert np.max(np.abs(got - want)) <= 2 * 131 * EPS * w.sum()
    assert np.max(np.abs(got.sum(axis=1) - w.sum())) <= 2 * (131 + 5) * EPS * w.sum()


def test_a_zero_likelihood_pattern_is_nan_alone():
    pre = np.ones((2, 1, 3, 2)); post = np.ones((2, 1, 3, 2))
    post[1, 0, 1] = 0.0
    out, z, bad = pr.posteriors(pre, post, [1.0])
    assert bad.tolist() == [[False, False, False], [False, True, False]]
    assert np.isnan(out[1, 1]).all() and np.isfinite(np.delete(out.reshape(6, 2), 4, axis=0)).all()
    states, probs = pr.map_states(out)
    assert states[1, 1] == 0 and np.isnan(probs[1, 1])


def test_the_entry_points_are_declared_bound_and_documented():
    header = open(os.path.join(ROOT, "include", "beagle_mi355.h")).read()
    for sym in SYMBOLS:
        assert "int %s(" % sym in header
        assert sym in bm.beagle.ABI_SYMBOLS
    for doc in ("DESIGN.md", "README.md", "INTEGRATION.md"):
        assert SYMBOLS[0] in open(os.path.join(ROOT, doc)).read(), doc
    assert hasattr(bm.beagle.Beagle, "nodePosteriors") and hasattr(bm.nodeposteriors, "NodePosteriors")


def test_the_scratch_layout(tmp_path):
    exe = str(tmp_path / "node_posterior_layout_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
                           os.path.join(ROOT, "tests", "native", "node_posterior_layout_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "node_posterior_layout_check: OK" in out.stdout
