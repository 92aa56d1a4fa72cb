"""The stochastic Dollo (ALS) likelihood on the CPU: the host restatement (tests/stochastic_dollo_reference.py) over the CPU oracle's
partials and scale factors, read back through beast-mcmc_amd/stochasticdollo.py's read-back route — first principles, scaling,
underflow and the inclusion masks, before any kernel is involved."""
import os
import re
import subprocess

import numpy as np
import pytest

import beast_mcmc_amd as bm
import helpers
import stochastic_dollo_cases as cases
import stochastic_dollo_reference as ref
from beast_mcmc_amd.stochasticdollo import ALSTreeLikelihood, mutation_death_generator

ROOT = helpers.ROOT
SYMBOLS = ("beagleMi355NodePatternLikelihoods", "beagleMi355NodePatternStats")


def oracle_als(tree, states, freqs, C=1, **model):
    rates, weights = cases.site_rates(C)
    return ALSTreeLikelihood.create(tree, states, np.ones(states.shape[1]), freqs, rates, weights, library=helpers.oracle_library(),
                                    route="readback", **model)


def pieces(als):
    """What the restatement takes, from one pruning pass: partials and own scale factors by node, inclusion, log weights by node."""
    als.prune()
    partials, scales = als.read_back()
    extant = ref.tip_extant(als.tip_states, als.tip_partials, als.S, als.death_state)
    below, incl = ref.inclusion(als.tree, extant)
    logw = [np.log(ref.node_survival_probability(als.tree, n, als.mu, als.average_rate(), als.branch_rates))
            for n in range(als.tree.node_count)]
    return partials, scales, incl, logw


def test_abi_and_documents_name_the_call():
    header = open(os.path.join(ROOT, "include", "beagle_mi355.h")).read()
    for sym in SYMBOLS:
        assert re.search(r"^int %s\(" % sym, header, re.M)
        assert sym in bm.beagle.ABI_SYMBOLS
    for doc in ("DESIGN.md", "README.md", "INTEGRATION.md"):
        assert SYMBOLS[0] in open(os.path.join(ROOT, doc)).read(), doc


def test_the_scratch_layout(tmp_path):
    exe = str(tmp_path / "node_pattern_layout_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
                           os.path.join(ROOT, "tests", "native", "node_pattern_layout_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "node_pattern_layout_check: OK" in out.stdout


def test_generator_is_the_mutation_death_model():
    freqs, base = cases.random_model(4, 3)
    Q = mutation_death_generator(base, freqs, mutation_rate=0.8, death_rate=0.6)
    scale = 2 * 0.8 * freqs[0] * freqs[1] * freqs[2]
    assert np.allclose(Q[:3, :3], scale * base - 0.6 * np.eye(3), rtol=0, atol=1e-15)
    assert np.all(Q[:3, 3] == 0.6) and np.all(Q[3] == 0.0)
    assert np.allclose(Q.sum(axis=1), 0.0, atol=1e-15)
    # MutationDeathModel.getTransitionProbabilities: the base model's matrix times exp(-delta d), 1 - exp(-delta d) into the death column
    d = 0.37
    M = bm.stochasticdollo.host_transition_matrix(Q, d)
    B = bm.stochasticdollo.host_transition_matrix(scale * base, d)
    assert np.allclose(M[:3, :3], B * np.exp(-0.6 * d), rtol=1e-13, atol=1e-16)
    assert np.allclose(M[:3, 3], 1 - np.exp(-0.6 * d), rtol=1e-13) and np.all(M[3] == [0, 0, 0, 1])


def test_pattern_sum_is_the_tree_weight():
    """S = 2 (extant, death), one category, mu = the model's death rate, every trait born extant: summed over all 255 patterns with
    at least one extant tip, cumLike is sum_i (1 - u0_i)(1 - p_i) — the probability that a trait born on the branch above i (weight
    1 - p_i = getNodeSurvivalProbability) is seen at some tip (1 - u0_i), which is what calculateLogTreeWeight adds up."""
    tree = cases.eight_tip_tree()
    states = cases.all_extant_patterns(8)
    assert states.shape == (8, 255)
    als = oracle_als(tree, states, [1.0, 0.0], death_rate=0.7, lam=1.3)
    partials, scales, incl, logw = pieces(als)
    expect = ref.tree_weight_sum(tree, 0.7, 1.0)
    cum = ref.linear_cum(tree, partials, scales, incl, als.freqs, [1.0], logw, np.float64)
    assert abs(cum.sum() - expect) <= 1e-13 * expect
    terms, _ = ref.log_terms(tree, tree.postorder(), partials, scales, incl, als.freqs, [1.0], logw, np.float64)
    assert abs(np.exp(ref.log_cum(terms, np.float64)).sum() - expect) <= 1e-13 * expect
    assert abs(np.exp(als.log_pattern_readback()).sum() - expect) <= 1e-13 * expect
    als.close()


@pytest.mark.parametrize("S,C", [(2, 1), (3, 2), (5, 4)])
def test_scaled_equals_unscaled(S, C):
    tree = cases.random_tree(12, seed=5)
    states = cases.random_alignment(12, 40, S, seed=6)
    freqs, base = cases.random_model(S, 7)
    out = []
    for rescale in (False, True):
        als = oracle_als(tree, states, freqs, C=C, base_generator=base, death_rate=0.9, lam=2.0, mutation_rate=1.1, rescale=rescale)
        partials, scales, incl, logw = pieces(als)
        assert rescale == bool(np.any(scales != 0.0))
        rates, weights = cases.site_rates(C)
        cum = ref.linear_cum(tree, partials, scales, incl, freqs, weights, logw, np.float64)
        terms, _ = ref.log_terms(tree, tree.postorder(), partials, scales, incl, freqs, weights, logw, np.float64)
        out.append((cum, ref.log_cum(terms, np.float64), als.getLogLikelihood()))
        als.close()
    assert np.all(out[0][0] > 0)
    assert np.allclose(out[0][0], out[1][0], rtol=1e-12, atol=0)
    assert np.allclose(out[0][1], out[1][1], rtol=1e-12, atol=0)
    assert np.allclose(np.log(out[0][0]), out[0][1], rtol=1e-12, atol=0)
    assert out[0][2] == pytest.approx(out[1][2], rel=1e-12)


def underflow_ladder(tips):
    """The ladder case: unit steps, binary data, death rate 1, rescaling ALWAYS; the first pattern has every tip extant."""
    tree = cases.ladder(tips)
    states = np.ones((tips, 3), dtype=np.int32)
    states[:, 0] = 0
    states[:2, 1] = 0
    states[-1, 2] = 0
    return oracle_als(tree, states, [1.0, 0.0], death_rate=1.0, lam=1.0, rescale=True)


def linear_forms(als):
    partials, scales, incl, logw = pieces(als)
    with np.errstate(divide="ignore"):
        return tuple(np.log(ref.linear_cum(als.tree, partials, scales, incl, als.freqs, [1.0], logw, dt)) for dt in (np.float64, np.longdouble))


def test_underflow_ladder():
    """The reference's linear-space cumLike underflows on a ladder of cases.UNDERFLOW_LADDER_TIPS tips (and on no smaller one); the
    log-space form stays finite and agrees with the long-double linear form."""
    assert np.finfo(np.longdouble).nmant >= 63, "the yardstick needs the 64-bit-mantissa long double"
    smallest = None
    for tips in range(4, 64):
        als = underflow_ladder(tips)
        log64, logld = linear_forms(als)
        als.close()
        assert np.all(np.isfinite(logld))
        if np.any(np.isneginf(log64)):
            smallest = tips
            break
    assert smallest == cases.UNDERFLOW_LADDER_TIPS
    als = underflow_ladder(smallest)
    partials, scales, incl, logw = pieces(als)
    _, logld = linear_forms(als)
    terms, _ = ref.log_terms(als.tree, als.tree.postorder(), partials, scales, incl, als.freqs, [1.0], logw, np.float64)
    value = ref.log_cum(terms, np.float64)
    assert np.all(np.isfinite(value))
    # (an absolute difference of logarithms is a relative difference of cumLike: the third pattern's value is log 1)
    assert np.allclose(value, logld.astype(np.float64), rtol=1e-12, atol=1e-12)
    assert np.isfinite(als.getLogLikelihood())
    als.close()


def test_inclusion_masks_by_hand():
    """The 5-taxon tree of testBinaryDollo.xml, (Ar,((Dr,An),(Ho,Ca))): tips Dr 0, Ar 1, Ca 2, Ho 3, An 4; (Dr,An) is node 5, (Ho,Ca)
    node 6, their parent 7, the root 8.  A node is included where every extant tip of the column lies below it."""
    g, tree, states = cases.binary_dollo_fixture()
    assert [int(tree.left[5]), int(tree.right[5])] == [0, 4] and [int(tree.left[6]), int(tree.right[6])] == [3, 2]
    assert [int(tree.left[7]), int(tree.right[7])] == [5, 6] and [int(tree.left[8]), int(tree.right[8])] == [1, 7] and tree.root == 8
    by_hand = {
        "10001": [0, 0, 0, 0, 0, 1, 0, 1, 1],       # Dr, An: their cherry and everything above it
        "00100": [0, 0, 1, 0, 0, 0, 1, 1, 1],       # Ca alone: the tip itself and its ancestors
        "01000": [0, 1, 0, 0, 0, 0, 0, 0, 1],       # Ar alone: the tip and the root
        "10100": [0, 0, 0, 0, 0, 0, 0, 1, 1],       # Dr, Ca: one in each cherry
        "11111": [0, 0, 0, 0, 0, 0, 0, 0, 1],
        "01001": [0, 0, 0, 0, 0, 0, 0, 0, 1],       # Ar, An: only the root is above both
        "00110": [0, 0, 0, 0, 0, 0, 1, 1, 1],       # Ca, Ho: their cherry
    }
    assert g["columns"] == list(by_hand)
    extant = ref.tip_extant(states, {}, 2, 1)
    assert np.array_equal(extant, 1 - states)
    below, incl = ref.inclusion(tree, extant)
    assert np.array_equal(incl.astype(int).T, np.array(list(by_hand.values())))
    assert np.array_equal(below[8], extant.sum(axis=0))
    # a column with no extant tip is included everywhere (0 >= 0), and a tip whose code is ambiguous with death is not extant
    _, none = ref.inclusion(tree, np.zeros((5, 1), dtype=np.int64))
    assert none.all()
    part = {0: np.array([[1.0, 1.0]] * 7)}
    assert not ref.tip_extant(states, part, 2, 1)[0].any()
    # the read-back route of the package forms the same masks: excluded terms are -inf
    als = oracle_als(tree, states, [1.0, 0.0], death_rate=1.0, lam=1.0)
    als.getLogLikelihood()
    order = tree.postorder()
    assert np.array_equal(np.isfinite(als.last["terms"]), incl[order])
    als.close()


@pytest.mark.parametrize("observation", ["anyTip", "singleTip"])
@pytest.mark.parametrize("integrate", [False, True])
@pytest.mark.parametrize("lists", [((), ()), ((0, 1), ()), ((), (2,)), ((0, 1, 3), (2,))])
def test_full_likelihood_is_the_restatement(observation, integrate, lists):
    tree = cases.random_tree(9, seed=11)
    states = cases.random_alignment(9, 33, 3, seed=12)
    freqs, base = cases.random_model(3, 13)
    rates, weights = cases.site_rates(2)
    pattern_weights = np.arange(1, 34) % 4 + 1.0
    als = ALSTreeLikelihood.create(tree, states, pattern_weights, freqs, rates, weights, library=helpers.oracle_library(),
                                   route="readback", base_generator=base, death_rate=0.8, lam=1.7, observation=observation,
                                   integrate_gain_rate=integrate, include=lists[0], exclude=lists[1],
                                   branch_rates=np.linspace(0.5, 1.5, tree.node_count))
    lnl = als.getLogLikelihood()
    partials, scales, incl, logw = pieces(als)
    terms, _ = ref.log_terms(tree, tree.postorder(), partials, scales, incl, freqs, weights, logw, np.float64)
    expect = ref.finish(ref.log_cum(terms, np.float64), pattern_weights, tree, 0.8, 1.7, als.average_rate(), observation, integrate,
                        lists[0], lists[1], als.branch_rates)
    assert np.isfinite(lnl) and lnl == pytest.approx(expect, rel=1e-12)
    als.close()
