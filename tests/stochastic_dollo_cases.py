"""Trees, alignments and models of the stochastic Dollo tests (tests/test_stochastic_dollo_host.py, tests/test_gpu_stochastic_dollo.py).

State numbering is MutationDeathType's: the live states first, the death state last.  The binary data type of
examples/TestXML/testBinaryDollo.xml is S = 2: code "1" (extant) = state 0, code "0" (death) = state 1.
"""
import itertools
import json
import os

import numpy as np

from beast_mcmc_amd.inputs import trees

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# The smallest ladder (caterpillar tree, unit steps between nodes, rescaling ALWAYS, the model of underflow_ladder below) for which
# the reference's linear-space cumLike is 0 in float64 — log gives -inf — on some pattern while the long-double form is finite;
# found by tests/test_stochastic_dollo_host.py::test_underflow_ladder, which asserts that this is the smallest.
UNDERFLOW_LADDER_TIPS = 39       # (its all-extant pattern has probability about exp(-779): the tree's total branch length)


def parse_newick(text, taxa):
    """A rooted binary ultrametric newick string -> trees.Tree; tip i is taxa[i], internal nodes in post-order."""
    text = text.strip().rstrip(";")
    pos = [0]

    def length():
        if pos[0] < len(text) and text[pos[0]] == ":":
            pos[0] += 1
            start = pos[0]
            while pos[0] < len(text) and text[pos[0]] not in ",()":
                pos[0] += 1
            return float(text[start:pos[0]])
        return 0.0

    def node():
        if text[pos[0]] == "(":
            pos[0] += 1
            a, ha = node()
            assert text[pos[0]] == ","
            pos[0] += 1
            b, hb = node()
            assert text[pos[0]] == ")"
            pos[0] += 1
            assert abs(ha - hb) < 1e-9, "ultrametric trees only"
            return (a, b, ha), ha + length()
        start = pos[0]
        while text[pos[0]] not in ":,()":
            pos[0] += 1
        tip = taxa.index(text[start:pos[0]])
        return tip, length()

    nested, _ = node()
    return trees.from_nested(nested, len(taxa))


def binary_dollo_fixture():
    """tests/golden/binary_dollo.json: the taxa (in alignment order), the tree string and a few columns of testBinaryDollo.xml."""
    g = json.load(open(os.path.join(GOLDEN, "binary_dollo.json")))
    tree = parse_newick(g["tree"], g["taxa"])
    columns = g["columns"]
    states = np.array([[0 if col[t] == "1" else 1 for col in columns] for t in range(len(g["taxa"]))], dtype=np.int32)
    return g, tree, states


def eight_tip_tree():
    """A fixed unbalanced 8-tip tree with unequal branch lengths."""
    nested = ((((0, 1, 0.3), 2, 0.7), ((3, 4, 0.2), (5, 6, 0.5), 0.9), 1.4), 7, 2.0)
    return trees.from_nested(nested, 8)


def all_extant_patterns(tip_count):
    """[T][2^T - 1]: every binary pattern with at least one extant tip (state 0 = extant, 1 = death)."""
    cols = [c for c in itertools.product((0, 1), repeat=tip_count) if 0 in c]
    return np.array(cols, dtype=np.int32).T.copy()


def ladder(tip_count, step=1.0):
    """Caterpillar tree whose internal nodes are ``step`` apart."""
    return trees.caterpillar_tree(tip_count, root_height=step * (tip_count - 1))


def random_tree(tip_count, seed, root_height=1.5):
    return trees.coalescent_tree(tip_count, np.random.default_rng(seed), root_height=root_height)


def random_alignment(tip_count, pattern_count, S, seed, death_fraction=0.5, unknown_fraction=0.05):
    """[T][P] codes: the death state (S - 1) with probability death_fraction, a few unknown codes (S), else a live state."""
    rng = np.random.default_rng(seed)
    states = rng.integers(0, S - 1, size=(tip_count, pattern_count)).astype(np.int32)
    states[rng.random((tip_count, pattern_count)) < death_fraction] = S - 1
    states[rng.random((tip_count, pattern_count)) < unknown_fraction] = S
    return states


def random_model(S, seed):
    """-> (freqs [S] with a zero death frequency, base generator [S-1][S-1] normalised to one change per unit time, or None for S = 2)."""
    rng = np.random.default_rng(seed)
    live = S - 1
    pi = rng.dirichlet(np.full(live, 5.0))
    freqs = np.concatenate([pi, [0.0]])
    if live == 1:
        return freqs, None
    ex = rng.gamma(2.0, 1.0, size=(live, live))
    ex = (ex + ex.T) / 2.0
    Q = ex * pi[None, :]
    np.fill_diagonal(Q, 0.0)
    np.fill_diagonal(Q, -Q.sum(axis=1))
    Q /= -(pi * np.diag(Q)).sum()
    return freqs, Q


def site_rates(C):
    """-> (category rates, weights): one category, or C unequal ones with mean rate 1."""
    if C == 1:
        return np.ones(1), np.ones(1)
    w = np.linspace(1.0, 2.0, C)
    w /= w.sum()
    r = np.linspace(0.3, 2.0, C)
    r /= (w * r).sum()
    return r, w


def tips_as_partials(states, S, tips, seed):
    """{tip: [P][S]}: the listed tips' codes as partials — one-hot, all ones for an unknown code, and on a few patterns an
    ambiguity between a live state and the death state (which makes the tip not extant there)."""
    rng = np.random.default_rng(seed)
    out = {}
    for t in tips:
        codes = states[t]
        part = np.ones((codes.size, S))
        known = codes < S
        part[known] = 0.0
        part[known, codes[known]] = 1.0
        mixed = rng.random(codes.size) < 0.1
        part[mixed, S - 1] = 1.0
        out[int(t)] = part
    return out
