"""Shared by the tip-emission tests (CPU and GPU tier): the shapes the feature is checked at, seeded alignments of observed codes with
a tenth of them ambiguous, and the tables.  At 4 states the tables are ``tipmodels.sequence_error_emission``'s; at any other state
count the same arithmetic on S states (ALL_SUBSTITUTIONS: the undamaged probability on the diagonal, the rest spread evenly)."""
import numpy as np

import helpers
from beast_mcmc_amd import tipmodels

# (states, taxa, patterns, categories): pattern counts that are no multiple of 128 (pair blocks) or 32 (T32 tiles), one C = 1 case
SHAPES = [(4, 10, 300, 4), (20, 10, 300, 4), (61, 6, 70, 2), (7, 8, 100, 2), (4, 5, 129, 1)]
_cache = {}


def workload(shape):
    if shape not in _cache:
        S, T, P, C = shape
        wl = helpers.random_workload(T, P, S, C, seed=500 + S + T, unknown_fraction=0.0)
        rng = np.random.default_rng(900 + S)
        codes = np.array(wl.tip_states, dtype=np.int32)
        codes[rng.random(codes.shape) < 0.1] = S                     # a tenth ambiguous
        codes[0, 0], codes[-1, -1] = S, S                            # ... the first and the last pattern among them
        wl.tip_states = np.ascontiguousarray(codes)
        ages = rng.uniform(0.0, 2.0, size=T)                         # a different age per tip
        _cache[shape] = (wl, codes, ages)
    return _cache[shape]


def table(S, base_rate, age, age_rate=0.3):
    e4 = tipmodels.sequence_error_emission(tipmodels.ALL_SUBSTITUTIONS, base_rate, age_rate, age)
    if S == 4:
        return e4
    p = e4[0, 0]
    e = np.full((S, S), (1.0 - p) / (S - 1.0))
    e[np.arange(S), np.arange(S)] = p
    return e


def tables(shape, base_rate):
    S, T = shape[0], shape[1]
    ages = workload(shape)[2]
    return [table(S, base_rate, ages[t]) for t in range(T)]


def transition_matrices(wl, branch_rates=None):
    """{node: [C][S][S]} from the workload's eigen system, in numpy."""
    e, tree = wl.eig, wl.tree
    out = {}
    for n in range(tree.node_count):
        if n == tree.root:
            continue
        t = tree.branch_length(n) * (1.0 if branch_rates is None else branch_rates[n])
        out[n] = np.stack([(e.evec * np.exp(e.evals * r * t)[None, :]) @ e.ievc for r in wl.cat_rates])
    return out
