"""What the CPU and the GPU tests of sequence simulation share: the distribution case (tree, model, seed, site count), its bounds
and the statistic."""
import itertools

import numpy as np
from scipy import stats

from beast_mcmc_amd.inputs import substmodel, trees

# ---- the distribution case: 4 tips, 4 states, 2 categories; unequal frequencies and GTR rates, so that P != P^T
N_SITES = 1 << 20
SEED = 20261019
CAT_WEIGHTS = np.array([0.3, 0.7])
CAT_RATES = np.array([0.5, 1.5])
FREQS = np.array([0.1, 0.2, 0.3, 0.4])
GTR_RATES = np.array([1.0, 2.5, 0.7, 1.4, 3.1, 0.9])
MIN_EXPECTED = 20.0
# Pearson's statistic over 256 cells has 255 degrees of freedom; a correct sampler exceeds this once in a million seeds
CHI2_BOUND = float(stats.chi2.ppf(1.0 - 1e-6, 255))
# the count of category 0 is Binomial(N, w0): six standard deviations
CAT_BOUND = 6.0 * float(np.sqrt(N_SITES * CAT_WEIGHTS[0] * CAT_WEIGHTS[1]))


def tree():
    """((0, 1), (2, 3)) with branches long enough that the rarest of the 256 tip patterns is expected MIN_EXPECTED times and more."""
    return trees.from_nested(((0, 1, 0.8), (2, 3, 1.0), 1.5), 4)


def model():
    return substmodel.gtr(GTR_RATES, FREQS)


def all_patterns():
    """[4][256]: every assignment of the four tips, pattern index = t0 * 64 + t1 * 16 + t2 * 4 + t3."""
    return np.array(list(itertools.product(range(4), repeat=4)), dtype=np.int32).T.copy()


def pattern_index(tips):
    t = np.asarray(tips, dtype=np.int64)
    return ((t[0] * 4 + t[1]) * 4 + t[2]) * 4 + t[3]


def tree_likelihood(library=None, tip_states=None, weights=None, **kw):
    """The case's model over all 256 patterns (or the given ones) on `library` (default: the engine)."""
    from beast_mcmc_amd.treelikelihood import BeagleTreeLikelihood
    pats = all_patterns() if tip_states is None else tip_states
    w = np.ones(pats.shape[1]) if weights is None else weights
    return BeagleTreeLikelihood(tree=tree(), tip_states=pats, weights=w, eig=model(), freqs=FREQS, cat_rates=CAT_RATES,
                                cat_weights=CAT_WEIGHTS, state_count=4, library=library, **kw)


def chi_square(tips, probabilities):
    """Pearson's statistic of the simulated tip patterns ([4][N]) against the exact pattern probabilities ([256])."""
    n = tips.shape[1]
    observed = np.bincount(pattern_index(tips), minlength=256).astype(np.float64)
    expected = n * np.asarray(probabilities, dtype=np.float64)
    return float(((observed - expected) ** 2 / expected).sum())


def check_distribution(tips, cats, probabilities):
    """The two bounds of the case; returns the figures (printed by the tests before they assert)."""
    n = tips.shape[1]
    assert n == N_SITES
    assert abs(float(np.sum(probabilities)) - 1.0) <= 1e-12
    assert n * float(np.min(probabilities)) >= MIN_EXPECTED
    stat = chi_square(tips, probabilities)
    cat0 = int(np.sum(np.asarray(cats) == 0))
    print("chi2 = %.2f (bound %.2f), category 0: %d of %d (expected %.0f +- %.0f)"
          % (stat, CHI2_BOUND, cat0, n, n * CAT_WEIGHTS[0], CAT_BOUND))
    assert stat < CHI2_BOUND
    assert abs(cat0 - n * CAT_WEIGHTS[0]) <= CAT_BOUND
    return stat, cat0
