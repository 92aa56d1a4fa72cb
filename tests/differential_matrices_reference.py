"""The restatement of the differential mass matrices that the tests of beagleMi355UpdateDifferentialMatrices compare with, and what goes
with it: a branch's whole slot, P(t) from the same eigen system, and the guard on the 1e-10 threshold.

The restatement itself — the reference's DifferentiableSubstitutionModelUtil.getExactDifferentialMassMatrix (real and complex eigen
systems) and getApproximateDifferentialMassMatrix in numpy, in a dtype of the caller's choice — is the one the package's host route
uses (beast_mcmc_amd.substgradient: ``exact`` also returns the un-thresholded V); tests/test_differential_matrices_host.py pins it
against finite differences of P.  np.longdouble tells how far float64 itself is off.
"""
import numpy as np

import helpers
from beast_mcmc_amd import substgradient as sg
from beast_mcmc_amd.substgradient import EXACT, FIRST_ORDER, THRESHOLD, exact, first_order, rotate, split_eigenvalues  # noqa: F401


def slot(evec, ievc, evals, dq, edge_length, rates, mode=EXACT, dtype=np.float64):
    """What one branch's matrix slot receives: [C][S][S], dist = edge_length x rate(c) (formed in float64, as the engine forms it)."""
    out = []
    for r in np.asarray(rates, dtype=np.float64):
        dist = np.float64(edge_length) * r
        out.append(exact(evec, ievc, evals, dq, dist, dtype)[0] if mode == EXACT else first_order(dq, dist, dtype))
    return np.stack(out)


def transition_probabilities(evec, ievc, evals, dist):
    """P(dist) from the same eigen system (real, or real block form): what the engine's transition kernel computes."""
    U, Ui = np.asarray(evec, dtype=np.float64), np.asarray(ievc, dtype=np.float64)
    S = U.shape[0]
    re, im, real, firsts = split_eigenvalues(np.asarray(evals, dtype=np.float64), S)
    E = np.zeros((S, S))
    for i in real:
        E[i, i] = np.exp(re[i] * dist)
    for I in firsts:
        e, c, s = np.exp(re[I] * dist), np.cos(im[I] * dist), np.sin(im[I] * dist)
        E[I, I], E[I, I + 1], E[I + 1, I], E[I + 1, I + 1] = e * c, e * s, -e * s, e * c
    return U @ E @ Ui


def assert_guard(raw_v, evals, S):
    """The threshold guard of every EXACT test: no entry of the un-thresholded V and no eigenvalue gap sits where rounding could push
    it across 1e-10 (the result would be discontinuous there)."""
    a = np.abs(np.asarray(raw_v, dtype=np.float64))
    assert not np.any((a > 1e-13) & (a < 1e-7)), "an entry of V lies next to the 1e-10 threshold"
    re, im, real, firsts = split_eigenvalues(np.asarray(evals, dtype=np.float64), S)
    lam = re[np.asarray(real, dtype=int)] if len(real) else np.zeros(0)
    gaps = np.abs(lam[:, None] - lam[None, :])
    assert not np.any((gaps > 1e-13) & (gaps < 1e-7)), "an eigenvalue gap lies next to the 1e-10 threshold"
    for x, I in enumerate(firsts):
        for J in firsts[x + 1:]:
            for g in (abs(re[I] - re[J]), abs(im[I] - im[J])):
                assert not (1e-13 < g < 1e-7), "a conjugate pair's gap lies next to the 1e-10 threshold"


# ---- the models and the plan both tiers use -------------------------------------------------------------------------------
def complex_case(S, seed, which=3):
    """-> (theta -> ParameterModel, theta): a seeded ComplexSubstitutionModel of S states with theta = rates[which]."""
    rates = np.random.default_rng(seed).gamma(1.0, 1.0, size=S * (S - 1)) + 0.05

    def make(theta):
        r = rates.copy()
        r[which] = theta
        return sg.complex_rate(r, S, [which])
    return make, float(rates[which])


CODON_PI = np.random.default_rng(0).dirichlet(np.full(61, 5.0))      # (flat frequencies leave 4 entries of V at 1.5e-13: inside the guard)


def three_class_plan(library, route="host", T=8, P=64, C=4, seed=31):
    """8 tips x 64 patterns x 4 categories, the branches in three classes that each have their own HKY kappa."""
    wl = helpers.random_workload(T, P, 4, C, seed=seed)
    kappas = [1.7, 3.2, 0.8]
    classes = np.arange(wl.tree.node_count) % 3
    models = [sg.hky_kappa(k, wl.freqs) for k in kappas]
    return wl, kappas, sg.SubstitutionParameterGradient(wl, models, classes, route=route, library=library)
