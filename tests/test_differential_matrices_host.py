"""Substitution-parameter differential matrices, CPU tier: the C ABI symbol, the numpy restatement of the reference's
getExactDifferentialMassMatrix (tests/differential_matrices_reference.py) against finite differences of P in the parameter, the
first-order form, and the host route of SubstitutionParameterGradient — driven by the CPU oracle — against finite differences of the
oracle's own log-likelihood."""
import os
import re

import numpy as np
import pytest

import beast_mcmc_amd as bm
import differential_matrices_reference as dr
import helpers
from beast_mcmc_amd import substgradient as sg

SYMBOL = "beagleMi355UpdateDifferentialMatrices"
EPS = np.finfo(float).eps


def test_library_exports_and_header_declares_the_call(engine_lib):
    assert hasattr(engine_lib.lib, SYMBOL)
    hdr = open(os.path.join(helpers.ROOT, "include", "beagle_mi355.h")).read()
    assert re.search(r"\bint\s+%s\s*\(" % SYMBOL, hdr)
    assert re.search(r"#define\s+BEAGLE_MI355_DIFFERENTIAL_EXACT\s+0\b", hdr)
    assert re.search(r"#define\s+BEAGLE_MI355_DIFFERENTIAL_FIRST_ORDER\s+1\b", hdr)
    assert SYMBOL in bm.beagle.ABI_SYMBOLS
    assert hasattr(bm.beagle.Beagle, "updateDifferentialMatrices")
    assert (bm.beagle.Beagle.DIFFERENTIAL_EXACT, bm.beagle.Beagle.DIFFERENTIAL_FIRST_ORDER) == (dr.EXACT, dr.FIRST_ORDER) == (0, 1)


CASES = {
    "hky-kappa": (lambda k: sg.hky_kappa(k, [0.1, 0.3, 0.2, 0.4]), 2.3, 0),
    "jc69-kappa": (lambda k: sg.hky_kappa(k, [0.25, 0.25, 0.25, 0.25]), 1.0, 0),       # a triple eigenvalue
    "gy94-omega": (lambda w: sg.gy94_omega(2.0, w, dr.CODON_PI), 0.4, 0),
    "complex-5": dr.complex_case(5, 0) + (1,),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_matches_finite_differences_of_p(name):
    """dP / d theta = P D: the restatement's D against (P(theta + h) - P(theta - h)) / 2h, h = 1e-6, to 1e-8 absolute.  With an
    analytic dQ the error is the difference's own: h^2 P''' / 6 ~ 1e-12 and rounding eps |P| / h ~ 2e-10 (measured 2e-10 .. 8e-10)."""
    make, theta, pairs = CASES[name]
    m = make(theta)
    S = m.eig.evec.shape[0]
    _, _, real, firsts = dr.split_eigenvalues(m.eig.evals, S)
    assert len(firsts) == pairs and len(real) == S - 2 * pairs
    if name == "jc69-kappa":
        lam = np.sort(m.eig.evals)
        assert lam[2] - lam[0] < 1e-10 and lam[3] - lam[2] > 1.0       # the |lambda_i - lambda_j| < 1e-10 branch is taken off the diagonal
    h = 1e-6
    up, dn = make(theta + h), make(theta - h)
    for t in (0.05, 0.7, 3.0):
        D, raw = dr.exact(m.eig.evec, m.eig.ievc, m.eig.evals, m.dq[0], t)
        dr.assert_guard(raw, m.eig.evals, S)
        P = dr.transition_probabilities(m.eig.evec, m.eig.ievc, m.eig.evals, t)
        fd = (dr.transition_probabilities(up.eig.evec, up.eig.ievc, up.eig.evals, t) -
              dr.transition_probabilities(dn.eig.evec, dn.eig.ievc, dn.eig.evals, t)) / (2 * h)
        err = float(np.max(np.abs(P @ D - fd)))
        print("%s t = %.2f: max |P D - dP/dtheta| = %.3e   smallest kept |V| = %.3e" % (name, t, err, np.min(np.abs(raw)[np.abs(raw) >= 1e-10])))
        assert err <= 1e-8


def test_longdouble_restatement_agrees():
    m = CASES["gy94-omega"][0](0.4)
    d64 = dr.exact(m.eig.evec, m.eig.ievc, m.eig.evals, m.dq[0], 0.7)[0]
    dld = dr.exact(m.eig.evec, m.eig.ievc, m.eig.evals, m.dq[0], 0.7, dtype=np.longdouble)[0]
    assert dld.dtype == np.longdouble
    assert float(np.max(np.abs(d64 - dld)) / np.max(np.abs(dld))) <= 61 * EPS


def test_first_order_is_dist_times_dq():
    m = CASES["hky-kappa"][0](2.3)
    rates = np.array([0.3, 1.7])
    got = dr.slot(m.eig.evec, m.eig.ievc, m.eig.evals, m.dq[0], 0.37, rates, mode=dr.FIRST_ORDER)
    for c, r in enumerate(rates):
        assert np.array_equal(got[c], (0.37 * r) * m.dq[0])


def test_host_route_gradient_matches_finite_differences_of_the_oracle(oracle_lib):
    """Every component against the central difference of the oracle's lnL in that class's kappa, h = 1e-4 kappa, with the bound of
    test_gradient_matches_finite_differences_on_the_engine: 1e-5 max(1, |g|) + 50 eps |lnL| / h."""
    wl, kappas, g = dr.three_class_plan(oracle_lib)
    lnl, grad = g.gradient()
    assert grad.shape == (3, 1)
    for k, kappa in enumerate(kappas):
        h = 1e-4 * kappa
        g.set_model(k, sg.hky_kappa(kappa + h, wl.freqs)); up = g.log_likelihood()
        g.set_model(k, sg.hky_kappa(kappa - h, wl.freqs)); dn = g.log_likelihood()
        g.set_model(k, sg.hky_kappa(kappa, wl.freqs))
        noise = 50 * EPS * abs(lnl) / h
        err = abs((up - dn) / (2 * h) - grad[k, 0])
        print("class %d: d lnL / d kappa = %.8g  error = %.3e  (rounding %.3e)" % (k, grad[k, 0], err, noise))
        assert err <= 1e-5 * max(1.0, abs(grad[k, 0])) + noise
    assert g.log_likelihood() == lnl
    with pytest.raises(ValueError):
        sg.SubstitutionParameterGradient(wl, g.models, g.branch_model, route="device", library=oracle_lib)      # the oracle lacks the symbol
    g.close()
