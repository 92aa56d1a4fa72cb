"""Inputs shared by the robust-counting tests (CPU and GPU tiers): the three position models, the registers, the unconditioned cases."""
import numpy as np

import helpers
import robust_counting_reference as rr
from beast_mcmc_amd.inputs import substmodel

UNCONDITIONED_LENGTHS = [0.0, 0.3, 5.0]
UNCONDITIONED_SITES = (1, 257)
UNCONDITIONED_SEED = 9041


def position_models(seed):
    """Three distinct random GTR models with distinct site rates -> (eigs, frequencies, site rates).  No pair of the product
    chain's 64 eigenvalues may have a gap in (1e-7, 1e-4): there the difference quotient of populateAuxInt amplifies the last bit
    of exp() beyond what the tests' floor allows for."""
    rng = np.random.default_rng(7000 + seed)
    eigs, pis = [], []
    for _ in range(3):
        pi = rng.dirichlet(np.full(4, 10.0))
        eigs.append(substmodel.gtr(rng.gamma(2.0, 1.0, size=6) + 0.1, pi))
        pis.append(pi)
    rates = [0.6, 1.0, 1.7]
    lam = rr.product_chain(eigs, rates)[2]
    gap = np.abs(lam[:, None] - lam[None, :])
    assert not ((gap > 1e-7) & (gap < 1e-4)).any(), gap[(gap > 1e-7) & (gap < 1e-4)]
    return eigs, pis, rates


def near_tie_position_models():
    """HKY kappa = 1 + 1e-6 and kappa = 1 + 8e-8, both with pi = (.1, .2, .3, .4), and one GTR model of position_models(0), at
    position_models' site rates -> (eigs, frequencies, site rates).  The product chain's eigenvalue gaps lie on both sides of
    populateAuxInt's 1e-7 threshold and inside the band position_models keeps out of; tests that use this chain measure against
    an exact yardstick (tests/markov_jumps_exact.py), not against a floor."""
    pi = np.array([0.1, 0.2, 0.3, 0.4])
    eigs, pis, rates = position_models(0)
    eigs = [substmodel.hky(1.0 + 1e-6, pi), substmodel.hky(1.0 + 8e-8, pi), eigs[2]]
    lam = rr.product_chain(eigs, rates)[2]
    gap = np.abs(lam[:, None] - lam[None, :])
    assert ((gap > 1e-7) & (gap < 1e-4)).any() and ((gap > 1e-9) & (gap < 1e-7)).any()
    return eigs, [pi, pi, pis[2]], rates


def three_registers(seed=5):
    """syn, non-syn and a general-valued register with a non-zero diagonal (which must be ignored)."""
    syn, non = rr.codon_registers(helpers.golden("robust_counting.json")["universal_code"]["table"])
    return np.stack([syn, non, np.random.default_rng(seed).uniform(0.0, 2.0, (64, 64))])


def unconditioned_cases():
    """name -> (Q, start frequencies, registers): the product chain of position_models(0) with the three registers, and one HKY."""
    eigs, pis, rates = position_models(0)
    _, _, _, Q, = rr.product_chain(eigs, rates)
    pi = np.kron(np.kron(pis[0], pis[1]), pis[2])
    h = substmodel.hky(2.0, [0.3, 0.2, 0.25, 0.25])
    Q4 = (h.evec * h.evals[None, :]) @ h.ievc
    R4 = np.stack([np.ones((4, 4)), np.random.default_rng(2).uniform(0.0, 1.0, (4, 4))])
    return {"chain64": (Q, pi, three_registers()), "hky4": (Q4, np.array([0.3, 0.2, 0.25, 0.25]), R4)}
