"""Reversible models decomposed on the device, CPU tier: the three C ABI symbols, the numpy restatement of the kernel's Jacobi iteration
(tests/eigen_reference.py) — its tournament order, sweep counts, residuals, eigenvalues against numpy's symmetric eigensolver and P(t)
against the longdouble scaling-and-squaring yardstick — and the host route of eigensystems.SubstitutionModelSet driven by the CPU
oracle against a hand-written loop of setEigenDecomposition calls."""
import os
import re

import numpy as np
import pytest

import beast_mcmc_amd as bm
import eigen_reference as er
import helpers
from beast_mcmc_amd import eigensystems
from beast_mcmc_amd.inputs import substmodel

SYMBOLS = ("beagleMi355SetReversibleModels", "beagleMi355GetEigenDecomposition", "beagleMi355EigenStats")
EPS = np.finfo(float).eps
MODELS = er.accuracy_models()
IDS = ["S%d-%s" % (S, name) for S, name, _, _ in MODELS]


def test_library_exports_and_header_declares_the_calls(engine_lib):
    hdr = open(os.path.join(helpers.ROOT, "include", "beagle_mi355.h")).read()
    for sym in SYMBOLS:
        assert hasattr(engine_lib.lib, sym)
        assert re.search(r"\bint\s+%s\s*\(" % sym, hdr)
        assert sym in bm.beagle.ABI_SYMBOLS
    for method in ("setReversibleModels", "getEigenDecomposition", "eigenStats"):
        assert hasattr(bm.beagle.Beagle, method)


@pytest.mark.parametrize("n", [2, 4, 6, 8, 10, 16, 20, 62, 64])
def test_tournament_meets_every_pair_once_per_sweep(n):
    seen = set()
    rounds = er.tournament(n)
    assert len(rounds) == n - 1
    for p, q in rounds:
        assert len(p) == n // 2 and np.all(p < q)
        assert sorted(np.concatenate([p, q]).tolist()) == list(range(n))          # disjoint pairs: everybody plays
        seen |= set(zip(p.tolist(), q.tolist()))
    assert len(seen) == n * (n - 1) // 2


@pytest.fixture(scope="module")
def decompositions():
    return [er.decompose(r, pi) for _, _, r, pi in MODELS]


@pytest.mark.parametrize("k", range(len(MODELS)), ids=IDS)
def test_restatement_converges_and_reconstructs(k, decompositions):
    """At most 15 sweeps on every test input (the cap of 30 is a failure flag), and U U^-1 = I, U diag(lambda) U^-1 = Q / n to Jacobi's
    backward error c S eps with c = 8 (test_gpu_differential_matrices.check_case's factor: another association of the same sums)."""
    S, name, r, pi = MODELS[k]
    d = decompositions[k]
    ident, recon = er.residuals(d, r, pi)
    print("%s: %d sweeps, |U U^-1 - I| = %.3e, |U L U^-1 - Q/n| / |Q/n| = %.3e, 8 S eps = %.3e" % (IDS[k], d.sweeps, ident, recon, 8 * S * EPS))
    assert not d.capped and d.sweeps <= 15
    assert np.all(np.diff(d.evals) >= 0)
    assert ident <= 8 * S * EPS
    assert recon <= 8 * S * EPS


@pytest.mark.parametrize("k", range(len(MODELS)), ids=IDS)
def test_eigenvalues_match_numpy_eigh(k, decompositions):
    """Both solvers are backward stable on the symmetric A: each eigenvalue moves by at most its solver's ||E||_2 <= c S eps ||A||_2
    (Weyl), so the two differ by at most twice that; c = 8 as above, ||A||_2 = max |mu|."""
    S, name, r, pi = MODELS[k]
    A, _, n = er.symmetrised(r, pi)
    ref = np.linalg.eigvalsh(A) / n
    err = float(np.max(np.abs(decompositions[k].evals - ref)))
    print("%s: max |lambda - eigh| = %.3e, bound %.3e" % (IDS[k], err, 16 * S * EPS * np.max(np.abs(ref))))
    assert err <= 16 * S * EPS * float(np.max(np.abs(ref)))


@pytest.mark.parametrize("k", range(len(MODELS)), ids=IDS)
def test_p_of_t_matches_the_longdouble_yardstick(k, decompositions):
    """P(t) = Pi^-1/2 (V exp(M t) V^T) Pi^1/2: the symmetric core has norm 1 and carries the products' c S eps; an entry is then scaled by
    sqrt(pi_j / pi_i) <= kappa, and an eigenvalue off by c S eps |lambda|_max moves exp(lambda t) by at most t times that.  So
    max |P_64 - P_ld| <= 8 S eps (kappa + t |lambda|_max)."""
    S, name, r, pi = MODELS[k]
    d = decompositions[k]
    kappa = float(np.sqrt(np.max(pi) / np.min(pi)))
    for t in er.LENGTHS:
        for rate in er.CATEGORY_RATES[[0, 3]]:
            dist = t * rate
            err = float(np.max(np.abs(er.transition_probabilities(d, dist) - er.yardstick_p(r, pi, dist))))
            bound = 8 * S * EPS * (kappa + dist * float(np.max(np.abs(d.evals))))
            print("%s t = %.4g: max |P - P_ld| = %.3e, bound %.3e" % (IDS[k], dist, err, bound))
            assert err <= bound


def test_yardstick_is_the_identity_at_zero_and_stochastic():
    _, _, r, pi = MODELS[IDS.index("S20-random0")]
    assert np.array_equal(er.yardstick_p(r, pi, 0.0), np.eye(20, dtype=np.longdouble))
    P = er.yardstick_p(r, pi, 0.9)
    assert P.dtype == np.longdouble and np.all(P > 0)
    assert float(np.max(np.abs(P.sum(axis=1) - 1))) <= 20 * float(np.finfo(np.longdouble).eps)


def test_longdouble_restatement_is_tighter():
    _, _, r, pi = MODELS[IDS.index("S61-gy94-flat")]
    d = er.decompose(r, pi, dtype=np.longdouble)
    assert d.evec.dtype == np.longdouble and not d.capped and d.sweeps <= 15
    ident, recon = er.residuals(d, r, pi)
    assert max(ident, recon) <= 8 * 61 * float(np.finfo(np.longdouble).eps)


def test_a_capped_model_gets_nan_eigenvalues(monkeypatch):
    monkeypatch.setattr(er, "CAP", 1)
    _, _, r, pi = MODELS[IDS.index("S5-random0")]
    d = er.decompose(r, pi)
    assert d.capped and d.sweeps == 1 and np.all(np.isnan(d.evals))


def _oracle_instance(oracle_lib, S, eigens):
    b = bm.beagle.Beagle(2, 3, 2, S, 16, eigens, 40, 4, 0, library=oracle_lib)
    b.setCategoryRates(er.CATEGORY_RATES)
    return b


@pytest.mark.parametrize("S", [4, 61])
def test_host_route_on_the_oracle_is_the_loop_of_set_eigen_decomposition(S, oracle_lib):
    """Per-branch HKY kappa (4 states) and per-branch GY94 omega (61): the set's host route leaves the oracle's eigen buffers — seen
    through the transition matrices they yield — bit for bit as a loop of decompose_reversible + setEigenDecomposition does, in the
    flipped buffers; a second update flips back."""
    count = 5
    models = eigensystems.SubstitutionModelSet(S, count, route="host", library=oracle_lib)
    assert models.eigen_buffer_count == 2 * count
    if S == 4:
        models.set_hky([1.0, 1.7, 3.2, 0.8, 12.0], [0.1, 0.3, 0.2, 0.4])
    else:
        models.set_gy94(2.0, [0.05, 0.2, 0.4, 1.0, 2.5])
    a, b = _oracle_instance(oracle_lib, S, 2 * count), _oracle_instance(oracle_lib, S, 2 * count)
    lengths = er.LENGTHS[np.arange(count) % len(er.LENGTHS)] + 0.01
    for expected_offset in (1, 0):
        updated = models.update(a)
        assert np.array_equal(updated, np.arange(count))
        idx = models.eigen_indices()
        assert np.array_equal(idx, np.arange(count) + expected_offset * count)
        for k in range(count):
            e = substmodel.decompose_reversible(substmodel.reversible_q(models.rates[k], models.freqs[k]), models.freqs[k])
            b.setEigenDecomposition(int(idx[k]), e.evec, e.ievc, e.evals)
        for x in (a, b):
            x.updateTransitionMatricesWithMultipleModels(idx, np.zeros(count, dtype=np.int32), np.arange(count), None, None, lengths, count)
        for k in range(count):
            assert np.array_equal(a.getTransitionMatrix(k), b.getTransitionMatrix(k))
        assert models.update(a).size == 0                    # nothing changed: nothing is decomposed, nothing flips
        assert np.array_equal(models.eigen_indices(), idx)
        models.dirty[:] = expected_offset == 1               # (once more, into the other buffers)
    models.store()
    models.set_model(2, models.rates[2] * 1.5, models.freqs[2])
    assert np.array_equal(models.update(a), [2]) and models.eigen_indices()[2] == 2 + count
    models.restore()
    assert models.eigen_indices()[2] == 2
    a.finalize(); b.finalize()


def test_device_route_on_the_oracle_raises(oracle_lib):
    for sym in SYMBOLS:
        assert not hasattr(oracle_lib.lib, sym) and not hasattr(oracle_lib.lib, "oracle_" + sym)
    with pytest.raises(ValueError):
        eigensystems.SubstitutionModelSet(4, 3, route="device", library=oracle_lib)
    models = eigensystems.SubstitutionModelSet(4, 3, route="host", library=oracle_lib)
    models.set_hky([1.0, 2.0, 3.0], [0.25, 0.25, 0.25, 0.25])
    b = _oracle_instance(oracle_lib, 4, 6)
    with pytest.raises(ValueError):
        models.update(b, route="device")
    with pytest.raises(AttributeError):
        b.setReversibleModels([0], models.rates[:1], models.freqs[:1])
    b.finalize()
