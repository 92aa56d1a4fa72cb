"""Robust counting on the host: the ABI surface, the veneer's registers and product chain against the reference's known answers
(tests/golden/robust_counting.json), and the restatement (tests/robust_counting_reference.py) the GPU tests compare with."""
import os
import re
import subprocess

import numpy as np
import pytest

import beast_mcmc_amd as bm
import helpers
import robust_counting_cases as cases
import robust_counting_reference as rr
from beast_mcmc_amd import robustcounting
from beast_mcmc_amd.inputs import substmodel

SYMBOLS = ("beagleMi355RobustCounts", "beagleMi355SimulateUnconditionedCounts")
G = helpers.golden("robust_counting.json")


def codon(text):
    return sum("ACGT".index(ch) << sh for ch, sh in zip(text, (4, 2, 0)))


def test_symbols_are_exported_declared_and_listed():
    out = subprocess.run(["nm", "-D", "--defined-only", bm.beagle.ENGINE_LIB], stdout=subprocess.PIPE, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    header = open(os.path.join(helpers.ROOT, "include", "beagle_mi355.h")).read()
    for name in SYMBOLS:
        assert name in exported, name
        assert re.search(r"^int %s\(" % name, header, re.M), name
        assert name in bm.beagle.ABI_SYMBOLS, name


def test_registers_match_the_reference():
    syn, non = robustcounting.codon_registers()
    assert robustcounting.UNIVERSAL_CODE == G["universal_code"]["table"]
    assert int(syn.sum()) == G["register_sums"]["syn"] and int(non.sum()) == G["register_sums"]["nonsyn"]
    stops = [codon(c) for c in ("TAA", "TAG", "TGA")]
    for R in (syn, non):
        assert np.array_equal(R, R.T) and not np.diag(R).any() and set(np.unique(R)) == {0.0, 1.0}
        assert not R[stops].any() and not R[:, stops].any()
    assert not (syn * non).any()
    a, b = rr.codon_registers(G["universal_code"]["table"])
    assert np.array_equal(a, syn) and np.array_equal(b, non)


def known_answer_chain():
    g = G["conditional_means"]
    eigs = [substmodel.hky(k, f) for k, f in zip(g["kappa"], g["frequencies_acgt"])]
    return g, eigs


def test_restated_tables_reproduce_the_known_answers():
    g, eigs = known_answer_chain()
    U, Ui, lam, Q = rr.product_chain(eigs, [1.0, 1.0, 1.0])
    syn, non = robustcounting.codon_registers()
    cond, _, _ = rr.tables(U, Ui, lam, Q, [syn, non], [0.0, g["time"]])
    got = [cond[("syn", "nonsyn").index(lab), 1, codon(g["from"]), codon(to)] for lab, to in zip(g["labeling"], g["to"])]
    np.testing.assert_allclose(got, g["values"], rtol=0, atol=g["tolerance"])
    V, Vi, mu, Qv = robustcounting.product_chain(eigs, [1.0, 1.0, 1.0])
    np.testing.assert_allclose(V, U, atol=1e-15)
    np.testing.assert_allclose(Vi, Ui, atol=1e-15)
    np.testing.assert_allclose(mu, lam, atol=1e-15)
    np.testing.assert_allclose(Qv, Q, atol=1e-14)


@pytest.mark.parametrize("seed", range(8))
def test_kronecker_eigen_system_reconstructs_q(seed):
    eigs, pis, rates = cases.position_models(seed)
    for build in (rr.product_chain, robustcounting.product_chain):
        U, Ui, lam, Q = build(eigs, rates)
        np.testing.assert_allclose((U * lam[None, :]) @ Ui, Q, rtol=0, atol=1e-12)
        np.testing.assert_allclose(U @ Ui, np.eye(64), rtol=0, atol=1e-12)
        np.testing.assert_allclose(Q.sum(axis=1), 0.0, atol=1e-12)
    pi = np.kron(np.kron(pis[0], pis[1]), pis[2])
    np.testing.assert_allclose(pi @ Q, 0.0, atol=1e-12)


def test_unconditioned_mean_is_marginal_rate_times_length():
    Q, pi, regs = cases.unconditioned_cases()["chain64"]
    regs = regs[:2]
    length, N = 0.8, 20000
    vals, _, cut = rr.unconditioned(Q, pi, [length], N, regs, 31)
    assert not cut.any()
    for k in range(2):
        exact = float(np.sum(pi[:, None] * (Q * regs[k]))) * length
        x = vals[k, 0]
        assert abs(x.mean() - exact) <= 5.0 * x.std(ddof=1) / np.sqrt(N), (k, x.mean(), exact)


def test_unconditioned_zero_length_and_totals_order():
    Q, pi, regs = cases.unconditioned_cases()["hky4"]
    vals, near, cut = rr.unconditioned(Q, pi, [0.0, 2.0], 300, regs, 5)
    assert not vals[:, 0].any() and vals[:, 1].any() and not cut.any()
    np.testing.assert_allclose(rr.block_totals(vals), vals.sum(axis=2), rtol=1e-13)


@pytest.mark.parametrize("name", ["chain64", "hky4"])
@pytest.mark.parametrize("sites", cases.UNCONDITIONED_SITES)
def test_gpu_unconditioned_inputs_need_no_exclusion(name, sites):
    Q, pi, regs = cases.unconditioned_cases()[name]
    _, near, cut = rr.unconditioned(Q, pi, cases.UNCONDITIONED_LENGTHS, sites, regs, cases.UNCONDITIONED_SEED)
    assert int(near.sum()) == 0 and not cut.any()
