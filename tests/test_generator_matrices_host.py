"""Transition matrices straight from generators, CPU tier: the two C ABI symbols and the document rows, and the numpy restatement of the
call's arithmetic (tests/generator_matrices_reference.py) pinned against the longdouble yardstick — every entry non-negative, the
chain's structural zeros exact, row sums and componentwise relative error within 8 (2^s + 20) eps — next to what the eigen route
(inputs.substmodel.decompose_complex) makes of the same generators, which is why the call exists."""
import os
import re

import numpy as np
import pytest

import beast_mcmc_amd as bm
import generator_matrices_reference as gr
import helpers
from beast_mcmc_amd import generators

SYMBOLS = ("beagleMi355UpdateTransitionMatricesFromGenerators", "beagleMi355GeneratorStats")
CASES = [(S, name) for S in (4, 20, 61) for name in ("dense", "bssvs", "stiff")] + [(8, "chain")]
IDS = ["S%d-%s" % c for c in CASES]


def _read(*path):
    return open(os.path.join(helpers.ROOT, *path)).read()


def test_header_exports_and_binding_name_the_calls():
    hdr = _read("include", "beagle_mi355.h")
    exports = _read("beast-mcmc_amd", "csrc", "exports.map")
    patterns = re.findall(r"^\s*([A-Za-z_*]+);", exports.split("local:")[0], re.M)
    for sym in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % sym, hdr)
        assert any(re.fullmatch(p.replace("*", ".*"), sym) for p in patterns)     # the version script lets it through
        assert sym in bm.beagle.ABI_SYMBOLS
    for method in ("updateTransitionMatricesFromGenerators", "generatorStats"):
        assert hasattr(bm.beagle.Beagle, method)
    assert generators.SYMBOL == SYMBOLS[0]


def test_library_exports_the_calls(engine_lib):
    for sym in SYMBOLS:
        assert hasattr(engine_lib.lib, sym)


def test_documents_carry_their_rows():
    assert re.search(r"^### 4\.14 .*beagleMi355UpdateTransitionMatricesFromGenerators", _read("DESIGN.md"), re.M)
    assert re.search(r"^\|.*beagleMi355UpdateTransitionMatricesFromGenerators", _read("README.md"), re.M)
    assert re.search(r"^\|.*beagleMi355UpdateTransitionMatricesFromGenerators", _read("SURVEY.md"), re.M)
    integration = _read("INTEGRATION.md")
    assert "beagleMi355UpdateTransitionMatricesFromGenerators" in integration and "BEAGLE_MI355_GENERATOR_CHUNK" in integration
    assert "generator_matrices_bench.py" in _read("tools", "README.md")


@pytest.mark.parametrize("x, s", [(0.0, 0), (0.75, 0), (1.0, 0), (1.0000000000000002, 1), (2.0, 1), (2.0000000000000004, 2), (3.0, 2),
                                  (4.0, 2), (2.0 ** 40, 40), (2.0 ** 40 * (1 + 2.0 ** -52), 41)])
def test_squarings_is_the_smallest_exponent_and_scaling_is_exact(x, s):
    got, tau = gr.squarings(x)
    assert got == s and tau * 2.0 ** s == x and tau <= 1.0
    assert s == 0 or x * 2.0 ** -(s - 1) > 1.0


def test_max_rate_scans_upwards():
    q = np.array([[-2.0, 2.0, 0.0], [1.0, -3.0, 2.0], [3.0, 0.0, -3.0]])
    assert gr.max_rate(q) == 3.0
    mu, table = gr.power_table(q)
    assert mu == 3.0 and len(table) == gr.TERMS
    assert np.array_equal(table[0], np.eye(3)) and np.array_equal(table[1], q / 3.0 + np.eye(3))
    assert np.array_equal(table[3], gr.mj.mm(gr.mj.mm(table[1], table[1]), table[1]))


@pytest.mark.parametrize("S, name", CASES, ids=IDS)
def test_restatement_against_the_yardstick(S, name):
    """The properties the device call inherits.  The worst case of these inputs: a relative error of 2.6e-10 at s = 23 (stiff, 61 states, d = 100)."""
    q = gr.generators(S)[name]
    for d in gr.LENGTHS:
        T, s = gr.restatement(q, d)
        Y, s2, e_ref = gr.reference(S, name, d)
        rows = float(np.abs(T.sum(axis=1) - 1.0).max())
        print("%s d = %-6g s = %2d  e_ref = %.2e  |row sum - 1| = %.2e  bound = %.2e" % (name, d, s, e_ref, rows, gr.bound(s)))
        assert s == s2 and s <= gr.MAX_SQUARINGS
        assert np.all(T >= 0.0)
        assert rows <= gr.bound(s)
        assert e_ref <= gr.bound(s)
        if d == 0.0:
            assert np.array_equal(T, np.eye(S))
        if name == "chain":
            assert np.all(T[np.tril_indices(S, -1)] == 0.0)               # structural zeros: exactly zero
            assert np.all(T[np.triu_indices(S)] > 0.0) or d == 0.0


def test_more_than_forty_squarings_is_nan():
    q = gr.chain(8)
    T, s = gr.restatement(q, 2.0 ** 40 * 1.5)
    assert s == 41 and np.all(np.isnan(T))
    T, s = gr.restatement(q, 2.0 ** 40)
    assert s == 40 and np.all(np.isfinite(T))


def test_eigen_route_gives_a_negative_probability_on_the_sparse_generator():
    """Why the call exists (1): U exp(D d) U^-1 of the 61-state BSSVS-like generator cancels — a "probability" below zero at one of the
    test's lengths at least — where the restatement has none (above)."""
    q = generators.normalised(gr.generators(61)["bssvs"])
    lowest = min(float(gr.eigen_route(q, d).min()) for d in gr.LENGTHS[1:])
    print("lowest entry of the eigen route: %.3e" % lowest)
    assert lowest < 0.0


def test_eigen_route_fails_on_the_defective_chain():
    """Why the call exists (2): the one-way chain is a single Jordan block.  Whatever an eigensolver returns for it, the product misses
    exp(Q d) by more than 0.1 in some entry (or is not finite, or the decomposition raises); the restatement's error there is as anywhere."""
    q = gr.chain(8)
    Y = np.asarray(gr.yardstick(q, 1.0), dtype=np.float64)
    try:
        w, V = np.linalg.eig(q)
        E = np.real(V @ np.diag(np.exp(w * 1.0)) @ np.linalg.inv(V))
        worst = float(np.abs(E - Y).max()) if np.all(np.isfinite(E)) else np.inf
    except np.linalg.LinAlgError:
        worst = np.inf
    print("eigen route on the chain: absolute error %.3e" % worst)
    assert worst > 0.1
    try:
        with np.errstate(all="ignore"):
            E2 = gr.eigen_route(q, 1.0)                                    # (decompose_complex normalises by a stationary rate of 0)
        worst2 = float(np.abs(E2 - Y).max()) if np.all(np.isfinite(E2)) else np.inf
    except (np.linalg.LinAlgError, ArithmeticError, IndexError, ValueError):
        worst2 = np.inf
    assert worst2 > 0.1


def test_host_route_on_the_oracle_is_the_eigen_sequence(oracle_lib):
    """GeneratorModelSet's host route on the CPU oracle: decompose_complex, setEigenDecomposition, updateTransitionMatrices — within
    the eigen route's own error of the yardstick on a dense generator; the device route needs the extension and says so."""
    S = 4
    q = generators.normalised(gr.generators(S)["dense"])
    models = generators.GeneratorModelSet(S, 1, route="host", library=oracle_lib)
    models.set_generator(0, q)
    b = bm.beagle.Beagle(2, 3, 2, S, 16, models.eigen_buffer_count, 8, 1, 0,
                         requirementFlags=bm.beagle.FLAG_EIGEN_COMPLEX, library=oracle_lib)
    try:
        b.setCategoryRates([1.0])
        lengths = [0.01, 0.5, 2.0]
        models.update_matrices(b, [0, 3, 5], lengths)
        for slot, d in zip([0, 3, 5], lengths):
            got = np.asarray(b.getTransitionMatrix(slot))[0]
            Y = np.asarray(gr.yardstick(q, d), dtype=np.float64)
            assert np.abs(got - Y).max() <= 1e-12
    finally:
        b.finalize()
    with pytest.raises(ValueError):
        generators.GeneratorModelSet(S, 1, route="device", library=oracle_lib)
    with pytest.raises(ValueError):
        models.update_matrices(b, [0], [0.1], route="device")
