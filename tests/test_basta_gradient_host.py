"""The BASTA gradient on the host: the reverse sweep beagleBastaGradient runs (basta_gradient_reference.adjoint) against the
reference's forward mode restated loop for loop (forward) and against central differences of the likelihood restatement in
numpy.longdouble (finite_difference); the chain rules by hand; the C ABI's declarations."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import basta_gradient_reference as gr
import basta_reference as br
import basta_states_cases as cases
import beast_mcmc_amd as bm
import helpers
from beast_mcmc_amd import basta
from beast_mcmc_amd.inputs import substmodel, trees

ROOT = helpers.ROOT


def make_tree(kind, tip_count):
    if kind == "ladder":
        return trees.caterpillar_tree(tip_count, root_height=2.0)
    if kind == "tied":                                       # two tips sampled at the same time
        if tip_count == 2:
            return trees.Tree([-1, -1, 0], [-1, -1, 1], [0.0, 0.0, 1.0], 2)
        if tip_count == 3:
            return trees.Tree([-1, -1, -1, 0, 3], [-1, -1, -1, 1, 2], [0.0, 0.0, 0.4, 0.7, 1.5], 4)
        tree = trees.heterochronous_coalescent_tree(tip_count, np.random.default_rng(5), sampling_span=1.0, population=3.0, tied=3)
        assert len(set(tree.height[:tip_count])) < tip_count
        return tree
    return trees.heterochronous_coalescent_tree(tip_count, np.random.default_rng(tip_count), sampling_span=1.0, population=3.0)


class Problem:
    """One evaluation in fp64 and everything the three gradients take."""

    def __init__(self, state_count, tree, sub, tips, seed, complex_eigen=False):
        rng = np.random.default_rng(seed)
        s, t = state_count, tree.tip_count
        self.tr = tr = basta.traverse(tree, cases.RATE, sub)
        if complex_eigen:
            q = np.array([[-1.0, 1.0, 0.0], [0.0, -0.7, 0.7], [1.3, 0.0, -1.3]])
            _, eig = substmodel.decompose_complex(q)
            assert np.any(eig.evals[3:] != 0.0)
            te = basta.transpose_eigen(eig)
            self.matrices = br.transition_matrices(te.evec, te.ievc, te.evals, tr.matrices)
        else:
            self.matrices = cases.matrices_for(cases.random_rates(s, rng), tr)
        self.sizes = rng.gamma(4.0, 0.5, size=s) + 0.05
        demes = rng.integers(0, s, size=t)
        self.tips = np.zeros((t, s))
        self.tips[np.arange(t), demes] = 1.0
        if tips == "ambiguous":
            for i in range(0, t, 2):
                on = rng.random(s) < 0.5
                on[demes[i]] = True
                self.tips[i] = on / on.sum()
        self.distances = basta.interval_distances(tr)
        _, self.partials, self.coalescent = br.evaluate(self.tips, tr.operations, tr.intervals, tr.lengths, self.matrices, self.sizes,
                                                        tr.buffer_count, tr.interval_count)

    def swept(self, function, dtype=np.float64):
        tr = self.tr
        return function(tr.operations, tr.intervals, tr.lengths, self.distances, self.partials, self.matrices, self.sizes, self.coalescent,
                        dtype=dtype)

    def differences(self):
        tr = self.tr
        return gr.finite_difference(self.tips, tr.operations, tr.intervals, tr.lengths, self.distances, self.matrices, self.sizes,
                                    tr.buffer_count, tr.interval_count)


def worst(a, b):
    """max |a - b| / max |b| over both gradients"""
    out = 0.0
    for key in ("theta", "migration"):
        x, y = np.asarray(a[key], dtype=np.longdouble), np.asarray(b[key], dtype=np.longdouble)
        out = max(out, float(np.abs(x - y).max() / np.abs(y).max()))
    return out


def check(problem, label):
    adjoint, forward, differences = problem.swept(gr.adjoint), problem.swept(gr.forward), problem.differences()
    figures = worst(adjoint, forward), worst(adjoint, differences), worst(forward, differences)
    print("%s: adjoint vs forward %.1e, adjoint vs differences %.1e, forward vs differences %.1e" % ((label,) + figures))
    assert np.all(np.isfinite(adjoint["migration"])) and np.abs(adjoint["migration"]).max() > 0.0
    assert figures[0] <= 1e-12
    assert figures[1] <= 1e-6 and figures[2] <= 1e-6


@pytest.mark.parametrize("tips", ["one-hot", "ambiguous"])
@pytest.mark.parametrize("sub", [1, 3])
@pytest.mark.parametrize("kind", ["heterochronous", "ladder", "tied"])
@pytest.mark.parametrize("tip_count", [2, 3, 7])
@pytest.mark.parametrize("state_count", [2, 3, 5])
def test_adjoint_forward_and_finite_differences_agree(state_count, tip_count, kind, sub, tips):
    if np.finfo(np.longdouble).eps >= np.finfo(np.float64).eps:
        pytest.skip("numpy.longdouble is no wider than float64 on this platform")
    problem = Problem(state_count, make_tree(kind, tip_count), sub, tips, seed=100 * state_count + 10 * tip_count + sub)
    check(problem, "S=%d T=%d %s sub=%d %s" % (state_count, tip_count, kind, sub, tips))


@pytest.mark.parametrize("sub", [1, 3])
def test_a_complex_eigen_system(sub):
    if np.finfo(np.longdouble).eps >= np.finfo(np.float64).eps:
        pytest.skip("numpy.longdouble is no wider than float64 on this platform")
    check(Problem(3, make_tree("heterochronous", 7), sub, "ambiguous", seed=9, complex_eigen=True), "complex sub=%d" % sub)


def test_the_adjoint_in_longdouble_is_the_fp64_one_to_rounding():
    problem = Problem(5, make_tree("heterochronous", 7), 3, "ambiguous", seed=3)
    assert worst(problem.swept(gr.adjoint), problem.swept(gr.adjoint, np.longdouble)) <= 1e-12


def test_a_second_forward_call_on_stale_storage_is_not_the_contract():
    """forward starts from zeroed storage every time: two calls, the same numbers (the reference's += into storage it never
    clears would give others)."""
    problem = Problem(3, make_tree("heterochronous", 3), 1, "one-hot", seed=1)
    first, second = problem.swept(gr.forward), problem.swept(gr.forward)
    assert np.array_equal(first["migration"], second["migration"]) and np.array_equal(first["theta"], second["theta"])


def test_chain_rules_by_hand():
    """Three demes.  W = [[1 2 3] [4 5 6] [7 8 9]], pi = (0.2, 0.3, 0.5): the upper triangle row by row, (W[i][j] - W[i][i]) pi_j =
    (2 - 1) 0.3, (3 - 1) 0.5, (6 - 5) 0.5; then the lower triangle column by column, (4 - 5) 0.2, (7 - 9) 0.2, (8 - 9) 0.3.
    G_theta = (2, -3, 0.5), N = (0.5, 2, 4): -G / N^2 = (-8, 0.75, -0.03125)."""
    w = np.arange(1.0, 10.0).reshape(3, 3)
    got = basta.migration_rate_chain_rule(w, [0.2, 0.3, 0.5])
    assert np.allclose(got, [0.3, 1.0, 0.5, -0.2, -0.4, -0.3], rtol=1e-15, atol=0.0)
    assert np.array_equal(basta.population_size_chain_rule([2.0, -3.0, 0.5], [0.5, 2.0, 4.0]), [-8.0, 0.75, -0.03125])


def test_interval_distances_follow_the_matrices():
    tree = make_tree("heterochronous", 7)
    tr = basta.traverse(tree, cases.RATE, 3)
    d = basta.interval_distances(tr)
    assert d.shape == tr.lengths.shape and np.allclose(d, cases.RATE * tr.lengths, rtol=1e-15)
    assert gr.matrix_times(tr.operations, tr.intervals, d) == dict(tr.matrices)


def test_the_header_declares_both_calls_and_they_are_bound_and_exported(engine_lib):
    hdr = open(os.path.join(ROOT, "include", "beagle_mi355.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in ("beagleBastaGradient", "beagleBastaGradientStats"):
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr)
        assert name in bm.beagle.ABI_SYMBOLS and hasattr(engine_lib.lib, name)
    assert hasattr(bm.beagle.Beagle, "bastaGradient") and hasattr(bm.beagle.Beagle, "bastaGradientStats")
    assert hasattr(basta.BastaLikelihood, "gradient")
    # the three natives stay declared as they were
    for name in ("UpdatePartialsGrad", "UpdateTransitionMatricesGrad", "AccumulatePartialsGrad"):
        assert "beagleBasta" + name in bm.beagle.ABI_SYMBOLS


def test_the_scratch_layout(tmp_path):
    exe = str(tmp_path / "basta_gradient_layout_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", os.path.join(ROOT, "tests", "native", "basta_gradient_layout_check.cpp"),
                           "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "basta_gradient_layout_check: OK" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]


def test_the_bench_tools_host_restatement_is_the_adjoint(tmp_path):
    """tools/basta_gradient_host_restatement.cpp: its adjoint sweep gives the numpy restatement's bits, its forward mode the same numbers
    to rounding (1e-12 of the largest entry, the bound of the numpy pair above)."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import basta_gradient_bench as bench
    finally:
        sys.path.pop(0)
    host = bench.host_library(str(tmp_path))
    for state_count, tip_count, sub in ((4, 12, 3), (9, 7, 1), (61, 5, 1)):
        x = cases.Inputs(state_count, tip_count, seed=3, tips="ambiguous", sub_intervals=sub)
        tr = x.traversal
        side = bench.HostSide(host, tr, x.tips, x.matrices, x.sizes, tr.buffer_count + 2)
        got, forward = side.adjoint()[1], side.forward()[1]
        want = gr.adjoint(tr.operations, tr.intervals, tr.lengths, side.distances, side.partials, x.matrices, x.sizes, side.coalescent)
        for key in ("adjoints", "theta", "migration"):
            assert np.array_equal(got[key], want[key]), (state_count, key)
        assert worst(forward, got) <= 1e-12


def test_gradient_needs_an_evaluation_first():
    like = basta.BastaLikelihood.__new__(basta.BastaLikelihood)
    like.traversal = None
    with pytest.raises(ValueError):
        like.gradient()
    with pytest.raises(ValueError):
        like.gradient(wrt="heights")
