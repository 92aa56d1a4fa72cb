"""CPU tier of the regraft scores (include/beagle_mi355.h beagleMi355RegraftScores): the numpy restatement the GPU tests use
(tests/regraft_reference.py) over the CPU oracle's read-back partials of the pruned tree against what the score means — the oracle's
own evaluation of the regrafted tree — its float64 twin against its np.longdouble twin, the package's restatement of the reference's
Gibbs operator through the host route against the same function fed the restated scores, the selection rule on hand-made vectors,
and the declarations."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import beast_mcmc_amd as bm
import helpers
import regraft_reference as ref
from beast_mcmc_amd.placement import log_likelihood
from beast_mcmc_amd.regraft import Regraft, node_distance, select

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("beagleMi355RegraftScores", "beagleMi355RegraftStats")
PARITY_TOL = 1e-10                                        # the project's parity constant

CASES = [(4, 4, False), (4, 1, True), (20, 1, False), (20, 4, True), (61, 2, False), (61, 1, True)]       # (states, categories, rescaled)


def movable(tree):
    """Nodes the operator may pick: not the root, not a child of the root."""
    return [n for n in range(tree.node_count) if n != tree.root and int(tree.parent[n]) != tree.root]


def pick(tree, internal):
    T = tree.tip_count
    return next(n for n in movable(tree) if (n >= T) == internal)


def setting(S, C, rescale, T=9, P=7):
    wl = helpers.random_workload(T, P, S, C, seed=500 + 7 * S + C)
    return Regraft(wl, library=helpers.oracle_library(), rescale=rescale)


def restated(g, dtype=np.float64):
    """lnL per row of the last list from the restatement over what the instance holds after prune()."""
    sub, logscale = g.read_subtree()
    R = ref.log_ratios(g.read_back(), sub, g.wl.cat_weights, logscale, dtype=dtype)
    return R, ref.scores(R, g.wl.weights, dtype=dtype)


@pytest.mark.parametrize("S,C,rescale", CASES)
@pytest.mark.parametrize("internal", [False, True])
def test_restatement_is_the_oracle_likelihood_of_the_regrafted_tree(S, C, rescale, internal):
    g = setting(S, C, rescale)
    lib = helpers.oracle_library()
    i = pick(g.tree, internal)
    lnl_pruned = g.prune(i)
    g.regraft_candidates(i)
    assert len(g.candidate_nodes) >= 2 and (g.subtree_scale != -1) == (rescale and internal)
    R, s = restated(g)
    assert np.isfinite(R).all()
    worst = 0.0
    for k, j in enumerate(g.candidate_nodes):
        expect = log_likelihood(g.regrafted_workload(i, j), library=lib, rescale=rescale)
        worst = max(worst, abs(lnl_pruned + s[k] - expect) / max(1.0, abs(expect)))
        assert abs(lnl_pruned + s[k] - expect) <= PARITY_TOL * max(1.0, abs(expect)), (k, j)
    # the last row is the original position: the unmoved tree
    unmoved = log_likelihood(g.wl, library=lib, rescale=rescale)
    assert abs(lnl_pruned + s[-1] - unmoved) <= PARITY_TOL * max(1.0, abs(unmoved))
    print(S, C, rescale, internal, "largest |lnL(T') + score - lnL(regrafted)| / max(1, |lnL|):", worst)
    # the float64 twin within the bounds of the longdouble twin
    Rld, sld = restated(g, np.longdouble)
    assert np.all(np.abs(R - Rld) <= ref.gamma(Rld, S, C))
    bound = ref.score_bound(Rld, g.wl.weights, S, C)
    assert np.all(np.abs(s - sld) <= bound)
    ok, ratio = ref.within(s, s, sld, bound)
    assert ok and ratio <= 1.0
    g.close()


def test_a_pattern_of_weight_zero_adds_nothing():
    R = np.array([[-1.5, np.nan, -0.25], [-2.0, -np.inf, -3.0]])
    w = np.array([2.0, 0.0, 3.0])
    assert np.array_equal(ref.scores(R, w), [2.0 * -1.5 + 3.0 * -0.25, 2.0 * -2.0 + 3.0 * -3.0])
    assert np.isnan(ref.scores(R, np.ones(3))[0]) and ref.scores(R, np.ones(3))[1] == -np.inf


@pytest.mark.parametrize("S,C,rescale", [(4, 4, False), (20, 1, True)])
@pytest.mark.parametrize("pruned", [False, True])
def test_gibbs_proposal_through_the_host_route_and_from_the_restated_scores(S, C, rescale, pruned):
    g = setting(S, C, rescale, T=12)
    g.max_distance = 3                                    # (nodeCount / 10 = 2 leaves the small tree's neighbourhoods nearly empty)
    lib = helpers.oracle_library()
    for trial, i in enumerate(movable(g.tree)[::4]):
        u = [0.03, 0.41, 0.77, 0.999][trial % 4]
        try:
            j, hastings, prob = g.gibbs_proposal(i, u, pruned=pruned, route="host")
        except RuntimeError:                              # an empty forward neighbourhood: the reference's refusal, on both sides
            g.prune(i); g.regraft_candidates(i)
            with pytest.raises(RuntimeError):
                g.proposal_from_scores(i, u, g.lnl_pruned + restated(g)[1], pruned=pruned)
            continue
        assert g.host_evaluations > 0
        # the host route's values are ordinary evaluations of the moved trees
        host_lnl, _ = (g.prune(i), g.regraft_candidates(i), g.scores(route="host"))[2]
        for k in (0, len(host_lnl) - 1):
            expect = log_likelihood(g.regrafted_workload(i, g.candidate_nodes[k]), library=lib, rescale=rescale)
            assert abs(host_lnl[k] - expect) <= PARITY_TOL * max(1.0, abs(expect))
        g.prune(i)
        g.regraft_candidates(i)
        lnl = g.lnl_pruned + restated(g)[1]
        assert np.all(np.abs(lnl - host_lnl) <= PARITY_TOL * np.maximum(1.0, np.abs(host_lnl)))
        j2, hastings2, prob2 = g.proposal_from_scores(i, u, lnl, pruned=pruned)
        tol = PARITY_TOL * max(1.0, float(np.max(np.abs(host_lnl))))
        assert j2 == j and len(prob) == len(prob2)
        some = prob > 0.0                                 # (a probability that underflowed does so on both sides: log -inf on both)
        assert np.array_equal(some, prob2 > 0.0) and np.all(np.abs(np.log(prob[some]) - np.log(prob2[some])) <= 2 * tol)
        assert abs(hastings - hastings2) <= 4 * tol
        assert abs(float(np.sum(prob)) - 1.0) <= 1e-12
    g.close()


def test_the_neighbourhoods_of_the_pruned_variant():
    """The forward neighbourhood is cut by distance on the tree as it stands, the backward one on the moved tree; the unlimited
    variant's Hastings ratio is that of the pruned variant with a distance nothing exceeds."""
    g = setting(4, 1, False, T=12)
    i = pick(g.tree, True)
    g.prune(i)
    g.regraft_candidates(i)
    lnl = g.lnl_pruned + restated(g)[1]
    g.max_distance = 10 ** 6
    a, b = g.proposal_from_scores(i, 0.5, lnl, pruned=False), g.proposal_from_scores(i, 0.5, lnl, pruned=True)
    assert a[0] == b[0] and abs(a[1] - b[1]) <= 1e-12 and np.allclose(a[2], b[2], rtol=0, atol=1e-15)
    tr = g.tree
    iP = int(tr.parent[i])
    assert g.admissible(i, 2) == [j for j in g.admissible(i) if node_distance(tr.parent, tr.height, iP, int(tr.parent[j])) <= 2]
    assert node_distance(tr.parent, tr.height, iP, iP) == 0 and node_distance(tr.parent, tr.height, iP, int(tr.parent[iP])) == 1
    with pytest.raises(ValueError):
        g.prune(tr.root)
    with pytest.raises(ValueError):
        g.prune(int(tr.left[tr.root]))
    g.close()


def test_the_selection_rule():
    p = [0.2, 0.5, 0.3]
    assert [select(p, u) for u in (1e-9, 0.19, 0.21, 0.69, 0.71, 0.9999)] == [0, 0, 1, 1, 2, 2]
    assert select(p, 0.0) == -1                           # ran = 0 subtracts nothing: the reference's index-- from 0, as written
    assert select([0.0, 0.0, 4.0], 0.5) == 2 and select([3.0], 0.999) == 0
    assert select([1e-99, 1e-99], 0.75) == 1              # just above the threshold
    for bad in ([], [0.0], [1e-101, 2e-101], [1e-100]):
        with pytest.raises(RuntimeError):
            select(bad, 0.5)


def test_the_entry_points_are_declared_bound_and_documented():
    header = open(os.path.join(ROOT, "include", "beagle_mi355.h")).read()
    exports = open(os.path.join(ROOT, "beast-mcmc_amd", "csrc", "exports.map")).read()
    for sym in SYMBOLS:
        assert "int %s(" % sym in header
        assert sym in bm.beagle.ABI_SYMBOLS
        assert "beagle*;" in exports and sym.startswith("beagle")
    for doc in ("DESIGN.md", "README.md", "SURVEY.md", "INTEGRATION.md"):
        assert SYMBOLS[0] in open(os.path.join(ROOT, doc)).read(), doc
    assert hasattr(bm.beagle.Beagle, "regraftScores") and hasattr(bm.beagle.Beagle, "regraftStats") and hasattr(bm.regraft, "Regraft")
    # the header's prototype, argument by argument, against the types the binding passes
    proto = re.search(r"int beagleMi355RegraftScores\(([^)]*)\);", header).group(1)
    kinds = ["p" if "*" in a else "i" for a in proto.split(",")]
    assert kinds == list("ipiiiiipp")
    assert "[candidateCount][7]" in header and "BEAGLE_MI355_REGRAFT_CHUNK" in header and "segments of 64 patterns" in header

    class Recorder:
        def __getattr__(self, name):
            self.f = lambda *a: 0
            return self.f
    b = bm.beagle.Beagle.__new__(bm.beagle.Beagle)
    b.lib = type("L", (), {"lib": Recorder()})()
    b.instance, b.patternCount = 0, 3
    s, r, rc = b.regraftScores(np.zeros((2, 7), dtype=np.int32), 5, pattern_log_ratios=True)
    assert rc == 0 and s.shape == (2,) and r.shape == (2, 3)
    want = [ctypes.c_int, ctypes.POINTER(ctypes.c_int)] + [ctypes.c_int] * 5 + [ctypes.POINTER(ctypes.c_double)] * 2
    assert list(b.lib.lib.f.argtypes) == want


def test_the_scratch_layout(tmp_path):
    exe = str(tmp_path / "regraft_layout_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
                           os.path.join(ROOT, "tests", "native", "regraft_layout_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "regraft_layout_check: OK" in out.stdout
