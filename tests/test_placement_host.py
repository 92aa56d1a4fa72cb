"""CPU tier of the placement scores (include/beagle_mi355.h beagleMi355PlacementScores): the package's host route over the CPU oracle
against what the score means — lnL(tree with the query attached) - lnL(tree), both from ordinary evaluations of the oracle — the
float64 restatement the GPU tests use (tests/placement_reference.py) against its np.longdouble twin, the reference's distance rule
on a hand-counted case, and the sites that must add exactly nothing."""
import os
import subprocess

import numpy as np
import pytest

import beast_mcmc_amd as bm
import helpers
import placement_reference as ref
from beast_mcmc_amd.placement import Placement, log_likelihood

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("beagleMi355PlacementScores", "beagleMi355PlacementStats")
PARITY_TOL = 1e-10                                        # the project's parity constant

CASES = [(4, 1, False), (4, 4, True), (5, 4, False), (5, 1, True), (20, 1, False), (20, 4, True)]       # (states, categories, rescaled)


def code_table(S, rng):
    """S + 1 codes: the states 0 .. S - 2, a partially ambiguous row (the last two states), a real-valued emission row."""
    return np.stack([np.eye(S)[s] for s in range(S - 1)] + [np.r_[np.zeros(S - 2), 1.0, 1.0], rng.uniform(0.05, 1.0, size=S)])


def setting(S, C, rescale, T=7, P=9, sites=40, Q=2):       # (an odd number of tips: some node has a tip and an internal child)
    wl = helpers.random_workload(T, P, S, C, seed=300 + 7 * S + C)
    g = Placement(wl, library=helpers.oracle_library(), rescale=rescale)
    g.prepare()
    tr = wl.tree
    # a root child's branch, a tip child under a tip sibling (a cherry), a tip child under an internal sibling, an internal child, above the root
    cherry = next(n for n in range(T, tr.node_count) if tr.left[n] < T and tr.right[n] < T)
    mixed = next(n for n in range(T, tr.node_count) if (tr.left[n] < T) != (tr.right[n] < T))
    tip_of_mixed = int(tr.left[mixed] if tr.left[mixed] < T else tr.right[mixed])
    inner_of_mixed = int(tr.right[mixed] if tr.left[mixed] < T else tr.left[mixed])
    edges = [int(tr.left[tr.root]), int(tr.right[tr.root]), int(tr.left[cherry]), tip_of_mixed, inner_of_mixed]
    g.candidates(edges=edges, fractions=(0.3, 0.8), above_root=(0.07,), pendant_lengths=0.11)
    rng = np.random.default_rng(S + C)
    table = code_table(S, rng)
    pats = rng.integers(-1, P, size=sites).astype(np.int32)
    codes = rng.integers(0, S + 1, size=(Q, sites)).astype(np.uint8)
    codes[0, 3] = 255
    return g, table, pats, codes


@pytest.mark.parametrize("S,C,rescale", CASES)
def test_host_route_is_the_difference_of_two_oracle_likelihoods(S, C, rescale):
    g, table, pats, codes = setting(S, C, rescale)
    scores, rc = g.scores(pats, codes, table, route="host")
    assert rc == 0 and scores.shape == (2, 11)
    lib = helpers.oracle_library()
    worst = 0.0
    for q in range(2):
        for k in range(scores.shape[1]):
            aug = g.attach(codes[q], k, pats, table)
            a, b = log_likelihood(aug, library=lib, rescale=rescale), log_likelihood(aug.base, library=lib, rescale=rescale)
            worst = max(worst, abs(scores[q, k] - (a - b)) / max(1.0, abs(a)))
            assert abs(scores[q, k] - (a - b)) <= PARITY_TOL * max(1.0, abs(a)), (q, k)
    print(S, C, rescale, "largest |score - (lnL_aug - lnL_tree)| / max(1, |lnL_aug|):", worst)
    g.close()


@pytest.mark.parametrize("S,C,rescale", CASES)
def test_float64_twin_within_the_bounds_of_the_longdouble_twin(S, C, rescale):
    g, table, pats, codes = setting(S, C, rescale)
    ops = g.read_back()
    host = g.log_table(table, route="host")[0]
    g.close()
    w = g.wl.cat_weights
    t64, tld = ref.log_tables(ops, w, table), ref.log_tables(ops, w, table, dtype=np.longdouble)
    assert np.isfinite(t64).all()
    assert np.all(np.abs(t64 - tld) <= ref.gamma(tld, S, C))
    assert np.all(np.abs(host - tld) <= ref.gamma(tld, S, C))                       # the package's einsum form of the same formulas
    s64, sld = ref.scores(t64, pats, codes), ref.scores(tld, pats, codes, dtype=np.longdouble)
    bound = ref.score_bound(tld, pats, codes, S, C)
    print(S, C, "table error / gamma:", float(np.max(np.abs(t64 - tld) / ref.gamma(tld, S, C))), "score error / Gamma:",
          float(np.max(np.abs(s64 - sld) / bound)))
    assert np.all(np.abs(s64 - sld) <= bound)
    ok, ratio = ref.within(s64, s64, sld, bound)
    assert ok and ratio <= 1.0


def test_missing_codes_and_skipped_sites_add_exactly_nothing():
    g, table, pats, codes = setting(4, 4, False)
    pats[5] = 2                                            # (a kept site under the missing code below)
    codes[1, 5] = 255
    keep = pats >= 0
    assert (~keep).any() and (codes == 255).any()
    full, _ = g.scores(pats, codes, table, route="host")
    dropped, _ = g.scores(pats[keep], codes[:, keep], table, route="host")
    assert np.array_equal(full, dropped)
    t64 = ref.log_tables(g.read_back(), g.wl.cat_weights, table)
    assert np.array_equal(ref.scores(t64, pats, codes), ref.scores(t64, pats[keep], codes[:, keep]))
    # a query with no kept site at all: exactly 0.0; a site under code 255 removed from one query alone
    nothing = np.full((1, len(pats)), 255, dtype=np.uint8)
    assert np.array_equal(g.scores(pats, nothing, table, route="host")[0], np.zeros((1, full.shape[1])))
    assert np.array_equal(ref.scores(t64, pats, nothing), np.zeros((1, full.shape[1])))
    one = codes[1:2].copy()
    without = np.arange(len(pats)) != 5
    assert np.array_equal(ref.scores(t64, pats, one), ref.scores(t64, pats[without], one[:, without]))
    # ... and an entry of the table that no site of a query uses never reaches its score
    t = t64.copy()
    unused = [(p, x) for p in range(t.shape[1]) for x in range(t.shape[2]) if not np.any((pats == p) & (codes[0] == x))][0]
    t[:, unused[0], unused[1]] = np.nan
    assert np.array_equal(ref.scores(t, pats, codes[:1]), ref.scores(t64, pats, codes[:1]))
    g.close()


def test_distance_route_on_a_hand_counted_case():
    """Three taxa over six sites, nucleotides; codes 0..3 the states, 4 an ambiguity (A or G), 5 a gap row of ones named as a gap code.
        taxon 0:  A C G T A -      taxon 1:  A C G T C C      taxon 2:  - - - - - -     (- : a state >= 4)
    query 0  =   A C G T A C   identical to taxon 0 where both are counted: 0 / 5, against taxon 1: 1 / 6, taxon 2: 0 / 0 = NaN -> taxon 0, 0.0
    query 1  =   R C T T gap C   (R ambiguous: counted, never a difference; the gap site is not counted)
                 taxon 0: sites 0 1 2 3 counted (site 4 the query's gap, site 5 the taxon's), difference at site 2: 1 / 4
                 taxon 1: sites 0 1 2 3 5 counted, difference at site 2: 1 / 5 -> taxon 1, 0.2
    query 2  =   skipped site 0 (pattern -1); C C G T A C -> taxon 0: sites 1..4 counted, 0 differences: 0 / 4 = 0.0 (taxon 1: 1 / 5)"""
    wl = helpers.random_workload(3, 6, 4, 1, seed=3)
    wl.tip_states[:] = np.array([[0, 1, 2, 3, 0, 4], [0, 1, 2, 3, 1, 1], [4, 4, 4, 4, 4, 4]], dtype=np.int32)
    g = Placement(wl, library=helpers.oracle_library())
    table = np.concatenate([np.eye(4), [[1.0, 0.0, 1.0, 0.0]], [[1.0, 1.0, 1.0, 1.0]]])
    codes = np.array([[0, 1, 2, 3, 0, 1], [4, 1, 3, 3, 5, 1]], dtype=np.uint8)
    closest, d = g.distances(np.arange(6), codes, table, gap_codes=(255, 5))
    assert closest.tolist() == [0, 1] and d.tolist() == [0.0, 0.2]
    closest, d = g.scores(np.array([-1, 1, 2, 3, 4, 5]), np.array([[1, 1, 2, 3, 0, 1]], dtype=np.uint8), table, route="distance")
    assert closest.tolist() == [0] and d.tolist() == [0.0]
    # identical sequences: distance exactly 0.0, the FIRST such taxon (strictly smaller wins)
    wl.tip_states[2] = wl.tip_states[0]
    closest, d = g.distances(np.arange(6), codes[:1], table)
    assert closest.tolist() == [0] and d.tolist() == [0.0]
    g.close()


def test_the_entry_points_are_declared_bound_and_documented():
    header = open(os.path.join(ROOT, "include", "beagle_mi355.h")).read()
    for sym in SYMBOLS:
        assert "int %s(" % sym in header
        assert sym in bm.beagle.ABI_SYMBOLS
    for doc in ("DESIGN.md", "README.md", "SURVEY.md"):
        assert SYMBOLS[0] in open(os.path.join(ROOT, doc)).read(), doc
    assert hasattr(bm.beagle.Beagle, "placementScores") and hasattr(bm.placement, "Placement")


def test_the_scratch_layout(tmp_path):
    exe = str(tmp_path / "placement_layout_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
                           os.path.join(ROOT, "tests", "native", "placement_layout_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "placement_layout_check: OK" in out.stdout
