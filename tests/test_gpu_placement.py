"""Placement scores in one call (include/beagle_mi355.h beagleMi355PlacementScores) on the HIP engine: the log table and the scores
within the issue's bounds of the np.longdouble restatement (tests/placement_reference.py) over the instance's own read-back partials
and matrices, within the project's parity tolerance of lnL(augmented tree) - lnL(tree) from the CPU oracle, the same bits whatever
the shape of the call, and every return code.  The restatement itself is pinned on the CPU tier (tests/test_placement_host.py).

Bounds (eps = 2^-53; no sum of the formulas cancels): per table entry |T_dev - T_ld| <= 8 max(|T_f64 - T_ld|, (3 S + C + 12 + |T|) eps);
per score |s_dev - s_ld| <= 8 max(|s_f64 - s_ld|, Gamma) with Gamma the entries' bounds added up plus siteCount eps sum |T_i|."""
import contextlib
import functools
import os

import numpy as np
import pytest

import beast_mcmc_amd as bm
import helpers
import placement_reference as ref
from beast_mcmc_amd.inputs.substmodel import EigenDecomposition
from beast_mcmc_amd.inputs.synth import Workload
from beast_mcmc_amd.placement import Placement, log_likelihood

pytestmark = pytest.mark.gpu

PARITY_TOL = 1e-10

# (S, C, P, tips, siteCount, queryCount, candidateCount): every value of every axis of the issue appears once at least — P at the
# block and T32 tile edges, S in both layouts and every kernel family, C 1 / 4 / 9, 8 to 24 tips
SHAPES = [(2, 1, 1, 8, 1, 1, 1), (4, 4, 33, 8, 257, 3, 15), (5, 9, 63, 10, 1000, 17, 16), (16, 4, 64, 12, 257, 3, 17),
          (20, 1, 65, 24, 1000, 3, 70), (21, 4, 97, 9, 257, 17, 15), (61, 4, 65, 8, 257, 3, 16), (64, 1, 33, 8, 257, 1, 17),
          (65, 9, 63, 8, 1, 3, 15)]


@contextlib.contextmanager
def environment(**values):
    old = {k: os.environ.get(k) for k in values}
    os.environ.update(values)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def code_table(S, rng, zero_row=False):
    """S + 1 codes: the states 0 .. S - 2, a partially ambiguous row (the last two states), a real-valued emission row; zero_row: one
    more, all zeros (an observation no state emits)."""
    rows = [np.eye(S)[s] for s in range(S - 1)] + [np.r_[np.zeros(S - 2), 1.0, 1.0], rng.uniform(0.05, 1.0, size=S)]
    if zero_row:
        rows.append(np.zeros(S))
    return np.stack(rows)


def build(S, C, P, T, library=None, seed=None, env=None, **kw):
    """An evaluation with every kind of tip: tip 0 held as partials, tip 1 behind an emission table of three codes (folded into its
    branch matrix on the engine), tip 2 unknown at every third pattern, the others compact states."""
    seed = 2000 + 7 * S + 3 * C + P if seed is None else seed
    wl = helpers.random_workload(T, P, S, C, seed=seed, unknown_fraction=0.1)
    wl.tip_states[2][::3] = S + 1
    rng = np.random.default_rng(seed + 1)
    with environment(**(env or {})):
        g = Placement(wl, library=library, **kw)
    g.tip_data = {0: rng.uniform(0.1, 1.0, size=(P, S))}
    g.set_tip_partials(0, g.tip_data[0])
    K = min(S, 3)
    table = rng.dirichlet(np.full(S, 0.5), size=K) * 0.9 + 0.1 / S
    codes = rng.integers(0, K, size=P)
    g.tip_data[1] = table[codes]
    if library is None:
        g.b.setTipEmission(1, codes, table)
    else:
        g.b.setTipPartials(1, table[codes].ravel())
    g.partial_tips.add(1)
    return g


def candidate_list(g, K):
    """K candidates: one (K odd) or two (K even) above the root, the others at a quarter and three quarters of branches spread over the
    tree — the root's children, tips and internal nodes among them."""
    above = (0.07,) if K % 2 else (0.07, 0.31)
    n = (K - len(above)) // 2
    tr = g.tree
    first = [int(tr.left[tr.root]), int(tr.right[tr.root]), 0, 1, 2, 3]
    edges = (first + [e for e in g.edges if e not in first])[:n]
    return g.candidates(edges=edges, fractions=(0.25, 0.75), above_root=above, pendant_lengths=0.13)


def queries(S, P, sites, Q, seed, X=None):
    rng = np.random.default_rng(seed)
    X = S + 1 if X is None else X
    pats = rng.integers(-1, P, size=sites).astype(np.int32) if sites > 1 else np.zeros(1, dtype=np.int32)
    codes = rng.integers(0, X, size=(Q, sites)).astype(np.uint8)
    codes[rng.random(codes.shape) < 0.05] = 255
    if sites == 1:
        codes[0, 0] = 0
    return pats, codes


def twins(g, table, pats, codes, rows=None):
    ops = g.read_back(rows)
    w = g.wl.cat_weights
    t64, tld = ref.log_tables(ops, w, table), ref.log_tables(ops, w, table, dtype=np.longdouble)
    return t64, tld, ref.scores(t64, pats, codes), ref.scores(tld, pats, codes, dtype=np.longdouble)


def check_against_twins(g, dev_table, dev_scores, table, pats, codes, label, rows=None):
    t64, tld, s64, sld = twins(g, table, pats, codes, rows)
    ok_t, ratio_t = ref.within(dev_table, t64, tld, ref.gamma(tld, g.S, g.C))
    ok_s, ratio_s = ref.within(dev_scores, s64, sld, ref.score_bound(tld, pats, codes, g.S, g.C))
    print("%s: largest error over max(e_f64, bound): table %.3g, scores %.3g" % (label, ratio_t, ratio_s))
    assert ok_t, ratio_t
    assert ok_s, ratio_s
    return tld, sld


@functools.lru_cache(maxsize=None)
def evaluated(shape):
    S, C, P, T, sites, Q, K = shape
    g = build(S, C, P, T)
    g.prepare()
    rows = candidate_list(g, K)
    table = code_table(S, np.random.default_rng(S))
    pats, codes = queries(S, P, sites, Q, seed=S + P)
    scores, logs, rc = g.b.placementScores(rows, pats, codes, table, log_table=True)
    return g, rows, table, pats, codes, scores, logs, rc


@pytest.mark.parametrize("shape", SHAPES)
def test_table_and_scores_within_the_bounds_of_the_longdouble_twin(shape):
    g, rows, table, pats, codes, scores, logs, rc = evaluated(shape)
    S, C, P, T, sites, Q, K = shape
    assert rc == 0 and scores.shape == (Q, K) and logs.shape == (K, P, S + 1)
    assert np.isfinite(logs).all() and np.isfinite(scores).all()
    check_against_twins(g, logs, scores, table, pats, codes, str(shape))
    # a query without a kept site scores exactly 0.0 everywhere
    none = g.b.placementScores(rows, pats, np.full((1, sites), 255, dtype=np.uint8), table)[0]
    assert np.array_equal(none, np.zeros((1, K)))


@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[4], SHAPES[6]])
def test_against_the_oracle(shape, oracle_lib):
    g, rows, table, pats, codes, scores, _, _ = evaluated(shape)
    S, C, P, T, sites, Q, K = shape
    for q, k in [(0, 0), (Q - 1, K - 1), (1 % Q, K // 2), (0, 1)]:
        aug = g.attach(codes[q], k, pats, table)
        tips = {t: x[aug.patterns] for t, x in g.tip_data.items()}
        a = log_likelihood(aug, partial_tips=tips, library=oracle_lib)
        b = log_likelihood(aug.base, partial_tips=tips, library=oracle_lib)
        print(shape, q, k, "device", scores[q, k], "oracle", a - b)
        assert abs(scores[q, k] - (a - b)) <= PARITY_TOL * max(1.0, abs(a))


def test_operands_not_stored_behind_a_held_list():
    """From the second evaluation of a chain on, the 4-state post-order passes leave short subtrees unstored and the pre-order list is
    held back: the call runs the list and materialises what it reads."""
    wl = helpers.random_workload(9, 257, 4, 4, seed=43)
    table = code_table(4, np.random.default_rng(2))
    pats, codes = queries(4, 257, 1000, 3, seed=8)
    out = []
    for env in ({}, {"BEAGLE_MI355_NO_VIRTUAL": "1"}):
        with environment(**env):
            ev = Placement(wl)
        rows = ev.candidates(fractions=(0.5,), above_root=(0.1,), pendant_lengths=0.2)       # (before the chain: the list stays held)
        for _ in range(3):
            ev.prepare()
        late = ev.b.gradientStats()["late"]
        scores, logs, rc = ev.b.placementScores(rows, pats, codes, table, log_table=True)
        held = ev.b.gradientStats()["late"] - late
        stats = ev.stats()
        print("materialised", stats["materialised"], "held lists run by the call", held)
        assert rc == 0 and stats["calls"] == 1 and stats["candidates"] == len(rows)
        if not env:
            assert held == 1
            assert stats["materialised"] > 0
            check_against_twins(ev, logs, scores, table, pats, codes, "unstored operands")
        else:
            assert stats["materialised"] == 0
        out.append((scores, logs))
        ev.close()
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])


def test_a_ladder_of_400_tips_with_rescaling():
    """Unscaled, the partials of a 400-tip ladder underflow at 20 states; the per-pattern scale factors cancel in N / D, so the scores of
    the rescaled instance are finite and are those of the restatement over the same scaled partials."""
    S, C, P, T = 20, 1, 33, 400
    wl = helpers.random_workload(T, P, S, C, seed=77, tree_kind="caterpillar", root_to_tip=4.0, unknown_fraction=0.0)
    table = code_table(S, np.random.default_rng(3))
    pats, codes = queries(S, P, 257, 3, seed=9)
    plain = Placement(wl, max_candidates=8)
    plain.b.updateTransitionMatrices(0, plain._edge_matrix[0], None, None, plain.branch_lengths[plain._nodes], len(plain._nodes))
    plain.b.updatePartials(plain._post_ops, len(plain._post_ops) // 7, -1)
    assert np.all(plain.b.getPartials(plain.post_index(wl.tree.root), -1) == 0.0)           # the unscaled root partial has underflowed
    plain.close()
    g = Placement(wl, rescale=True, max_candidates=8)
    assert np.isfinite(g.prepare())
    tr = wl.tree
    edges = [int(tr.left[tr.root]), int(tr.right[tr.root]), T - 2, T - 30, 2 * T - 10, 2 * T - 50]       # (the pre-order partials are unscaled: near the root)
    rows = g.candidates(edges=edges, fractions=(0.5,), above_root=(0.05,), pendant_lengths=0.1)
    scores, logs, rc = g.b.placementScores(rows, pats, codes, table, log_table=True)
    assert rc == 0 and np.isfinite(scores).all() and np.isfinite(logs).all()
    check_against_twins(g, logs, scores, table, pats, codes, "400-tip ladder")
    g.close()


@pytest.mark.parametrize("S", [4, 20, 61])
def test_same_bits_under_different_call_shapes(S):
    C, P, T, sites, Q, K = 4, 97, 9, 257, 17, 17
    g = build(S, C, P, T)
    g.prepare()
    rows = candidate_list(g, K)
    table = code_table(S, np.random.default_rng(S))
    pats, codes = queries(S, P, sites, Q, seed=S)

    def call(r=rows, c=codes):
        s, t, rc = g.b.placementScores(r, pats, c, table, log_table=True)
        assert rc == 0
        return s, t

    first = call()
    again = call()
    assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1])                   # two calls
    order = np.random.default_rng(5).permutation(K)
    shuffled = call(rows[order])
    back = np.argsort(order)
    assert np.array_equal(first[0], shuffled[0][:, back]) and np.array_equal(first[1], shuffled[1][back])     # permuted, permuted back
    a, b = call(rows[:5]), call(rows[5:])
    assert np.array_equal(first[0], np.concatenate([a[0], b[0]], axis=1))                               # a list split in two
    assert np.array_equal(first[1], np.concatenate([a[1], b[1]], axis=0))
    launches = g.stats()["launches"]
    with environment(BEAGLE_MI355_PLACEMENT_CHUNK="7", BEAGLE_MI355_PLACEMENT_QUERY_CHUNK="7"):
        chunked = call()
    assert g.stats()["launches"] - launches == 1 + 3 * (1 + 3 * 3)          # pendant tables; per 7 candidates a table and per 7 queries counts, product, sum
    assert np.array_equal(first[0], chunked[0]) and np.array_equal(first[1], chunked[1])                # any chunk size
    fewer = call(c=codes[:3])                                                                          # ... nor on the query count
    assert np.array_equal(first[0][:3], fewer[0])
    g.close()


def reducible_workload(P, impossible):
    """Two blocks of two states that no branch joins (the eigen system written out, so the cross-block entries of every transition
    matrix are sums of exact zeros); every pattern inside the first block but `impossible`, whose first two tips sit in different ones."""
    wl = helpers.random_workload(6, P, 4, 2, seed=12)
    r = np.sqrt(0.5)
    evec = np.array([[r, r, 0, 0], [r, -r, 0, 0], [0, 0, r, r], [0, 0, r, -r]])
    eig = EigenDecomposition(evec, evec.T.copy(), np.array([0.0, -2.0, 0.0, -3.0]))
    states = np.where(wl.tip_states >= 4, wl.tip_states, wl.tip_states % 2).astype(np.int32)
    if impossible is not None:
        states[0, impossible], states[1, impossible] = 0, 2
    return Workload("reducible", wl.tree, eig, np.full(4, 0.25), wl.cat_rates, wl.cat_weights, states, wl.weights, 4)


def prepare_through_a_zero(g):
    try:
        g.prepare()
    except bm.beagle.BeagleException as e:                 # the root sum of an impossible pattern; the post-order partials are there
        assert e.code == -8
        g.b.setPartials(g.pre_offset + g.tree.root, g._root_pre)
        g.b.updatePrePartials(g._pre_ops, len(g._pre_ops) // 7, -1)


def test_zero_denominators_and_zero_numerators():
    P, j = 70, 66
    table = code_table(4, np.random.default_rng(4), zero_row=True)                    # code 5: no state emits it; codes 2 and 3: states of the
                                                                                      # block no pattern is in, as impossible
    pats = np.arange(P, dtype=np.int32)
    codes = np.zeros((3, P), dtype=np.uint8)                                          # query 0: state 0 everywhere
    codes[1, j] = 255                                                                 # query 1 does not use pattern j
    codes[2] = codes[1]; codes[2, 3] = 5                                              # query 2 observes the impossible at pattern 3
    out = []
    for impossible in (j, None):
        g = Placement(reducible_workload(P, impossible))
        prepare_through_a_zero(g)
        rows = g.candidates(fractions=(0.5,), above_root=(0.1,), pendant_lengths=0.2)
        out.append(g.b.placementScores(rows, pats, codes, table, log_table=True))
        g.close()
    (s_bad, t_bad, rc_bad), (s_good, t_good, rc_good) = out
    assert rc_bad == -8 and rc_good == 0
    # D = 0: the pattern's row of every candidate's table is NaN, and so is the score of the query that uses it — nothing else
    assert np.isnan(t_bad[:, j]).all() and np.isnan(s_bad[0]).all()
    others = np.arange(P) != j
    assert np.array_equal(t_bad[:, others], t_good[:, others])
    assert np.array_equal(s_bad[1:], s_good[1:])
    # N = 0: -inf and success; it reaches the query that observes it alone
    assert np.all(t_good[:, :, [2, 3, 5]] == -np.inf) and np.isfinite(t_good[:, :, [0, 1, 4]]).all()
    assert np.all(s_good[2] == -np.inf) and np.isfinite(s_good[:2]).all()


def test_refusals():
    g = build(4, 2, 65, 8, double_buffer=True)
    g.prepare()
    rows = candidate_list(g, 15)
    table = code_table(4, np.random.default_rng(6))
    pats, codes = queries(4, 65, 257, 3, seed=6)
    watched = sorted(set(int(x) for x in rows[:, [0, 1, 3]].ravel() if x >= 0))

    def snapshot():
        return [g.b.getPartials(x, -1).copy() for x in watched if x >= g.T or x in g.partial_tips]

    good = g.b.placementScores(rows, pats, codes, table)                 # (the folded tip has its partials from here on)
    assert good[2] == 0
    before = snapshot()

    def code(r=rows, p=pats, c=codes, t=table, **kw):
        with pytest.raises(bm.beagle.BeagleException) as e:
            g.b.placementScores(r, p, c, t, **kw)
        return e.value.code

    for column in range(7):
        for value in (10 ** 6, -2):
            bad = rows.copy(); bad[3, column] = value
            assert code(bad) == -5, (column, value)
    for column in (0, 3, 5, 6):                                          # only the sibling pair and the upper matrix may be NONE
        bad = rows.copy(); bad[3, column] = -1
        assert code(bad) == -5, column
    bad = rows.copy(); bad[3, 1] = -1                                    # a sibling's matrix without the sibling
    assert code(bad) == -5
    bad = rows.copy(); bad[4, 0] = 3                                     # parentPre holds compact tip states
    assert code(bad) == -5
    unwritten = g.T + (1 - g._set) * g._partial_set                      # the first internal buffer of the set no evaluation has used
    for column in (0, 1, 3):
        bad = rows.copy(); bad[3, column] = unwritten
        assert code(bad) == -5, column
    p = pats.copy(); p[5] = 65
    assert code(p=p) == -5                                               # a pattern index >= P
    p[5] = -2
    assert code(p=p) == -5
    c = codes.copy(); c[1, 7] = 5
    assert code(c=c) == -5                                               # a code >= codeCount other than 255
    assert code(flags=1) == -5
    assert code(categoryWeightsIndex=7) == -5
    assert code(rows[:0]) == -5                                          # no candidate
    after = snapshot()
    assert len(after) == len(before) and all(np.array_equal(x, y) for x, y in zip(before, after))
    again = g.b.placementScores(rows, pats, codes, table)                # and the instance still answers, with the same bits
    assert again[2] == 0 and np.array_equal(again[0], good[0])
    # a partitioned instance, a BASTA instance, a sharded handle: not built (the fourth -7 case, more than 255 states, has no instance to
    # be tried on: beagleCreateInstance refuses such a state count)
    g.b.setPatternPartitions(2, (np.arange(65) // 33).astype(np.int32))
    assert code() == -7
    g.close()
    b = bm.beagle.Beagle(0, 8, 0, 3, 1, 2, 4, 1, 1)
    b.allocateCoalescentBuffers(5, 4, 12, 1)
    with pytest.raises(bm.beagle.BeagleException) as e:
        b.placementScores([[1, -1, -1, 0, -1, 0, 1]], [0], [[0]], np.eye(3))
    assert e.value.code == -7
    b.finalize()
    all_gpus = len(bm.beagle.engine().resource_list()) - 1
    m = build(4, 2, 65, 8, env={"BEAGLE_MI355_SHARDS": "3"}, resource_list=(all_gpus,))
    m.prepare()
    with pytest.raises(bm.beagle.BeagleException) as e:
        m.b.placementScores(candidate_list(m, 3), pats, codes, table)
    assert e.value.code == -7
    m.close()
