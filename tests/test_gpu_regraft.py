"""Regraft scores in one call (include/beagle_mi355.h beagleMi355RegraftScores) on the HIP engine: the log ratios and the scores within
the bounds of the np.longdouble restatement (tests/regraft_reference.py) over the instance's own read-back partials and matrices,
the identity with the stock likelihood of the unpruned tree, the CPU oracle's evaluation of regrafted trees, the same bits whatever
the shape of the call, every return code, and the restated Gibbs operator through both routes.  The restatement itself is pinned on
the CPU tier (tests/test_regraft_host.py).

Bounds (eps = 2^-53; no sum of the formulas cancels): per pattern |R_dev - R_ld| <= 8 max(|R_f64 - R_ld|, (4 S + C + 12 + |R|) eps);
per score |s_dev - s_ld| <= 8 max(|s_f64 - s_ld|, Gamma) with Gamma the entries' bounds weighted by the pattern weights plus
P eps sum |w_p R_p|."""
import functools

import numpy as np
import pytest

import beast_mcmc_amd as bm
import helpers
import regraft_reference as ref
from beast_mcmc_amd.placement import log_likelihood
from beast_mcmc_amd.regraft import Regraft
from test_gpu_placement import environment, reducible_workload

pytestmark = pytest.mark.gpu

PARITY_TOL = 1e-10

# (S, C, P, tips): P at the block and T32 tile edges, S in both layouts and every kernel family, C 1 / 4 / 9, 8 to 24 tips
SHAPES = [(2, 1, 1, 8), (4, 4, 33, 8), (5, 9, 63, 10), (16, 4, 64, 12), (20, 1, 65, 24), (21, 4, 97, 9), (61, 4, 65, 8), (64, 1, 33, 8),
          (65, 9, 63, 8)]
KINDS = ["compact tip", "partials tip", "emission tip", "internal node"]


def movable(tree):
    return [n for n in range(tree.node_count) if n != tree.root and int(tree.parent[n]) != tree.root]


def build(S, C, P, T, library=None, seed=None, env=None, **kw):
    """An evaluation with every kind of tip, as tests/test_gpu_placement.py builds it: tip 0 held as partials, tip 1 behind an emission
    table of three codes (folded into its branch matrix on the engine), tip 2 unknown at every third pattern, the others compact
    states — on the first seeded tree in which the operator may move each of the three."""
    seed = 3000 + 7 * S + 3 * C + P if seed is None else seed
    while True:
        wl = helpers.random_workload(T, P, S, C, seed=seed, unknown_fraction=0.1)
        if all(int(wl.tree.parent[t]) != wl.tree.root for t in (0, 1, 2)):
            break
        seed += 1000
    wl.tip_states[2][::3] = S + 1
    rng = np.random.default_rng(seed + 1)
    with environment(**(env or {})):
        g = Regraft(wl, library=library, **kw)
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


def node_of(g, kind):
    return {"compact tip": 2, "partials tip": 0, "emission tip": 1}.get(kind, next(n for n in movable(g.tree) if n >= g.T))


def twins(g, rows=None):
    ops = g.read_back(rows)
    sub, logscale = g.read_subtree()
    w = g.wl.cat_weights
    r64, rld = ref.log_ratios(ops, sub, w, logscale), ref.log_ratios(ops, sub, w, logscale, dtype=np.longdouble)
    return r64, rld, ref.scores(r64, g.wl.weights), ref.scores(rld, g.wl.weights, dtype=np.longdouble)


def check_against_twins(g, dev_scores, dev_ratios, label, rows=None):
    r64, rld, s64, sld = twins(g, rows)
    ok_r, ratio_r = ref.within(dev_ratios, r64, rld, ref.gamma(rld, g.S, g.C))
    ok_s, ratio_s = ref.within(dev_scores, s64, sld, ref.score_bound(rld, g.wl.weights, g.S, g.C))
    print("%s: largest error over max(e_f64, bound): ratios %.3g, scores %.3g" % (label, ratio_r, ratio_s))
    assert ok_r, ratio_r
    assert ok_s, ratio_s


@functools.lru_cache(maxsize=None)
def instance(shape):
    g = build(*shape)
    g.unpruned = g.log_likelihood()
    return g


@functools.lru_cache(maxsize=None)
def evaluated(shape, kind):
    g = instance(shape)
    i = node_of(g, kind)
    lnl = g.prune(i)
    rows = g.regraft_candidates(i)
    scores, ratios, rc = g.log_ratios()
    return g, i, lnl, rows, list(g.candidate_nodes), scores, ratios, rc


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES)
def test_ratios_and_scores_within_the_bounds_of_the_longdouble_twin(shape, kind):
    g, i, lnl, rows, nodes, scores, ratios, rc = evaluated(shape, kind)
    S, C, P, T = shape
    assert rc == 0 and scores.shape == (len(rows),) and ratios.shape == (len(rows), P) and len(rows) >= 2
    assert np.isfinite(ratios).all() and np.isfinite(scores).all()
    g.prune(i)                                             # (the cached list of another kind may have been the last one evaluated)
    g.regraft_candidates(i)
    check_against_twins(g, scores, ratios, "%s %s" % (shape, kind))
    # the original position: the stock likelihood of the unpruned tree
    print(shape, kind, "lnL(T') + score[original]", lnl + scores[-1], "stock", g.unpruned)
    assert abs(lnl + scores[-1] - g.unpruned) <= PARITY_TOL * max(1.0, abs(g.unpruned))


@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[4], SHAPES[6]])
def test_against_the_oracle(shape, oracle_lib):
    for kind in ("emission tip", "internal node"):
        g, i, lnl, rows, nodes, scores, _, _ = evaluated(shape, kind)
        K = len(nodes)
        for k in sorted({0, K - 1, K // 2, 1}):
            moved = g.regrafted_workload(i, nodes[k])
            expect = log_likelihood(moved, partial_tips=g.tip_data, library=oracle_lib)
            print(shape, kind, nodes[k], "device", lnl + scores[k], "oracle", expect)
            assert abs(lnl + scores[k] - expect) <= PARITY_TOL * max(1.0, abs(expect))


def test_operands_not_stored_behind_a_held_list():
    """From the second evaluation of a chain on, the 4-state post-order passes leave short subtrees unstored and the pre-order list is
    held back: the call runs the list and materialises what it reads."""
    wl = helpers.random_workload(9, 257, 4, 4, seed=43)
    out = []
    for env in ({}, {"BEAGLE_MI355_NO_VIRTUAL": "1"}):
        with environment(**env):
            ev = Regraft(wl)
        i = next(n for n in movable(ev.tree) if n >= ev.T)
        for _ in range(3):
            ev.prune(i)
        rows = ev.regraft_candidates(i)                    # (spare matrix slots: the list stays held)
        late = ev.b.gradientStats()["late"]
        scores, ratios, rc = ev.log_ratios()
        held = ev.b.gradientStats()["late"] - late
        stats = ev.stats()
        print("materialised", stats["materialised"], "held lists run by the call", held)
        assert rc == 0 and stats["calls"] == 1 and stats["candidates"] == len(rows)
        if not env:
            assert held == 1
            assert stats["materialised"] > 0
            check_against_twins(ev, scores, ratios, "unstored operands")
        else:
            assert stats["materialised"] == 0
        out.append((scores, ratios))
        ev.close()
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])


def test_a_ladder_of_400_tips_with_rescaling():
    """Unscaled, the partials of a 400-tip ladder underflow at 20 states.  The subtree cut off is the ladder below the third node from
    the root: its own factors come through the named scale buffer, those of T' cancel in N / D, and the candidates sit near the
    root, where the (unscaled) pre-order partials are still numbers."""
    S, C, P, T = 20, 1, 33, 400
    wl = helpers.random_workload(T, P, S, C, seed=77, tree_kind="caterpillar", root_to_tip=4.0, unknown_fraction=0.0)
    plain = Regraft(wl, max_candidates=8)
    plain.b.updateTransitionMatrices(0, plain._edge_matrix[0], None, None, plain.branch_lengths[plain._nodes], len(plain._nodes))
    plain.b.updatePartials(plain._post_ops, len(plain._post_ops) // 7, -1)
    assert np.all(plain.b.getPartials(plain.post_index(wl.tree.root), -1) == 0.0)           # the unscaled root partial has underflowed
    plain.close()
    g = Regraft(wl, rescale=True, max_candidates=8)
    unpruned = g.log_likelihood()
    assert np.isfinite(unpruned)
    tr = wl.tree
    inner = lambda n: int(tr.left[n]) if tr.left[n] >= T else int(tr.right[n])           # noqa: E731
    i = inner(inner(inner(tr.root)))
    lnl = g.prune(i)
    assert g.subtree_scale != -1 and np.isfinite(lnl)
    assert np.all(g.b.getPartials(g.post_index(i), -1).max(axis=2) > 0.0)                   # ... while the scaled subtree's has not:
    assert np.all(g.b.getLogScaleFactors(g.subtree_scale) < -300.0)                         # what it lost is in its scale buffer
    rows = g.regraft_candidates(i)
    assert len(rows) >= 3
    scores, ratios, rc = g.log_ratios()
    assert rc == 0 and np.isfinite(scores).all() and np.isfinite(ratios).all()
    check_against_twins(g, scores, ratios, "400-tip ladder")
    assert abs(lnl + scores[-1] - unpruned) <= PARITY_TOL * max(1.0, abs(unpruned))
    g.close()


@pytest.mark.parametrize("S", [4, 20, 61])
def test_same_bits_under_different_call_shapes(S):
    g = build(S, 4, 97, 16)
    i = max((n for n in movable(g.tree) if 2 < n < g.T), key=lambda n: len(g.admissible(n)))       # a compact tip, the longest list
    g.prune(i)
    rows = g.regraft_candidates(i)
    K = len(rows)
    assert K > 7

    def call(r=rows, **kw):
        s, t, rc = g.b.regraftScores(r, g.post_index(i), g.subtree_scale, **kw)
        assert rc == 0
        return s, t

    first = call(pattern_log_ratios=True)
    again = call(pattern_log_ratios=True)
    assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1])                   # two calls
    order = np.random.default_rng(5).permutation(K)
    shuffled = call(rows[order], pattern_log_ratios=True)
    back = np.argsort(order)
    assert np.array_equal(first[0], shuffled[0][back]) and np.array_equal(first[1], shuffled[1][back])  # permuted, permuted back
    a, b = call(rows[:5], pattern_log_ratios=True), call(rows[5:], pattern_log_ratios=True)
    assert np.array_equal(first[0], np.concatenate([a[0], b[0]]))                                       # a list split in two
    assert np.array_equal(first[1], np.concatenate([a[1], b[1]], axis=0))
    launches = g.stats()["launches"]
    with environment(BEAGLE_MI355_REGRAFT_CHUNK="7"):
        chunked = call(pattern_log_ratios=True)
    assert g.stats()["launches"] - launches == 1 + 3 * ((K + 6) // 7)        # the pendant vector; per 7 candidates the ratios, the segments, their sum
    assert np.array_equal(first[0], chunked[0]) and np.array_equal(first[1], chunked[1])                # any chunk size
    bare = call()                                                                                      # R requested or not
    assert bare[1] is None and np.array_equal(first[0], bare[0])
    g.close()


def prune_through_a_zero(g, i):
    try:
        g.prune(i)
    except bm.beagle.BeagleException as e:                 # the root sum of an impossible pattern; both passes have run
        assert e.code == -8


def test_zero_denominators_and_zero_numerators():
    P, j = 70, 66
    probe = reducible_workload(P, None)
    i = next(n for n in movable(probe.tree) if 1 < n < probe.tree.tip_count)          # a tip other than the two that make pattern j impossible
    out = {}
    for name, impossible, weight in (("bad", j, None), ("good", None, None), ("bad at weight 0", j, 0.0), ("good at weight 0", None, 0.0)):
        wl = reducible_workload(P, impossible)
        if weight is not None:
            wl.weights = wl.weights.copy(); wl.weights[j] = weight
        g = Regraft(wl)
        prune_through_a_zero(g, i)
        g.regraft_candidates(i)
        out[name] = g.log_ratios()
        g.close()
    s_bad, r_bad, rc_bad = out["bad"]
    s_good, r_good, rc_good = out["good"]
    assert rc_bad == -8 and rc_good == 0
    # D = 0: the pattern's R of every candidate is NaN, and so is every score — nothing else changes
    others = np.arange(P) != j
    assert np.isnan(r_bad[:, j]).all() and np.isnan(s_bad).all()
    assert np.array_equal(r_bad[:, others], r_good[:, others]) and np.isfinite(r_good).all() and np.isfinite(s_good).all()
    # ... and at weight 0 it reaches no score: success, the scores of the possible data at the same weights bit for bit
    s_zero, r_zero, rc_zero = out["bad at weight 0"]
    assert rc_zero == 0 and np.isfinite(s_zero).all() and np.isnan(r_zero[:, j]).all()
    assert np.array_equal(s_zero, out["good at weight 0"][0]) and np.array_equal(r_zero[:, others], r_good[:, others])
    # N = 0: the subtree is a tip in the block no other tip is in at pattern 5: -inf and success
    wl = reducible_workload(P, None)
    wl.tip_states[i, 5] = 2
    g = Regraft(wl)
    g.prune(i)
    g.regraft_candidates(i)
    s, r, rc = g.log_ratios()
    assert rc == 0 and np.all(r[:, 5] == -np.inf) and np.all(s == -np.inf)
    assert np.array_equal(r[:, np.arange(P) != 5], r_good[:, np.arange(P) != 5])
    g.close()


def test_refusals():
    g = build(4, 2, 65, 8, double_buffer=True, rescale=True)
    i = next(n for n in movable(g.tree) if n >= g.T)
    g.prune(i)
    rows = g.regraft_candidates(i)
    assert len(rows) >= 4
    sub, scale = g.post_index(i), g.subtree_scale
    assert scale != -1
    watched = sorted(set(int(x) for x in rows[:, [0, 1, 3]].ravel() if x >= 0) | {sub})

    def snapshot():
        return [g.b.getPartials(x, -1).copy() for x in watched if x >= g.T or x in g.partial_tips]

    good = g.b.regraftScores(rows, sub, scale)                           # (the folded tip has its partials from here on)
    assert good[2] == 0
    before = snapshot()

    def code(r=rows, s=sub, sc=scale, **kw):
        with pytest.raises(bm.beagle.BeagleException) as e:
            g.b.regraftScores(r, s, sc, **kw)
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
    bad = rows.copy(); bad[2, 0] = 3                                     # parentPre holds compact tip states
    assert code(bad) == -5
    unwritten = g.T + (1 - g._set) * g._partial_set                      # the first internal buffer of the set no evaluation has used
    for column in (0, 1, 3):
        bad = rows.copy(); bad[3, column] = unwritten
        assert code(bad) == -5, column
    for s in (10 ** 6, -2, -1, unwritten):                               # the subtree: a bad index, none, a buffer never written
        assert code(s=s) == -5, s
    for sc in (10 ** 6, -2):                                             # a bad scale index (none is allowed)
        assert code(sc=sc) == -5, sc
    assert code(flags=1) == -5
    assert code(categoryWeightsIndex=7) == -5
    assert code(rows[:0]) == -5                                          # no candidate
    after = snapshot()
    assert len(after) == len(before) and all(np.array_equal(x, y) for x, y in zip(before, after))
    again = g.b.regraftScores(rows, sub, scale)                          # and the instance still answers, with the same bits
    assert again[2] == 0 and np.array_equal(again[0], good[0])
    # a partitioned instance, a BASTA instance, a sharded handle: not built (the fourth -7 case, more than 255 states, has no instance to
    # be tried on: beagleCreateInstance refuses such a state count)
    g.b.setPatternPartitions(2, (np.arange(65) // 33).astype(np.int32))
    assert code() == -7
    g.close()
    b = bm.beagle.Beagle(0, 8, 0, 3, 1, 2, 4, 1, 1)
    b.allocateCoalescentBuffers(5, 4, 12, 1)
    with pytest.raises(bm.beagle.BeagleException) as e:
        b.regraftScores([[1, -1, -1, 0, -1, 0, 1]], 2)
    assert e.value.code == -7
    b.finalize()
    all_gpus = len(bm.beagle.engine().resource_list()) - 1
    m = build(4, 2, 65, 8, env={"BEAGLE_MI355_SHARDS": "3"}, resource_list=(all_gpus,))
    with pytest.raises(bm.beagle.BeagleException) as e:
        m.b.regraftScores(rows, sub)
    assert e.value.code == -7
    m.close()


@pytest.mark.parametrize("pruned", [False, True])
@pytest.mark.parametrize("T", [12, 24])
@pytest.mark.parametrize("S,C,P", [(4, 4, 130), (20, 1, 65)])
def test_the_operator_through_both_routes(S, C, P, T, pruned):
    g = build(S, C, P, T)
    rng = np.random.default_rng(100 * T + S)
    nodes = movable(g.tree)
    drawn = 0
    for i in rng.choice(nodes, size=5, replace=False):
        u = float(rng.uniform(0.01, 0.99))
        g.prune(i)
        g.regraft_candidates(i)
        device_lnl, rc = g.scores(route="device")
        host_lnl, _ = g.scores(route="host")
        assert rc == 0
        tol = PARITY_TOL * np.maximum(1.0, np.abs(host_lnl))
        print(S, T, "node", int(i), "candidates", len(host_lnl), "largest |device - host| / max(1, |lnL|):",
              float(np.max(np.abs(device_lnl - host_lnl) / np.maximum(1.0, np.abs(host_lnl)))))
        assert np.all(np.abs(device_lnl - host_lnl) <= tol)
        try:
            j, hastings, prob = g.gibbs_proposal(i, u, pruned=pruned, route="device")
        except RuntimeError:                                             # an empty neighbourhood: the reference's refusal, on both routes
            with pytest.raises(RuntimeError):
                g.gibbs_proposal(i, u, pruned=pruned, route="host")
            continue
        j2, hastings2, prob2 = g.gibbs_proposal(i, u, pruned=pruned, route="host")
        drawn += 1
        worst = float(np.max(tol))
        assert len(prob) == len(prob2) and np.array_equal(prob == 0.0, prob2 == 0.0)        # (underflowed on both routes: log -inf on both)
        some = prob > 0.0
        assert np.all(np.abs(np.log(prob[some]) - np.log(prob2[some])) <= 2 * worst)
        assert abs(hastings - hastings2) <= 4 * worst
        if j != j2:                                                      # only where u falls on the boundary between two candidates
            edge = np.cumsum(prob)
            assert np.min(np.abs(edge - u)) <= 4 * worst
    assert drawn >= 1 or pruned
    g.close()
