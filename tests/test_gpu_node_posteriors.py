"""Marginal node state posteriors in one call (include/beagle_mi355.h beagleMi355NodePosteriors) on the HIP engine: bit for bit the
float64 restatement (tests/node_posteriors_reference.py) over the instance's own read-back partials, within the first-order bound of
its np.longdouble twin, within the project's parity tolerance of the same quantities formed from the CPU oracle's partials — and the
same bits whatever the shape of the call.  The restatement itself is pinned on the CPU tier against the enumerated marginal
(tests/test_node_posteriors_host.py)."""
import functools
import os

import numpy as np
import pytest

import beast_mcmc_amd as bm
import helpers
import node_posteriors_reference as pr
from beast_mcmc_amd.nodeposteriors import NodePosteriors
from beast_mcmc_amd.inputs.substmodel import EigenDecomposition
from beast_mcmc_amd.inputs.synth import Workload

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
PARITY_TOL = 1e-10

ALL_STATES = [2, 4, 5, 15, 16, 20, 21, 61, 64, 80]
# every state count at one pattern count and one category count, then the pattern and the category sweeps at 4, 20 and 61 states:
# one pattern, the T32 tile edge (33), the 64-pattern block edge (65), the workgroup edge (257)
SHAPES = [(S, 4, 65) for S in ALL_STATES] + [(S, 4, P) for S in (4, 20, 61) for P in (1, 33, 257)] + \
         [(S, C, 65) for S in (4, 20, 61) for C in (1, 17)]


def entry_bound(S, C):
    """Twice the first-order bound of one posterior: C products, C weightings and C sums per state, S sums, a division — numerator and
    denominator are sums of non-negative products, so the relative errors add and nothing cancels."""
    return 2 * (C * S + C + 5) * EPS


def build(S, C, P, T=None, library=None, seed=None, env=None, **kw):
    """An evaluation with every kind of tip: tip 0 held as partials (an ambiguity code), tip 1 an emission table of three codes
    (folded into its branch matrix on the engine), tip 2 unknown at every third pattern, the others compact states."""
    seed = 1000 + 7 * S + 3 * C + P if seed is None else seed
    T = (9 if S == 2 else 7) if T is None else T              # (two states: nine taxa have enough distinct columns for 65 patterns)
    wl = helpers.random_workload(T, P, S, C, seed=seed, unknown_fraction=0.1)
    wl.tip_states[2][::3] = S + 1
    rng = np.random.default_rng(seed + 1)
    old = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    try:
        g = NodePosteriors(wl, library=library, **kw)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    g.set_tip_partials(0, rng.uniform(0.1, 1.0, size=(P, S)))
    K = min(S, 3)
    table = rng.dirichlet(np.full(S, 0.5), size=K) * 0.9 + 0.1 / S
    codes = rng.integers(0, K, size=P)
    if library is None:
        g.b.setTipEmission(1, codes, table)
    else:
        g.b.setTipPartials(1, table[codes].ravel())
    g.partial_tips.add(1)
    return g


def read_back(g, nodes=None):
    """(pre, post) [R, C, P, S] of the listed nodes from the instance's own getPartials; compact tips expanded from their states."""
    nodes = range(g.N) if nodes is None else nodes
    pre = np.stack([g.b.getPartials(g.pre_offset + int(n), -1).reshape(g.C, g.P, g.S) for n in nodes])
    post = np.stack([pr.expand_states(g.wl.tip_states[int(n)], g.S, g.C) if (n < g.T and int(n) not in g.partial_tips)
                     else g.b.getPartials(g.post_index(int(n)), -1).reshape(g.C, g.P, g.S) for n in nodes])
    return pre, post


def everything(g, nodes=None):
    out = g.posteriors(nodes, full=True, map=True, totals=True, categories=True)
    return out


@functools.lru_cache(maxsize=None)
def evaluated(S, C, P):
    """One device call over every node and what the restatements make of the same partials, computed once per shape."""
    g = build(S, C, P)
    g.prepare()
    dev = everything(g)
    pre, post = read_back(g)
    g.close()
    f64 = pr.posteriors(pre, post, g.wl.cat_weights)[0]
    ld = pr.posteriors(pre, post, g.wl.cat_weights, dtype=np.longdouble)[0]
    for a in (f64, ld, pre, post):
        a.setflags(write=False)
    return g, dev, pre, post, f64, ld


@pytest.mark.parametrize("S,C,P", SHAPES)
def test_bit_for_bit_the_restatement(S, C, P):
    g, dev, pre, post, f64, _ = evaluated(S, C, P)
    assert dev["code"] == 0
    assert dev["posteriors"].shape == (g.N, P, S)
    assert np.array_equal(dev["posteriors"], f64)
    states, probs = pr.map_states(f64)
    assert np.array_equal(dev["map_states"], states)
    assert np.array_equal(dev["map_probabilities"], probs)
    assert np.array_equal(dev["categories"], pr.category_posteriors(pre[0], post[0], g.wl.cat_weights))
    assert np.array_equal(dev["totals"], pr.state_totals_in_device_order(f64, g.wl.weights))
    # an unambiguous compact tip: exactly 1.0 at its state, 0.0 elsewhere
    for tip in range(3, g.T):
        st = np.asarray(g.wl.tip_states[tip])
        known = np.nonzero(st < S)[0]
        want = np.zeros((len(known), S)); want[np.arange(len(known)), st[known]] = 1.0
        assert np.array_equal(dev["posteriors"][tip][known], want), tip
        assert np.array_equal(dev["map_states"][tip][known], st[known])


@pytest.mark.parametrize("S,C,P", SHAPES)
def test_within_the_bound_of_the_longdouble_twin(S, C, P):
    g, dev, pre, post, _, ld = evaluated(S, C, P)
    bound = entry_bound(S, C)
    err = np.abs(dev["posteriors"] - ld)
    ratio = float(np.max(err / np.maximum(bound * ld, np.finfo(float).tiny) * (err > 0)))
    print("S %d C %d P %d: largest error as a fraction of the bound: %.3g" % (S, C, P, ratio))
    assert np.all(err <= bound * ld)
    cats = pr.category_posteriors(pre[0], post[0], g.wl.cat_weights, dtype=np.longdouble)
    assert np.all(np.abs(dev["categories"] - cats) <= bound * cats)
    w = float(np.sum(g.wl.weights))
    tot_bound = 2 * (P + C * S + C + 5) * EPS * w
    assert np.all(np.abs(dev["totals"] - pr.state_totals(ld, g.wl.weights)) <= tot_bound)
    assert np.all(np.abs(dev["totals"].sum(axis=1) - w) <= tot_bound)


@pytest.mark.parametrize("S", [4, 20, 61])
def test_against_the_oracle(S, oracle_lib):
    g, dev, _, _, _, _ = evaluated(S, 4, 65)
    o = build(S, 4, 65, library=oracle_lib)
    o.prepare()
    pre, post = read_back(o)
    o.close()
    want = pr.posteriors(pre, post, o.wl.cat_weights)[0]
    assert np.max(np.abs(dev["posteriors"] - want)) <= PARITY_TOL
    assert np.max(np.abs(dev["categories"] - pr.category_posteriors(pre[0], post[0], o.wl.cat_weights))) <= PARITY_TOL
    assert np.max(np.abs(dev["totals"] - pr.state_totals(want, o.wl.weights, dtype=np.float64))) <= PARITY_TOL * np.sum(o.wl.weights)
    # the host route of the package over the same instance kind says the same
    h = build(S, 4, 65)
    h.prepare()
    host = h.posteriors(full=True, map=True, totals=True, categories=True, route="host")
    h.close()
    assert np.max(np.abs(host["posteriors"] - dev["posteriors"])) <= PARITY_TOL
    assert np.max(np.abs(host["categories"] - dev["categories"])) <= PARITY_TOL
    assert np.max(np.abs(host["totals"] - dev["totals"])) <= PARITY_TOL * np.sum(o.wl.weights)


@pytest.mark.parametrize("S,C", [(4, 4), (20, 4), (61, 1)])
def test_scale_factors_cancel(S, C):
    P, T = 65, 9
    plain, scaled = build(S, C, P, T=T, seed=77 + S), build(S, C, P, T=T, seed=77 + S, rescale=True)
    plain.prepare(); scaled.prepare()
    a, b = everything(plain), everything(scaled)
    root = plain.tree.root
    assert not np.array_equal(plain.b.getPartials(plain.post_index(root), -1), scaled.b.getPartials(scaled.post_index(root), -1))
    plain.close(); scaled.close()
    assert a["code"] == 0 and b["code"] == 0
    bound = entry_bound(S, C)
    err = np.abs(a["posteriors"] - b["posteriors"])
    print("S %d: rescaled against plain, largest error as a fraction of the bound: %.3g"
          % (S, float(np.max(err / np.maximum(bound * a["posteriors"], np.finfo(float).tiny) * (err > 0)))))
    assert np.all(err <= bound * a["posteriors"])
    w = float(np.sum(plain.wl.weights))
    assert np.all(np.abs(a["totals"] - b["totals"]) <= 2 * (P + C * S + C + 5) * EPS * w)


def same_bits(a, b, totals=True):
    for key in ("posteriors", "map_states", "map_probabilities", "categories") + (("totals",) if totals else ()):
        assert np.array_equal(a[key], b[key], equal_nan=True), key


@pytest.mark.parametrize("S", [4, 20, 61])
def test_same_bits_under_different_call_shapes(S):
    C, P = 4, 257
    g = build(S, C, P)
    g.prepare()
    first = everything(g)
    same_bits(first, everything(g))
    launches = g.b.nodePosteriorStats()["launches"]
    old = os.environ.get("BEAGLE_MI355_NODE_POSTERIOR_CHUNK")
    os.environ["BEAGLE_MI355_NODE_POSTERIOR_CHUNK"] = "1"
    try:
        split = everything(g)
    finally:
        if old is None:
            os.environ.pop("BEAGLE_MI355_NODE_POSTERIOR_CHUNK", None)
        else:
            os.environ["BEAGLE_MI355_NODE_POSTERIOR_CHUNK"] = old
    assert g.b.nodePosteriorStats()["launches"] - launches == 2 * g.N + 1          # a row and its totals per launch, the categories once
    same_bits(first, split)
    order = np.random.default_rng(3).permutation(g.N)
    order = np.concatenate([[0], order[order != 0], [int(order[-1])]])             # (node 0 stays first: the categories are the first row's; one node twice)
    shuffled = everything(g, order)
    back = {k: (v if k in ("categories", "code") else v[np.argsort(order[:-1], kind="stable")]) for k, v in shuffled.items()}
    same_bits(first, back)
    assert np.array_equal(shuffled["posteriors"][-1], first["posteriors"][int(order[-1])])
    g.close()
    # three shards of one device: every pattern's bits, the totals to the bound of the yardstick
    all_gpus = len(bm.beagle.engine().resource_list()) - 1
    m = build(S, C, P, env={"BEAGLE_MI355_SHARDS": "3"}, resource_list=(all_gpus,))
    m.prepare()
    sharded = everything(m)
    m.close()
    same_bits(first, sharded, totals=False)
    w = float(np.sum(g.wl.weights))
    assert np.all(np.abs(first["totals"] - sharded["totals"]) <= 2 * (P + C * S + C + 5) * EPS * w)


def test_operands_not_stored_behind_a_held_list():
    """From the second evaluation of a chain on, the 4-state post-order passes leave short subtrees unstored and the pre-order list is
    held back: the call runs the list and materialises what it reads."""
    wl = helpers.random_workload(9, 257, 4, 4, seed=41)
    g = NodePosteriors(wl)
    old = os.environ.get("BEAGLE_MI355_NO_VIRTUAL")
    os.environ["BEAGLE_MI355_NO_VIRTUAL"] = "1"
    try:
        twin = NodePosteriors(wl)
    finally:
        if old is None:
            os.environ.pop("BEAGLE_MI355_NO_VIRTUAL", None)
        else:
            os.environ["BEAGLE_MI355_NO_VIRTUAL"] = old
    out = []
    for ev in (g, twin):
        for _ in range(3):
            ev.prepare()
        late = ev.b.gradientStats()["late"]
        out.append(everything(ev))
        held = ev.b.gradientStats()["late"] - late
        stats = ev.b.nodePosteriorStats()
        print("materialised", stats["materialised"], "held lists run by the call", held)
        assert stats["calls"] == 1 and stats["rows"] == ev.N
        if ev is g:
            assert held == 1
            assert stats["materialised"] > 0
        else:
            assert stats["materialised"] == 0
    same_bits(out[0], out[1])
    pre, post = read_back(g)
    assert np.array_equal(out[0]["posteriors"], pr.posteriors(pre, post, wl.cat_weights)[0])
    g.close(); twin.close()


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
        return 0
    except bm.beagle.BeagleException as e:                 # the root sum of an impossible pattern; the post-order partials are there
        assert e.code == -8
        g.b.setPartials(g.pre_offset + g.tree.root, g._root_pre)
        g.b.updatePrePartials(g._pre_ops, len(g._pre_ops) // 7, -1)
        return -8


def test_a_zero_likelihood_pattern():
    P, j = 70, 66
    bad, good = NodePosteriors(reducible_workload(P, j)), NodePosteriors(reducible_workload(P, None))
    prepare_through_a_zero(bad)
    assert prepare_through_a_zero(good) == 0
    a, b = everything(bad), everything(good)
    bad.close(); good.close()
    assert a["code"] == -8 and b["code"] == 0
    assert np.isnan(a["posteriors"][:, j]).all() and np.isnan(a["map_probabilities"][:, j]).all() and np.isnan(a["categories"][j]).all()
    assert np.all(a["map_states"][:, j] == 0)
    assert np.isnan(a["totals"]).all() and np.isfinite(b["totals"]).all()
    others = np.arange(P) != j
    assert np.array_equal(a["posteriors"][:, others], b["posteriors"][:, others])
    assert np.array_equal(a["map_states"][:, others], b["map_states"][:, others])
    assert np.array_equal(a["map_probabilities"][:, others], b["map_probabilities"][:, others])
    assert np.array_equal(a["categories"][others], b["categories"][others])
    assert np.isfinite(b["posteriors"]).all()


def test_refusals():
    g = build(4, 2, 65, double_buffer=True)
    g.prepare()
    rows = g.rows()
    watched = sorted(set(int(x) for x in rows.ravel()))                  # every listed buffer

    def snapshot():
        return [g.b.getPartials(x, -1).copy() for x in watched if x >= g.T or x in g.partial_tips]

    everything(g)                                                        # (the folded tip has its partials from here on)
    before = snapshot()

    def code(r, **kw):
        with pytest.raises(bm.beagle.BeagleException) as e:
            g.b.nodePosteriors(r, **kw)
        return e.value.code

    for column in range(2):
        for value in (10 ** 6, -1):
            bad = rows.copy(); bad[3, column] = value
            assert code(bad) == -5, (column, value)
    bad = rows.copy(); bad[4, 1] = 3                                     # pre(i) holds compact tip states
    assert code(bad) == -5
    unwritten = g.T + (1 - g._set) * g._partial_set                      # the first internal buffer of the set no evaluation has used
    for column in range(2):
        bad = rows.copy(); bad[g.T, column] = unwritten
        assert code(bad) == -5, column
    assert code(rows, flags=1) == -5
    assert code(rows, full=False) == -5                                  # every output NULL
    assert code(rows[:0]) == -5                                          # nodeCount 0
    assert code(rows, categoryWeightsIndex=7) == -5
    after = snapshot()
    assert len(after) == len(before) and all(np.array_equal(x, y) for x, y in zip(before, after))
    out, rc = g.b.nodePosteriors(rows)                                   # and the instance still answers
    assert rc == 0 and np.isfinite(out["posteriors"]).all()
    # a partitioned instance, a BASTA instance: not built
    g.b.setPatternPartitions(2, (np.arange(65) // 33).astype(np.int32))
    assert code(rows) == -7
    again = snapshot()
    assert len(again) == len(before) and all(np.array_equal(x, y) for x, y in zip(before, again))
    g.close()
    b = bm.beagle.Beagle(0, 8, 0, 3, 1, 2, 4, 1, 1)
    b.allocateCoalescentBuffers(5, 4, 12, 1)
    with pytest.raises(bm.beagle.BeagleException) as e:
        b.nodePosteriors([[0, 1]])
    assert e.value.code == -7
    b.finalize()
