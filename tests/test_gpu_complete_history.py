"""Complete histories on the GPU (include/beagle_mi355.h beagleMi355SimulateCompleteHistories, beast-mcmc_amd/completehistory.py)
against the host restatement (tests/complete_history_reference.py): states, categories, event counts, the events' states and every
count register's values must be IDENTICAL on every history — tests/test_complete_history_host.py shows on the CPU that no history of
any case used here has an event time within 1e-12 relative of its branch's end, so none is excluded.  Rewards and event heights agree
within the bound below.

The bound, with e = 2^-53 (half an ulp, relative).  1 - u is exact on both sides.  The device's log and numpy's are each within one
ulp (2 e relative) of the true logarithm, so they differ by at most 4 e relative; the division that follows is rounded once on each
side: a waiting time differs by at most 6 e of itself.  A time t_m is m waiting times added in order; each addition rounds once on
each side (2 e of the partial sum, itself below tau), so |dt_m| <= (6 + 2 m) e tau, and the sojourn t_(i+1) - t_i — which is what a
reward register multiplies — differs by at most 6 e w_(i+1) + 2 e tau plus its own subtraction's rounding.  Over a history of n jumps:
the n sojourns contribute (6 + 2 n) e tau max|R|, the final term R (tau - t_n) another (6 + 2 n) e tau max|R| through dt_n, the
subtractions and products 4 e tau max|R| (one rounding each, each side, the sojourns summing to tau), the n + 1 additions of the
accumulation 2 (n + 1) e tau max|R|: (6 n + 18) e tau max|R| in all, which is below 8 (n + 2) e tau max|R| for every n >= 1 (n = 0:
one product of identical operands, no difference).  Hence c = 8 (complete_history_cases.BOUND_C) in
    |device - restatement| <= c (n + 2) 2^-53 tau max|R_kk|.
Event heights, h_parent + (t / tau) (h_child - h_parent) for the m-th jump: t / tau differs by (6 + 2 m) e + 2 e, the product adds
2 e: below c (m + 2) e |h_parent - h_child|, the same form.  (The final addition rounds once more on each side, relative to the height
itself; the form the bound is stated in does not carry that term, and the assertion below does not add it.)
The largest observed fractions of the bounds are printed by test_equals_the_restatement and recorded in DESIGN.md 4.11.
"""
import ctypes as C
import os

import numpy as np
import pytest

import beast_mcmc_amd as bm
import complete_history_cases as cc
import complete_history_reference as hr
import helpers
import simulate_cases as sc
from beast_mcmc_amd.completehistory import CompleteHistorySimulator
from beast_mcmc_amd.treelikelihood import BeagleTreeLikelihood

pytestmark = pytest.mark.gpu


def instance_for(c, resource_list=(1,)):
    """An instance on which nothing but the model setters is ever called."""
    b = bm.beagle.Beagle(c.tree.tip_count, c.tree.node_count, c.tree.tip_count, c.S, 16, 1, 2, c.C, 0, resourceList=resource_list)
    b.setStateFrequencies(0, c.freqs)
    b.setCategoryRates(c.cat_rates)
    b.setCategoryWeights(0, c.cat_weights)
    return b


def call(b, c, seed=None, sites=None, **kw):
    kw.setdefault("history", True)
    return b.simulateCompleteHistories(c.rows, c.sites if sites is None else sites, c.lengths, c.Q, c.registers, c.flags,
                                       c.seed if seed is None else seed, nodeHeights=c.heights, **kw)


def same_bytes(a, b):
    assert a.keys() == b.keys()
    for key in a:
        assert np.array_equal(np.asarray(a[key]), np.asarray(b[key])), key


def check_equal(out, res, c):
    """One call against the restatement -> the largest fractions of the reward and height bounds."""
    for r in range(len(c.rows)):
        assert np.array_equal(out["states"][c.rows[r, 0]], res["states"][r]), r
    assert np.array_equal(out["categories"], res["categories"])
    assert np.array_equal(out["event_counts"], res["counts"])
    assert out["event_total"] == len(res["event_site"])
    assert np.array_equal(out["event_states"], res["event_states"])
    counts = (c.flags & hr.REWARDS) == 0
    assert np.array_equal(out["values"][counts], res["values"][counts])
    bound = cc.reward_bound(res, c)
    diff = np.abs(out["values"] - res["values"])
    assert np.all(diff <= bound)
    hb = cc.height_bound(res, c)
    hd = np.abs(out["event_heights"] - res["event_heights"])
    assert np.all(hd <= hb)
    # the totals are the device's own values in the fixed orders, bit for bit
    assert np.array_equal(out["row_totals"], hr.row_totals(out["values"]))
    st = np.zeros_like(out["site_totals"])
    for r in range(1, len(c.rows)):
        st = st + out["values"][:, r]
    assert np.array_equal(out["site_totals"], st)
    assert np.array_equal(out["site_totals"][counts], res["site_totals"][counts])
    assert not out["values"][:, 0].any()
    with np.errstate(invalid="ignore", divide="ignore"):
        fr = float(np.nanmax(np.where(bound > 0, diff / bound, 0.0))) if bound.size else 0.0
        fh = float(np.nanmax(np.where(hb > 0, hd / hb, 0.0))) if hb.size else 0.0
    return fr, fh


@pytest.mark.parametrize("name", sorted(cc.CASES))
def test_equals_the_restatement(name):
    c, res = cc.build(name), cc.restated(name)
    b = instance_for(c)
    out = call(b, c)
    fr, fh = check_equal(out, res, c)
    print("%s: %d histories, %d events, rewards at most %.3f of their bound, heights %.3f" %
          (name, res["counts"].size, out["event_total"], fr, fh))
    # asking for fewer outputs does not change the others
    few = call(b, c, values=False, site_totals=False, history=False)
    assert np.array_equal(few["states"], out["states"]) and np.array_equal(few["row_totals"], out["row_totals"])
    b.finalize()


def test_per_branch_generators():
    c, res = cc.build_generators(), cc.restated_generators()
    q = c.rows[1:, 1]
    assert (np.diff(q) == 0).any() and (np.diff(q) != 0).any() and set(q) == {0, 1, 2}
    b = instance_for(c)
    check_equal(call(b, c), res, c)
    # every row under generator 1 of three = the one-generator call with that generator
    one = cc.build("s4")
    d = type(c)(**vars(c)); d.rows = c.rows.copy(); d.rows[1:, 1] = 1
    e = type(c)(**vars(one)); e.Q = c.Q[1:2]
    same_bytes(call(b, d, seed=7), call(b, e, seed=7))
    b.finalize()


def test_determinism(monkeypatch):
    c = cc.build("s4")
    b = instance_for(c)
    s1, s2 = cc.OTHER_SEEDS
    whole = call(b, c, seed=s1)
    same_bytes(whole, call(b, c, seed=s1))
    other = call(b, c, seed=s2)
    assert not np.array_equal(whole["states"], other["states"]) and not np.array_equal(whole["values"], other["values"])
    rng = np.random.default_rng(1)
    root, cats = rng.integers(0, c.S, size=c.sites).astype(np.uint8), rng.integers(0, c.C, size=c.sites).astype(np.int32)
    given = call(b, c, seed=s1, root_states=root, rate_categories=cats)
    assert np.array_equal(given["states"][c.rows[0, 0]], root) and np.array_equal(given["categories"], cats)
    for chunk in ("64", "257"):                             # (rounded up to whole blocks of 256: four launches, two launches)
        monkeypatch.setenv("BEAGLE_MI355_HIST_CHUNK_SITES", chunk)
        same_bytes(whole, call(b, c, seed=s1))
        same_bytes(given, call(b, c, seed=s1, root_states=root, rate_categories=cats))
    monkeypatch.delenv("BEAGLE_MI355_HIST_CHUNK_SITES")
    b.finalize()


def test_the_class_returns_the_same_bytes_by_tree_node():
    c, res = cc.build("s4"), cc.restated("s4")
    sim = CompleteHistorySimulator.from_model(c.tree, c.cat_rates, c.cat_weights, c.freqs, c.Q[0])
    for k in range(c.K):
        if c.flags[k] & hr.REWARDS:
            sim.add_register("r%d" % k, np.diag(c.registers[k]), "rewards")
        else:
            sim.add_register("c%d" % k, c.registers[k], "counts")
    rows, order = sim.node_list()
    assert np.array_equal(rows, c.rows) and np.array_equal(order, c.order)
    got = sim.simulate(c.sites, c.seed, history=True)
    t = c.tree.tip_count
    by_node = np.empty(len(order), dtype=np.int64); by_node[order] = np.arange(len(order))
    assert np.array_equal(np.vstack([got["alignment"], got["ancestral"]]), res["states"][by_node])
    assert got["alignment"].shape[0] == t and np.array_equal(got["event_counts"], res["counts"][by_node])
    assert np.array_equal(got["events"]["node"], order[res["event_row"]]) and np.array_equal(got["events"]["site"], res["event_site"])
    assert np.array_equal(got["values"][0], res["values"][0][by_node])
    assert np.array_equal(got["sum_across_sites"][0], got["values"][0].sum(axis=1))          # (integers: any order)
    tips = sim.simulate(c.sites, c.seed, ancestral=False, per_site=False)
    assert tips["ancestral"] is None and np.array_equal(tips["alignment"], got["alignment"])
    assert np.array_equal(tips["sum_across_sites"], got["sum_across_sites"])
    sim.close()


@pytest.fixture
def shards(request):
    n = getattr(request, "param", 0)
    old = os.environ.get("BEAGLE_MI355_SHARDS")
    if n:
        os.environ["BEAGLE_MI355_SHARDS"] = str(n)
    yield n
    if old is None:
        os.environ.pop("BEAGLE_MI355_SHARDS", None)
    else:
        os.environ["BEAGLE_MI355_SHARDS"] = old


@pytest.mark.parametrize("shards", [0, 3], indirect=True)
def test_sharded_handle_simulates_what_one_instance_simulates(shards):
    g = len(bm.beagle.engine().resource_list()) - 2
    c = cc.build("s4")
    n, seed = cc.SHARDED_SITES, cc.SHARDED_SEED
    single, multi = instance_for(c), instance_for(c, resource_list=(g + 1,))
    rng = np.random.default_rng(2)
    root, cats = rng.integers(0, 4, size=n).astype(np.uint8), rng.integers(0, 4, size=n).astype(np.int32)
    for kw in ({}, {"root_states": root, "rate_categories": cats}):
        a, m = call(single, c, seed=seed, sites=n, **kw), call(multi, c, seed=seed, sites=n, **kw)
        for key in a:
            if key != "row_totals":
                assert np.array_equal(np.asarray(a[key]), np.asarray(m[key])), key
        counts = (c.flags & hr.REWARDS) == 0
        assert np.array_equal(a["row_totals"][counts], m["row_totals"][counts])
        # the shards' sums — each in the fixed order, its blocks counted from its first site — added in shard order
        parts = max(shards, 1) if shards else None
        if parts:
            want = np.zeros_like(a["row_totals"])
            for k in range(parts):
                want = want + hr.row_totals(a["values"][:, :, n * k // parts:n * (k + 1) // parts])
            assert np.array_equal(m["row_totals"], want)
        else:
            assert np.allclose(a["row_totals"], m["row_totals"], rtol=1e-12, atol=0.0)
    single.finalize(); multi.finalize()


def test_event_capacity():
    c, res = cc.build("s4"), cc.restate(cc.build("s4"), seed=cc.OTHER_SEEDS[0])
    total = len(res["event_site"])
    b = instance_for(c)
    short = call(b, c, seed=cc.OTHER_SEEDS[0], event_capacity=total - 1, retry=False)
    assert short["rc"] == -5 and short["event_total"] == total
    full = call(b, c, seed=cc.OTHER_SEEDS[0], event_capacity=total, retry=False)
    assert "rc" not in full and full["event_total"] == total
    for key in ("states", "categories", "values", "row_totals", "site_totals", "event_counts"):
        assert np.array_equal(short[key], full[key]), key
    check_equal(full, res, c)
    same_bytes(full, call(b, c, seed=cc.OTHER_SEEDS[0], event_capacity=3))         # the binding's second call with the exact size
    b.finalize()


_PROTO = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
          C.c_void_p, C.c_int, C.c_ulonglong, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
          C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p, C.c_void_p]


def raw(b, c, **kw):
    """The C call itself with every argument replaceable -> (return code, outputs)."""
    n, sites = len(c.rows), kw.get("siteCount", c.sites)
    m = max(1, sites)
    a = dict(nodes=np.ascontiguousarray(c.rows, dtype=np.int32), nodeCount=n, siteCount=sites, lengths=np.ascontiguousarray(c.lengths),
             heights=np.ascontiguousarray(c.heights), Q=np.ascontiguousarray(c.Q), qCount=len(c.Q), rates=0, w=0, f=0,
             registers=np.ascontiguousarray(c.registers), regFlags=np.ascontiguousarray(c.flags, dtype=np.int32), K=c.K, seed=c.seed,
             flags=0, root=None, cats=None, states=np.full((int(c.rows[:, 0].max()) + 1, m), 255, dtype=np.uint8),
             outCats=np.full(m, -1, dtype=np.int32), values=np.full((c.K, n, m), np.nan), rowTotals=np.full((c.K, n), np.nan),
             siteTotals=np.full((c.K, m), np.nan), counts=np.full((n, m), -1, dtype=np.int32), capacity=1 << 20,
             evHeights=np.zeros(1 << 20), evStates=np.zeros((1 << 20, 2), dtype=np.uint8), total=C.c_longlong(-1))
    a.update(kw)

    def p(x):
        return None if x is None else (C.addressof(x) if isinstance(x, C.c_longlong) else x.ctypes.data)

    fn = b._ext("beagleMi355SimulateCompleteHistories", _PROTO)
    rc = fn(b.instance, p(a["nodes"]), a["nodeCount"], a["siteCount"], p(a["lengths"]), p(a["heights"]), p(a["Q"]), a["qCount"],
            a["rates"], a["w"], a["f"], p(a["registers"]), p(a["regFlags"]), a["K"], a["seed"], a["flags"], p(a["root"]), p(a["cats"]),
            p(a["states"]), p(a["outCats"]), p(a["values"]), p(a["rowTotals"]), p(a["siteTotals"]), p(a["counts"]), a["capacity"],
            p(a["evHeights"]), p(a["evStates"]), p(a["total"]))
    return rc, a


def test_the_jump_cap():
    """One site, two states, a branch of 1e9 expected jumps: given up at 100 000, everything written, -8."""
    c = type(cc.build("s2"))(**vars(cc.build("s2")))
    c.rows = np.array([[0, 0, -1], [1, 0, 0]], dtype=np.int32)
    c.lengths, c.heights = np.array([0.0, 1e9]), np.array([1e9, 0.0])
    c.Q = np.array([[[-1.0, 1.0], [1.0, -1.0]]])
    c.registers, c.flags, c.K, c.sites = np.stack([np.ones((2, 2)), np.eye(2)]), np.array([0, 1], dtype=np.int32), 2, 1
    b = instance_for(cc.build("s2"))
    rc, a = raw(b, c)
    assert rc == -8
    assert a["total"].value == 100000 and a["counts"][1, 0] == 100000 and a["values"][0, 1, 0] == 100000.0
    assert a["states"][1, 0] == a["states"][0, 0] < 2                    # an even number of jumps between two states
    assert 0.0 < a["values"][1, 1, 0] < 1e9 and a["rowTotals"][0, 1] == 100000.0 and a["siteTotals"][0, 0] == 100000.0
    assert np.all(np.diff(a["evHeights"][:100000]) < 0) and np.array_equal(a["evStates"][:4, 0], a["evStates"][:4, 1] ^ 1)
    with pytest.raises(bm.beagle.BeagleException) as e:
        b.simulateCompleteHistories(c.rows, 1, c.lengths, c.Q, c.registers, c.flags, c.seed, history=False)
    assert e.value.code == -8
    b.finalize()


def test_the_instance_is_left_as_it_was():
    wl = helpers.random_workload(20, 500, 4, 4, seed=55)
    tl = BeagleTreeLikelihood(wl)
    before, site_before = tl.getLogLikelihood(), tl.getSiteLogLikelihoods().copy()
    sim = CompleteHistorySimulator(tl)
    sim.add_register("all", np.ones((4, 4)))
    sim.add_register("time", np.ones(4), "rewards")
    got = sim.simulate(900, 17, history=True)
    assert got["alignment"].shape == (20, 900) and got["events"]["site"].size == got["event_counts"].sum() > 0
    # the time spent on a branch is its length x the site's rate, whatever happened on it
    order = sim.preorder()
    tau = np.asarray(wl.cat_rates)[got["categories"]][None, :] * np.array([sim.branch_lengths(order)[order.index(n)] for n in range(39)])[:, None]
    assert np.allclose(got["values"][1], tau, rtol=1e-12, atol=0.0)
    assert tl.getLogLikelihood() == before and np.array_equal(tl.getSiteLogLikelihoods(), site_before)
    tl.makeDirty()
    assert tl.getLogLikelihood() == before and np.array_equal(tl.getSiteLogLikelihoods(), site_before)      # bitwise
    # pattern partitions change nothing
    sim.beagle.setPatternPartitions(2, (np.arange(wl.pattern_count) >= wl.pattern_count // 2).astype(np.int32))
    again = sim.simulate(900, 17, history=True)
    assert np.array_equal(again["alignment"], got["alignment"]) and np.array_equal(again["values"], got["values"])
    tl.close()


def test_distribution_on_the_device():
    """The tree, seed and site count of tests/test_complete_history_host.py against the engine's own site likelihoods."""
    tl = sc.tree_likelihood()
    assert np.isfinite(tl.getLogLikelihood())
    prob = np.exp(tl.getSiteLogLikelihoods())
    sim = CompleteHistorySimulator(tl)
    sim.add_register("all", np.ones((4, 4)))
    got = sim.simulate(sc.N_SITES, sc.SEED, ancestral=False, per_site=False)
    sc.check_distribution(got["alignment"], got["categories"], prob)
    tl.close()


def test_error_codes():
    c = cc.build("s4")
    b = instance_for(c)
    assert raw(b, c)[0] == 0
    for key in ("nodes", "lengths", "Q", "registers"):
        assert raw(b, c, **{key: None})[0] == -5, key
    assert raw(b, c, regFlags=None)[0] == 0 and raw(b, c, heights=None, evHeights=None)[0] == 0
    for key in ("nodeCount", "siteCount", "qCount"):
        assert raw(b, c, **{key: 0})[0] == -5 and raw(b, c, **{key: -2})[0] == -5, key
    for key in ("rates", "w", "f"):
        assert raw(b, c, **{key: 7})[0] == -5 and raw(b, c, **{key: -1})[0] == -5, key
    rows = np.ascontiguousarray(c.rows, dtype=np.int32)
    for r, col, v in ((4, 1, 1), (4, 1, -1), (3, 2, 5), (2, 2, 2), (5, 2, -1), (6, 0, int(rows[2, 0])), (6, 0, -2)):
        bad = rows.copy(); bad[r, col] = v
        assert raw(b, c, nodes=bad)[0] == -5, (r, col, v)      # qIndex, parent after / equal / missing, outRow twice / below -1
    for v in (np.nan, np.inf):
        Q = c.Q.copy(); Q[0, 1, 2] = v
        assert raw(b, c, Q=Q)[0] == -5
        ln = c.lengths.copy(); ln[3] = v
        assert raw(b, c, lengths=ln)[0] == -5
    ln = c.lengths.copy(); ln[3] = -1e-9
    assert raw(b, c, lengths=ln)[0] == -5
    ln[3] = 0.0; ln[0] = -1.0
    assert raw(b, c, lengths=ln)[0] == 0                                  # row 0 is ignored
    fl = np.ascontiguousarray(c.flags, dtype=np.int32).copy(); fl[0] = 2
    assert raw(b, c, regFlags=fl)[0] == -5                                # scale-by-time is not accepted here
    fl[0] = 4
    assert raw(b, c, regFlags=fl)[0] == -5
    assert raw(b, c, K=0)[0] == -5 and raw(b, c, K=9)[0] == -5
    assert raw(b, c, flags=1)[0] == -5
    root = np.zeros(c.sites, dtype=np.uint8); root[-1] = 4
    assert raw(b, c, root=root)[0] == -5
    cats = np.zeros(c.sites, dtype=np.int32); cats[-1] = 4
    assert raw(b, c, cats=cats)[0] == -5
    cats[-1] = -1
    assert raw(b, c, cats=cats)[0] == -5
    assert raw(b, c, heights=None)[0] == -5                               # event heights asked for without node heights
    assert raw(b, c, capacity=-1)[0] == -5
    none = dict(states=None, outCats=None, values=None, rowTotals=None, siteTotals=None, counts=None, evHeights=None, evStates=None,
                total=None)
    assert raw(b, c, **none)[0] == -5
    only = dict(none); only["rowTotals"] = np.full((c.K, len(c.rows)), np.nan)
    rc, a = raw(b, c, **only)
    assert rc == 0 and np.array_equal(a["rowTotals"], raw(b, c)[1]["rowTotals"])
    b.finalize()
    # -7: more than 64 states, a BASTA instance
    big = bm.beagle.Beagle(2, 6, 2, 65, 8, 1, 4, 1, 0)
    d = type(c)(**vars(cc.build("s2")))
    d.Q, d.registers, d.S = np.zeros((1, 65, 65)), np.zeros((1, 65, 65)), 65
    assert raw(big, d)[0] == -7
    big.finalize()
    basta = bm.beagle.Beagle(0, 8, 0, 2, 1, 2, 4, 1, 1)
    basta.allocateCoalescentBuffers(5, 4, 12, 1)
    assert raw(basta, cc.build("s2"))[0] == -7
    basta.finalize()
