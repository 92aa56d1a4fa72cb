"""Uniformized Markov jumps on the GPU (include/beagle_mi355.h beagleMi355SampleMarkovJumpsUniformized, markovjumps.py) against the
host restatement (tests/uniformized_reference.py) over what the engine reads back.  The draw must be the ancestral sampler's byte for
byte; the number of subordinated changes, the event counts and the events' states exactly equal except at (row, pattern) pairs the
restatement flags as within 1e-12 relative of a Poisson-draw boundary (the device's exp() may round differently); values and event
heights to 1e-12 relative (log() in the jump times)."""
import json
import os

import numpy as np
import pytest

import beast_mcmc_amd as bm
import helpers
import markov_jumps_reference as mr
import uniformized_reference as ur
from beast_mcmc_amd.inputs import substmodel, synth, trees
from beast_mcmc_amd.markovjumps import MarkovJumpsSampler
from beast_mcmc_amd.treelikelihood import RESCALE_ALWAYS, RESCALE_DYNAMIC, BeagleTreeLikelihood

pytestmark = pytest.mark.gpu


def registers(sampler, S, seed):
    """all jumps, "upper" (i < j), "lower" (i > j), one pair scaled by time, a reward scaled by time"""
    rng = np.random.default_rng(seed)
    sampler.add_register("all", np.ones((S, S)))
    sampler.add_register("upper", np.triu(np.ones((S, S)), 1))
    sampler.add_register("lower", np.tril(np.ones((S, S)), -1))
    one = np.zeros((S, S)); one[0, S - 1] = 1.0
    sampler.add_register("from_to", one, scale_by_time=True)
    sampler.add_register("reward", rng.uniform(0.0, 2.0, S), kind="rewards", scale_by_time=True)
    return sampler


def make(wl, branch_rate_seed=None, **kw):
    tl = BeagleTreeLikelihood(wl, **kw)
    if branch_rate_seed is not None:
        tl.set_branch_rates(np.random.default_rng(branch_rate_seed).uniform(0.5, 1.5, wl.tree.node_count))
    tl.getLogLikelihood()
    return tl


def raw_call(s, seed, simulants=1, history=False, Q=None, **kw):
    rows, order = s.ancestral.node_list()
    times, rates = s.branch_times(order)
    heights = s.node_heights(order)
    Q = s.infinitesimal_matrix() if Q is None else Q
    return s.beagle.sampleMarkovJumpsUniformized(rows, times, rates, heights, Q, 0, 0, 0, np.stack(s.registers), s.flags(), seed,
                                                 simulants=simulants, history=history, **kw)


def matrices(tl, s):
    rows, _ = s.ancestral.node_list()
    S, C = tl.state_count, tl.category_count
    mats = np.zeros((len(rows), C, S, S))
    cache = {}
    for r in range(1, len(rows)):
        m = int(rows[r, 1])
        if m not in cache:
            cache[m] = s.beagle.getTransitionMatrix(m).reshape(C, S, S)
        mats[r] = cache[m]
    return mats


def restated(tl, s, states, cats, seed, simulants, Q=None, patterns=None, pattern_count=None):
    rows, order = s.ancestral.node_list()
    times, rates = s.branch_times(order)
    Q = s.infinitesimal_matrix() if Q is None else Q
    return ur.restate(rows[:, 2], times, rates, s.node_heights(order), states, cats, tl.cat_rates, matrices(tl, s), Q, s.registers,
                      s.flags(), simulants, seed, pattern_count=pattern_count, patterns=patterns)


def close(a, b, ok=None):
    err = np.abs(a - b)
    bad = err > 1e-12 * np.maximum(np.abs(b), 1e-3 * max(np.abs(b).max(), 1e-300))
    if ok is not None:
        bad &= ok
    assert not bad.any(), (np.argwhere(bad)[:5], a[bad][:5], b[bad][:5])


def event_keys(counts):
    """(row, pattern) of every event of a device list, from its counts [n][P] (pattern, row, time order)"""
    n, P = counts.shape
    rows = np.repeat(np.tile(np.arange(n), P), counts.T.ravel())
    pats = np.repeat(np.arange(P), counts.sum(axis=0))
    return rows, pats


def check(tl, s, seed, simulants, history, Q=None):
    res = raw_call(s, seed, simulants, history, Q=Q, states=True, jumps=True)
    rows, _ = s.ancestral.node_list()
    st, ca = s.beagle.sampleAncestralStates(rows, 0, 0, seed)
    assert np.array_equal(res["states"], st) and np.array_equal(res["categories"], ca)
    ref = restated(tl, s, st, ca, seed, simulants, Q=Q)
    near = ref["near"]
    assert near.sum() <= 1e-4 * near.size + 0.5 * near.any()
    ok = ~near[None]
    close(res["jumps"], ref["values"], ok)
    if not near.any():
        close(res["pattern_totals"], ref["pattern_totals"])
        close(res["row_totals"], ref["row_totals"])
        assert res["fallbacks"] == ref["fallbacks"]
    if history:
        assert np.array_equal(res["event_counts"][~near], ref["event_counts"][~near])
        dr, dp = event_keys(res["event_counts"])
        keep_d = ~near[dr, dp]
        keep_r = ~near[ref["event_rows"], ref["event_patterns"]]
        assert np.array_equal(res["event_states"][keep_d], ref["event_states"][keep_r])
        close(res["event_heights"][keep_d], ref["event_heights"][keep_r])
        assert res["event_total"] == res["event_counts"].sum()
        assert np.array_equal(res["jumps"][0], res["event_counts"].astype(float))          # all jumps = the real changes
    assert np.array_equal(res["jumps"][0], res["jumps"][1] + res["jumps"][2])                 # one history per simulant
    again = raw_call(s, seed, simulants, history, Q=Q, states=True, jumps=True)
    for key in res:
        assert np.array_equal(res[key], again[key]), key                                     # deterministic
    return res, ref


@pytest.mark.parametrize("S,C,T,P,rescale,simulants", [
    (4, 4, 9, 300, False, 1),
    (4, 3, 25, 257, True, 4),
    (4, 1, 12, 500, False, 1),
    (20, 2, 8, 100, False, 1),
    (61, 1, 6, 70, False, 4),
    (7, 2, 6, 50, True, 1),
])
def test_histories_equal_the_restatement(S, C, T, P, rescale, simulants):
    wl = helpers.random_workload(T, P, S, C, seed=500 + S + T)
    tl = make(wl, branch_rate_seed=S, rescaling=RESCALE_ALWAYS if rescale else RESCALE_DYNAMIC, delay_rescaling=not rescale)
    s = registers(MarkovJumpsSampler(tl), S, seed=S)
    res, ref = check(tl, s, 77 + S, simulants, simulants == 1)
    assert np.all(res["jumps"][:, 0] == 0.0) and res["jumps"][0].sum() > 0.0
    if simulants == 1:
        other = raw_call(s, 78 + S, history=True)
        assert not np.array_equal(other["event_heights"][:50], res["event_heights"][:50])    # another seed, other events
    tl.close()


def test_unknown_compact_tips_and_tips_with_partials():
    import ctypes as C
    wl = helpers.random_workload(30, 400, 4, 4, seed=31, unknown_fraction=0.2)
    tl = BeagleTreeLikelihood(wl)
    rng = np.random.default_rng(4)
    for t in (0, 3, 11):
        part = rng.uniform(0.0, 1.0, size=(wl.pattern_count, 4))
        part[rng.random(wl.pattern_count) < 0.5] = 1.0
        part = np.ascontiguousarray(part)
        assert tl.h.btlSetTipPartials(tl.ptr, t, part.ctypes.data_as(C.POINTER(C.c_double))) == 0
    tl.getLogLikelihood()
    s = registers(MarkovJumpsSampler(tl), 4, seed=9)
    check(tl, s, 99, 1, True)
    tl.close()


def test_zero_rate_category():
    wl = helpers.random_workload(10, 400, 4, 3, seed=41)
    tl = BeagleTreeLikelihood(wl)
    tl.set_site_model([0.0, 1.2, 1.8], [0.3, 0.4, 0.3])           # p-inv: category 0 has rate 0
    tl.getLogLikelihood()
    s = registers(MarkovJumpsSampler(tl), 4, seed=3)
    res, _ = check(tl, s, 5, 1, True)
    inv = res["categories"] == 0
    assert inv.any() and (~inv).any()
    rows, order = s.ancestral.node_list()
    times, _ = s.branch_times(order)
    assert np.all(res["jumps"][:4][:, :, inv] == 0.0) and np.all(res["event_counts"][:, inv] == 0)
    same = res["states"][rows[1:, 2]][:, inv] == res["states"][1:][:, inv]
    assert np.array_equal(res["jumps"][4][1:, inv], np.where(same, times[1:, None], 0.0))
    tl.close()


def test_eigen_complex_instance():
    from test_oracle_golden import _cyclic_model
    S = 4
    qn, pi, eig = _cyclic_model(S, 7)
    rng = np.random.default_rng(8)
    T, P = 12, 300
    tree = trees.coalescent_tree(T, rng, root_height=0.7)
    tips = rng.integers(0, S, size=(T, P)).astype(np.int32)
    wl = synth.Workload("complex", tree, eig, pi, [0.4, 1.0, 1.6], [0.3, 0.4, 0.3], tips, np.ones(P), S)
    tl = make(wl, requirement_flags=bm.beagle.FLAG_EIGEN_COMPLEX)
    s = registers(MarkovJumpsSampler(tl), S, seed=2)
    check(tl, s, 12, 1, True, Q=qn)
    with pytest.raises(bm.beagle.BeagleException) as e:
        s.sample(12)                                                  # the integrated call needs a real eigen system
    assert e.value.code == -7
    tl.close()


def test_same_states_as_the_integrated_call_and_means_agree():
    wl = helpers.random_workload(20, 2000, 4, 4, seed=61)
    tl = make(wl, branch_rate_seed=3)
    s = registers(MarkovJumpsSampler(tl), 4, seed=5)
    a = s.sample(404, states=True, per_site=True)
    b = s.sample(404, states=True, per_site=True, uniformization=True, simulants=64)
    assert np.array_equal(a["states"], b["states"]) and np.array_equal(a["categories"], b["categories"])
    d = b["pattern"] - a["pattern"]                                   # [K][P]: independent across patterns
    se = d.std(axis=1) * np.sqrt(d.shape[1])
    assert np.all(np.abs(d.sum(axis=1)) <= 5 * se), (d.sum(axis=1), se)
    tl.close()


def test_two_tip_expectations():
    """MarkovJumpsTest's two tips (tests/golden/markov_jumps.json): 10 000 identical patterns, one sampled history each; each
    register's mean within 5 standard errors of the exact enumeration."""
    g = json.load(open(os.path.join(helpers.ROOT, "tests", "golden", "markov_jumps.json")))["two_tips"]
    pi = np.asarray(g["frequencies_acgt"])
    eig = substmodel.hky(g["kappa"], pi)
    tree = trees.Tree([-1, -1, 0], [-1, -1, 1], [0.0, 0.0, 1.0], 2)
    N = 10000
    wl = synth.Workload("two-tips", tree, eig, pi, [g["mu"]], [1.0], np.zeros((2, N), dtype=np.int32), np.ones(N), 4)
    tl = make(wl)
    s = MarkovJumpsSampler(tl)
    for values, kind, sc in zip(g["registers"], g["kinds"], g["scale_by_time"]):
        s.add_register("r", np.reshape(values, (4, 4)) if kind == "counts" else values, kind=kind, scale_by_time=sc)
    out = s.sample(666, uniformization=True)
    U, Ui, lam = eig.evec, eig.ievc, eig.evals
    P = (U * np.exp(lam * g["mu"])) @ Ui
    post = pi * P[:, 0] * P[:, 0]
    post = post / post.sum()
    cond = mr.tables(U, Ui, lam, s.registers, s.kinds, s.scale_by_time, [0.0, 1.0, 1.0], None, [g["mu"]], np.stack([P[None]] * 3))
    exact = np.array([2.0 * np.sum(post * cond[k, 1, 0, :, 0]) for k in range(3)])
    mean = out["pattern"].mean(axis=1)
    se = out["pattern"].std(axis=1) / np.sqrt(N)
    assert np.all(np.abs(mean - exact) <= 5 * se), (mean, exact, se)
    tl.close()


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


@pytest.mark.parametrize("shards", [1, 3], indirect=True)
def test_sharded_handle_gives_what_one_instance_gives(shards):
    g = len(bm.beagle.engine().resource_list()) - 2
    wl = helpers.random_workload(40, 3001, 4, 4, seed=901)
    single, multi = make(wl), make(wl, resource_list=(g + 1,))
    a = registers(MarkovJumpsSampler(single), 4, seed=2)
    b = registers(MarkovJumpsSampler(multi), 4, seed=2)
    for history, sims in ((True, 1), (False, 3)):
        x = raw_call(a, 31, sims, history, states=True, jumps=True)
        y = raw_call(b, 31, sims, history, states=True, jumps=True)
        for key in x:
            if key != "row_totals":
                assert np.array_equal(x[key], y[key]), key
        np.testing.assert_allclose(y["row_totals"], x["row_totals"], rtol=1e-13, atol=1e-13 * np.abs(x["row_totals"]).max())
    single.close(); multi.close()


def test_event_capacity():
    wl = helpers.random_workload(30, 1000, 4, 2, seed=71)
    tl = make(wl)
    s = registers(MarkovJumpsSampler(tl), 4, seed=1)
    full = raw_call(s, 8, history=True, jumps=True, states=True)
    assert full["event_total"] > 10
    short = raw_call(s, 8, history=True, jumps=True, states=True, event_capacity=10, retry=False)
    assert short["rc"] == -5 and short["event_total"] == full["event_total"]
    for key in ("states", "categories", "jumps", "pattern_totals", "row_totals", "event_counts"):
        assert np.array_equal(short[key], full[key]), key
    retried = raw_call(s, 8, history=True, jumps=True, states=True, event_capacity=10)
    for key in full:
        assert np.array_equal(retried[key], full[key]), key
    tl.close()


def test_error_codes():
    wl = helpers.random_workload(12, 300, 4, 2, seed=21)
    tl = make(wl)
    s = registers(MarkovJumpsSampler(tl), 4, seed=1)
    rows, order = s.ancestral.node_list()
    times, rates = s.branch_times(order)
    heights = s.node_heights(order)
    Q0 = s.infinitesimal_matrix()

    def code(regs=None, flags=None, Q=Q0, sims=1, history=False, h=heights, **kw):
        regs = np.stack(s.registers) if regs is None else regs
        flags = s.flags() if flags is None else flags
        with pytest.raises(bm.beagle.BeagleException) as e:
            s.beagle.sampleMarkovJumpsUniformized(rows, times, rates, h, Q, kw.get("rates", 0), 0, 0, regs, flags, 1, simulants=sims,
                                                  history=history, pattern_totals=kw.get("pt", True), row_totals=kw.get("rt", True))
        return e.value.code

    assert code(regs=np.zeros((0, 4, 4)), flags=np.zeros(0, dtype=np.int32)) == -5
    assert code(regs=np.zeros((9, 4, 4)), flags=np.zeros(9, dtype=np.int32)) == -5
    assert code(flags=np.array([0, 4, 0, 0, 0], dtype=np.int32)) == -5
    assert code(sims=0) == -5 and code(sims=1025) == -5
    assert code(Q=np.zeros((4, 4))) == -5 and code(Q=np.full((4, 4), np.nan)) == -5
    assert code(pt=False, rt=False) == -5
    assert code(history=True, sims=2) == -5 and code(history=True, h=None) == -5
    assert code(rates=-1) == -5
    s.beagle.setPatternPartitions(2, (np.arange(wl.pattern_count) >= wl.pattern_count // 2).astype(np.int32))
    assert code() == -7
    tl.close()


def test_jump_calls_leave_the_likelihood_path_alone():
    wl = helpers.random_workload(60, 2000, 4, 4, seed=55)
    a, b = make(wl), make(wl)
    s = registers(MarkovJumpsSampler(a), 4, seed=4)
    rng = np.random.default_rng(3)
    height = np.array(wl.tree.height, dtype=float)
    t_, n_ = wl.tree.tip_count, wl.tree.node_count
    la, lb = [a.getLogLikelihood()], [b.getLogLikelihood()]
    calls = 0
    for it in range(30):
        node = int(rng.integers(t_, n_))
        while wl.tree.parent[node] < 0:
            node = int(rng.integers(t_, n_))
        lo = max(height[int(wl.tree.left[node])], height[int(wl.tree.right[node])])
        hi = height[wl.tree.parent[node]]
        old = float(height[node])
        height[node] = lo + (hi - lo) * float(rng.uniform(0.1, 0.9))
        for t in (a, b):
            t.storeState()
            t.set_node_height(node, float(height[node]))
        la.append(a.getLogLikelihood()); lb.append(b.getLogLikelihood())
        if it % 3 == 1:
            for t in (a, b):
                t.restoreState()
                t.restore_node_height(node, old)
            height[node] = old
            la.append(a.getLogLikelihood()); lb.append(b.getLogLikelihood())
        if it % 5 == 4:
            out = s.sample(it, per_site=it % 10 == 4, uniformization=True, history=it % 10 == 9)
            assert a.node_height(node) == height[node]
            calls += 1
    assert calls == 6
    assert la == lb                                           # bitwise
    for t in (a, b):
        st = helpers.walk_stats(t)
        assert st["walks"] > 0 and st["fast_walks"] == st["walks"], st
    a.close(); b.close()


def test_full_size_totals_on_chosen_patterns():
    a = synth.config_a(scale=0.01)
    wl = synth.make_workload("A:GTR+G4", 1000, 10000, a.eig, a.freqs, seed=1)     # config A's model, 1000 taxa x 1e4 patterns
    tl = make(wl)
    s = registers(MarkovJumpsSampler(tl), 4, seed=6)
    res = raw_call(s, 2027, states=True)
    P = tl.pattern_count
    pats = np.random.default_rng(1).choice(P, 500, replace=False)
    pats.sort()
    ref = restated(tl, s, res["states"][:, pats], res["categories"][pats], 2027, 1, patterns=pats, pattern_count=P)
    ok = ~ref["near"].any(axis=0)
    assert ok.mean() >= 0.99
    close(res["pattern_totals"][:, pats][:, ok], ref["pattern_totals"][:, ok])
    tl.close()
