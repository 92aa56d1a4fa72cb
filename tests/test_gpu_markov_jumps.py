"""Markov jumps on the GPU (include/beagle_mi355.h beagleMi355SampleMarkovJumps, beast-mcmc_amd/markovjumps.py) against the host
restatement (tests/markov_jumps_reference.py) over what the engine reads back: the draw must be the ancestral sampler's byte for
byte, the values and totals equal to 1e-12 relative, with an absolute floor from the row's scale: 1e-15 (a few ulps) of what the entry's terms
add up to in magnitude, |U| ((|A| o |M_k|) |U^-1|) / P (the kernels and the restatement form every product and sum alike; the
device's exp() and the host's differ in the last bit, and a table entry is a difference of terms far larger than itself where P is
small or the branch short).  An error that kernel and restatement share, or one the floor is sized to forgive, is invisible here:
tests/test_gpu_markov_jumps_exact.py holds the same tables to an exact yardstick with no eigenvalue in it, on tied and nearly tied
models, short branches and a zero-length branch, which the cases below stay away from.
"""
import os

import numpy as np
import pytest

import beast_mcmc_amd as bm
import helpers
import markov_jumps_reference as mr
from beast_mcmc_amd.inputs import substmodel, synth, trees
from beast_mcmc_amd.markovjumps import MarkovJumpsSampler
from beast_mcmc_amd.treelikelihood import RESCALE_ALWAYS, RESCALE_DYNAMIC, BeagleTreeLikelihood

pytestmark = pytest.mark.gpu


def three_registers(sampler, S, seed):
    rng = np.random.default_rng(seed)
    sampler.add_register("jump", np.ones((S, S)))
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


def restated(tl, s, states, cats, pattern_count=None):
    """-> (values [K][n][P], pattern totals [K][P], row totals [K][n], floors) of the restatement for the drawn `states` (row order);
    floors: the same three of 1e-15 x the magnitudes of the gathered entries (module docstring)."""
    rows, order = s.ancestral.node_list()
    times, rates = s.branch_times(order)
    S, C = tl.state_count, tl.category_count
    mats = np.zeros((len(rows), C, S, S))
    cache = {}
    for r in range(1, len(rows)):
        m = int(rows[r, 1])
        if m not in cache:
            cache[m] = s.beagle.getTransitionMatrix(m).reshape(C, S, S)
        mats[r] = cache[m]
    eig = tl.eig
    kinds = s.kinds
    cond = mr.tables(eig.evec, eig.ievc, eig.evals, s.registers, kinds, s.scale_by_time, times, rates, tl.cat_rates, mats)
    mags = mr.magnitudes(eig.evec, eig.ievc, eig.evals, s.registers, kinds, s.scale_by_time, times, rates, tl.cat_rates, mats)
    floors = mr.site_values(1e-15 * mags, states, rows[:, 2], cats)
    return mr.site_values(cond, states, rows[:, 2], cats) + (floors,)


def assert_close(a, b, floor):
    """|a - b| <= 1e-12 |b| + floor"""
    err = np.abs(a - b)
    bad = err > 1e-12 * np.abs(b) + floor
    assert not bad.any(), (np.argwhere(bad)[:5], a[bad][:5], b[bad][:5])


def raw_call(s, seed, use_map=False, **kw):
    rows, order = s.ancestral.node_list()
    times, rates = s.branch_times(order)
    return s.beagle.sampleMarkovJumps(rows, times, rates, s.tl.eigen_index(), 0, 0, 0, np.stack(s.registers), s.flags(), seed,
                                      map=use_map, **kw)


def check_against_restatement(tl, s, seed, use_map):
    res = raw_call(s, seed, use_map, states=True, jumps=True)
    rows, _ = s.ancestral.node_list()
    st, ca = s.beagle.sampleAncestralStates(rows, 0, 0, seed, map=use_map)
    assert np.array_equal(res["states"], st) and np.array_equal(res["categories"], ca)       # the sampler's draw, byte for byte
    vals, tot, row_tot, floors = restated(tl, s, st, ca)
    assert_close(res["jumps"], vals, floors[0])
    assert_close(res["pattern_totals"], tot, floors[1])
    assert_close(res["row_totals"], row_tot, floors[2])
    again = raw_call(s, seed, use_map, states=True, jumps=True)
    for key in res:
        assert np.array_equal(res[key], again[key]), key                                     # deterministic
    return res


@pytest.mark.parametrize("S,C,T,P,rescale", [
    (4, 4, 9, 300, False),
    (4, 3, 25, 257, True),       # stored partials carry scale factors
    (4, 1, 12, 500, False),
    (20, 2, 8, 100, False),      # T32 layout
    (61, 1, 6, 70, False),       # 16 state tiles; the widest LDS table
    (7, 2, 6, 50, False),        # general-S layout
    (100, 2, 5, 40, False),      # one entry per thread
])
def test_jumps_equal_the_restatement(S, C, T, P, rescale):
    wl = helpers.random_workload(T, P, S, C, seed=300 + S + T)
    tl = make(wl, branch_rate_seed=S, rescaling=RESCALE_ALWAYS if rescale else RESCALE_DYNAMIC, delay_rescaling=not rescale)
    s = three_registers(MarkovJumpsSampler(tl), S, seed=S)
    for use_map in (False, True):
        res = check_against_restatement(tl, s, 77 + S, use_map)
    assert np.all(res["jumps"][:, 0] == 0.0) and np.all(res["row_totals"][:, 0] == 0.0)
    assert np.all(res["jumps"][0] >= 0.0) and res["jumps"][0].sum() > 0.0
    tl.close()


def test_zero_rate_category():
    wl = helpers.random_workload(10, 400, 4, 3, seed=41)
    tl = BeagleTreeLikelihood(wl)
    tl.set_site_model([0.0, 1.2, 1.8], [0.3, 0.4, 0.3])           # p-inv: category 0 has rate 0
    tl.getLogLikelihood()
    s = three_registers(MarkovJumpsSampler(tl), 4, seed=3)
    res = check_against_restatement(tl, s, 5, False)
    inv = res["categories"] == 0
    assert inv.any() and (~inv).any()
    rows, order = s.ancestral.node_list()
    times, _ = s.branch_times(order)
    assert np.all(res["jumps"][0][:, inv] == 0.0) and np.all(res["jumps"][1][:, inv] == 0.0)
    assert np.array_equal(res["jumps"][2][1:, inv], np.broadcast_to(times[1:, None], (len(rows) - 1, inv.sum())))
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
    s = three_registers(MarkovJumpsSampler(tl), 4, seed=9)
    for use_map in (False, True):
        check_against_restatement(tl, s, 99, use_map)
    tl.close()


def test_a_tenth_of_config_a_without_states():
    wl = synth.config_a(scale=0.1)
    tl = make(wl)
    s = three_registers(MarkovJumpsSampler(tl), 4, seed=1)
    res = raw_call(s, 2026)
    assert set(res) == {"pattern_totals", "row_totals"}
    rows, _ = s.ancestral.node_list()
    st, ca = s.beagle.sampleAncestralStates(rows, 0, 0, 2026)
    _, tot, row_tot, floors = restated(tl, s, st, ca)
    assert_close(res["pattern_totals"], tot, floors[1])
    assert_close(res["row_totals"], row_tot, floors[2])
    out = s.sample(2026)                                             # the node-indexed view of the same call
    assert np.array_equal(out["pattern"], res["pattern_totals"])
    assert np.array_equal(out["branch"][:, np.asarray(s.ancestral.node_list()[1])], res["row_totals"])
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


@pytest.mark.parametrize("shards", [0, 3], indirect=True)
def test_sharded_handle_gives_what_one_instance_gives(shards):
    g = len(bm.beagle.engine().resource_list()) - 2
    wl = helpers.random_workload(40, 3001, 4, 4, seed=901)
    single, multi = make(wl), make(wl, resource_list=(g + 1,))
    a = three_registers(MarkovJumpsSampler(single), 4, seed=2)
    b = three_registers(MarkovJumpsSampler(multi), 4, seed=2)
    for use_map in (False, True):
        x = raw_call(a, 31, use_map, states=True, jumps=True)
        y = raw_call(b, 31, use_map, states=True, jumps=True)
        for key in ("states", "categories", "jumps", "pattern_totals"):
            assert np.array_equal(x[key], y[key]), key
        np.testing.assert_allclose(y["row_totals"], x["row_totals"], rtol=1e-13, atol=1e-13 * np.abs(x["row_totals"]).max())
    single.close(); multi.close()


def test_two_tip_expectations_on_the_device():
    """MarkovJumpsTest (src/test/dr/app/beagle/MarkovJumpsTest.java): HKY kappa 10, two tips at distance 1, both A, mu 0.5; 10 000
    identical patterns are 10 000 independent draws.  Each register's mean is within 4 standard errors of the exact enumeration."""
    import json
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
    out = s.sample(666)
    U, Ui, lam = eig.evec, eig.ievc, eig.evals
    P = (U * np.exp(lam * g["mu"])) @ Ui
    post = pi * P[:, 0] * P[:, 0]
    post = post / post.sum()
    cond = mr.tables(U, Ui, lam, s.registers, s.kinds, s.scale_by_time, [0.0, 1.0, 1.0], None, [g["mu"]], np.stack([P[None]] * 3))
    exact = np.array([2.0 * np.sum(post * cond[k, 1, 0, :, 0]) for k in range(3)])
    np.testing.assert_allclose(exact, g["valuesFromR"], atol=g["tolerance"])
    mean = out["pattern"].mean(axis=1)
    se = out["pattern"].std(axis=1) / np.sqrt(N)
    assert np.all(np.abs(mean - exact) <= 4 * se), (mean, exact, se)
    tl.close()


def test_error_codes():
    wl = helpers.random_workload(12, 300, 4, 2, seed=21)
    tl = make(wl)
    s = three_registers(MarkovJumpsSampler(tl), 4, seed=1)
    rows, order = s.ancestral.node_list()
    times, rates = s.branch_times(order)

    def code(regs=None, flags=None, **kw):
        regs = np.stack(s.registers) if regs is None else regs
        flags = s.flags() if flags is None else flags
        with pytest.raises(bm.beagle.BeagleException) as e:
            s.beagle.sampleMarkovJumps(rows, times, rates, kw.get("eig", tl.eigen_index()), kw.get("rates", 0), 0, 0, regs, flags, 1,
                                       pattern_totals=kw.get("pt", True), row_totals=kw.get("rt", True))
        return e.value.code

    assert code(regs=np.zeros((0, 4, 4)), flags=np.zeros(0, dtype=np.int32)) == -5
    assert code(regs=np.zeros((9, 4, 4)), flags=np.zeros(9, dtype=np.int32)) == -5
    assert code(pt=False, rt=False) == -5
    assert code(flags=np.array([0, 4, 0], dtype=np.int32)) == -5
    assert code(eig=7) == -5 and code(rates=-1) == -5
    s.beagle.setPatternPartitions(2, (np.arange(wl.pattern_count) >= wl.pattern_count // 2).astype(np.int32))
    assert code() == -7
    tl.close()
    cx = bm.beagle.Beagle(3, 5, 3, 4, 10, 1, 4, 2, 0, requirementFlags=bm.beagle.FLAG_EIGEN_COMPLEX)
    with pytest.raises(bm.beagle.BeagleException) as e:
        cx.sampleMarkovJumps([[4, 0, -1], [0, 0, 0]], [0.0, 1.0], None, 0, 0, 0, 0, np.ones((1, 4, 4)), [0], 1)
    assert e.value.code == -7
    cx.finalize()


def test_jump_calls_leave_the_likelihood_path_alone():
    wl = helpers.random_workload(60, 2000, 4, 4, seed=55)
    a, b = make(wl), make(wl)
    s = three_registers(MarkovJumpsSampler(a), 4, seed=4)
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
            s.sample(it, per_site=it % 10 == 4)
            calls += 1
    assert calls == 6
    assert la == lb                                           # bitwise
    for t in (a, b):
        st = helpers.walk_stats(t)
        assert st["walks"] > 0 and st["fast_walks"] == st["walks"], st
    a.close(); b.close()
