"""Ancestral-state draws on the GPU (include/beagle_mi355.h beagleMi355SampleAncestralStates, beast-mcmc_amd/ancestral.py) against
the host restatement (tests/ancestral_reference.py) over what the engine reads back: states and categories must be IDENTICAL."""
import ctypes as C
import os

import numpy as np
import pytest

import ancestral_reference as ar
import beast_mcmc_amd as bm
import helpers
from beast_mcmc_amd.ancestral import AncestralStateSampler
from beast_mcmc_amd.treelikelihood import RESCALE_ALWAYS, RESCALE_DYNAMIC, BeagleTreeLikelihood

pytestmark = pytest.mark.gpu


def make(wl, **kw):
    tl = BeagleTreeLikelihood(wl, **kw)
    tl.workload = wl                      # (the model arrays the caller set: the restatement's category weights and frequencies)
    return tl


def restated(tl, sampler, seed, use_map=False, compact=None, patterns=None):
    rows = sampler.node_list()[0]
    compact = set(range(tl.tip_count)) if compact is None else compact
    return ar.sample_from_engine(sampler.beagle, rows, compact, tl.workload.cat_weights, tl.workload.freqs, seed, use_map=use_map,
                                 patterns=patterns)


def check_identical(tl, sampler, seed, use_map, compact=None):
    states, cats = sampler.sample(seed, map=use_map)
    rows, order = sampler.node_list()
    ref, ref_cats, bad = restated(tl, sampler, seed, use_map, compact)
    assert not bad
    assert np.array_equal(cats, ref_cats)
    assert np.array_equal(states[order], ref), np.argwhere(states[order] != ref)[:5]
    return states, cats


@pytest.mark.parametrize("S,C,T,P,rescale", [
    (4, 4, 9, 300, False),       # small tree: most internal nodes are virtual subtrees until the draw materialises them
    (4, 1, 40, 1000, False),     # deeper tree
    (4, 3, 25, 257, True),       # stored partials carry scale factors
    (20, 2, 8, 100, False),      # T32 layout
    (61, 1, 6, 70, False),       # T32 layout, 16 state tiles
    (7, 2, 6, 50, False),        # general-S layout
])
def test_draws_equal_the_restatement(S, C, T, P, rescale):
    wl = helpers.random_workload(T, P, S, C, seed=100 + S + T)
    tl = make(wl, rescaling=RESCALE_ALWAYS if rescale else RESCALE_DYNAMIC, delay_rescaling=not rescale)
    tl.getLogLikelihood()
    sampler = AncestralStateSampler(tl)
    for use_map in (False, True):
        states, cats = check_identical(tl, sampler, 2024 + S, use_map)
    assert np.array_equal(states[:T][wl.tip_states < S], wl.tip_states[wl.tip_states < S])     # known tips are copied
    if C > 1:
        assert len(np.unique(cats)) > 1
    tl.close()


def test_caterpillar_of_2000_tips():
    wl = helpers.random_workload(2000, 300, 4, 2, seed=77, tree_kind="caterpillar", root_to_tip=2.0)
    tl = make(wl)
    assert np.isfinite(tl.getLogLikelihood())
    sampler = AncestralStateSampler(tl)
    check_identical(tl, sampler, 5, False)
    tl.close()


def test_unknown_compact_tips_and_tips_with_partials():
    wl = helpers.random_workload(30, 400, 4, 4, seed=31, unknown_fraction=0.2)
    tl = make(wl)
    rng = np.random.default_rng(4)
    with_partials = [0, 3, 11]
    for t in with_partials:
        part = rng.uniform(0.0, 1.0, size=(wl.pattern_count, 4))
        part[rng.random(wl.pattern_count) < 0.5] = 1.0                     # ambiguous sites
        part = np.ascontiguousarray(part)
        assert tl.h.btlSetTipPartials(tl.ptr, t, part.ctypes.data_as(C.POINTER(C.c_double))) == 0
    tl.getLogLikelihood()
    sampler = AncestralStateSampler(tl)
    compact = set(range(wl.tip_count)) - set(with_partials)
    for use_map in (False, True):
        states, _ = check_identical(tl, sampler, 99, use_map, compact=compact)
    unknown = wl.tip_states[1] >= 4
    assert unknown.any() and np.all(states[1][unknown] < 4)
    tl.close()


def test_seeds():
    wl = helpers.random_workload(20, 500, 4, 4, seed=8)
    tl = make(wl)
    tl.getLogLikelihood()
    sampler = AncestralStateSampler(tl)
    a, ca = sampler.sample(1)
    b, cb = sampler.sample(1)
    c, cc = sampler.sample(2)
    assert np.array_equal(a, b) and np.array_equal(ca, cb)
    assert not np.array_equal(a, c) and not np.array_equal(ca, cc)
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
def test_sharded_handle_draws_what_one_instance_draws(shards):
    g = len(bm.beagle.engine().resource_list()) - 2
    wl = helpers.random_workload(40, 3001, 4, 4, seed=901)
    single = make(wl)
    multi = make(wl, resource_list=(g + 1,))
    assert single.getLogLikelihood() == pytest.approx(multi.getLogLikelihood(), rel=1e-12)
    s1, s2 = AncestralStateSampler(single), AncestralStateSampler(multi)
    for use_map in (False, True):
        a, ca = s1.sample(31, map=use_map)
        b, cb = s2.sample(31, map=use_map)
        assert np.array_equal(a, b) and np.array_equal(ca, cb)
    single.close(); multi.close()


def test_draws_leave_the_likelihood_path_alone():
    wl = helpers.random_workload(60, 2000, 4, 4, seed=55)
    a, b = make(wl), make(wl)
    sampler = AncestralStateSampler(a)
    rng = np.random.default_rng(3)
    height = np.array(wl.tree.height, dtype=float)
    t_, n_ = wl.tree.tip_count, wl.tree.node_count
    la, lb = [a.getLogLikelihood()], [b.getLogLikelihood()]
    draws = 0
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
            sampler.sample(it)
            draws += 1
    assert draws == 6
    assert la == lb                                           # bitwise
    for t in (a, b):
        st = helpers.walk_stats(t)
        assert st["walks"] > 0 and st["fast_walks"] == st["walks"], st
    a.close(); b.close()


def test_error_codes():
    wl = helpers.random_workload(12, 300, 4, 2, seed=21)
    tl = make(wl)
    tl.getLogLikelihood()
    sampler = AncestralStateSampler(tl)
    raw = sampler.beagle
    rows, order = sampler.node_list()

    def code(r, **kw):
        with pytest.raises(bm.beagle.BeagleException) as e:
            raw.sampleAncestralStates(r, kw.get("w", 0), kw.get("f", 0), 1)
        return e.value.code

    bad = rows.copy(); bad[3, 2] = 5                                  # parent after its child
    assert code(bad) == -5
    bad = rows.copy(); bad[2, 2] = 2                                  # parent = itself
    assert code(bad) == -5
    bad = rows.copy(); bad[4, 0] = 10 ** 6                            # buffer
    assert code(bad) == -5
    bad = rows.copy(); bad[4, 1] = -1                                 # matrix
    assert code(bad) == -5
    assert code(rows, w=7) == -5 and code(rows, f=-1) == -5
    tip_row = int(np.flatnonzero(order < wl.tip_count)[0])
    bad = rows.copy(); bad[0, 0] = rows[tip_row, 0]                   # a compact tip as the root
    assert code(bad) == -5
    f = raw._ext("beagleMi355SampleAncestralStates", [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_ulonglong, C.c_int,
                                                       C.c_void_p, C.c_void_p])
    out = np.zeros((len(rows), wl.pattern_count), dtype=np.uint8)
    r = np.ascontiguousarray(rows)
    assert f(raw.instance, r.ctypes.data, 0, 0, 0, 1, 0, out.ctypes.data, None) == -5
    assert f(raw.instance, r.ctypes.data, len(rows), 0, 0, 1, 0, None, None) == -5
    assert f(raw.instance, r.ctypes.data, len(rows), 0, 0, 1, 0, out.ctypes.data, None) == 0      # categories may be NULL
    # -8: one tip's partials all zero — that tip's states are 0, every other draw is still made
    t0 = int(order[tip_row])
    raw.setTipPartials(t0, np.zeros(wl.pattern_count * 4))
    compact = set(range(wl.tip_count)) - {t0}
    ref, ref_cats, any_bad = restated(tl, sampler, 17, compact=compact)
    assert any_bad
    assert f(raw.instance, r.ctypes.data, len(rows), 0, 0, 17, 0, out.ctypes.data, None) == -8
    assert np.array_equal(out, ref)
    assert np.all(out[tip_row] == 0) and out[0].any() and out[np.arange(len(rows)) != tip_row].any()
    with pytest.raises(bm.beagle.BeagleException) as e:
        raw.sampleAncestralStates(rows, 0, 0, 17)
    assert e.value.code == -8
    # -7: an instance with pattern partitions
    raw.setPatternPartitions(2, (np.arange(wl.pattern_count) >= wl.pattern_count // 2).astype(np.int32))   # (contiguous ranges)
    assert code(rows) == -7
    tl.close()


def test_headline_size():
    wl = bm.synth.config_a()
    tl = make(wl)
    tl.getLogLikelihood()
    sampler = AncestralStateSampler(tl)
    states, cats = sampler.sample(2026)
    rows, order = sampler.node_list()
    pats = helpers.sample_with_tail(wl.pattern_count, 2000, seed=6)
    ref, ref_cats, bad = restated(tl, sampler, 2026, patterns=pats)
    # (the restatement keys the random numbers on the whole alignment's pattern index)
    assert not bad
    assert np.array_equal(cats[pats], ref_cats)
    assert np.array_equal(states[order][:, pats], ref)
    tl.close()
