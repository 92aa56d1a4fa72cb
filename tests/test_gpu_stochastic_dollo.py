"""The stochastic Dollo (ALS) node-pattern likelihood on the GPU (include/beagle_mi355.h beagleMi355NodePatternLikelihoods,
beast-mcmc_amd/stochasticdollo.py) against the long-double restatement (tests/stochastic_dollo_reference.py) over the partials and
scale factors the engine reads back, against the read-back route on the engine and on the CPU oracle, and its exact properties.

The tolerance of the per-pattern values and the node terms is stochastic_dollo_reference.bound: 8 x max(what the float64
restatement loses against the long-double one, eps x (|value| + the largest |operand| entering it)).  Observed on an MI355X over
the cases below, as a fraction of that bound: at most 0.125 for the pattern values and 0.125 for the node terms (0.125: the
device's bits are the float64 restatement's)
(test_against_the_long_double_yardstick prints the figure of each case).
"""
import ctypes as C
import os

import numpy as np
import pytest

import beast_mcmc_amd as bm
import helpers
import stochastic_dollo_cases as cases
import stochastic_dollo_reference as ref
from beast_mcmc_amd.stochasticdollo import ALSTreeLikelihood

pytestmark = pytest.mark.gpu

NONE = bm.beagle.NONE
SETTINGS = [(obs, integrate, lists) for obs in ("anyTip", "singleTip") for integrate in (False, True)
            for lists in (((), ()), ((0,), ()), ((), (0,)))]


def build(tips, kind, P, S, C, partial_tips, rescale, library=None, resource_list=(1,), seed=0, **model):
    tree = cases.ladder(tips, 0.25) if kind == "ladder" else cases.random_tree(tips, seed=40 + tips + seed)
    states = cases.random_alignment(tips, P, S, seed=50 + P + S + seed)
    freqs, base = cases.random_model(S, 60 + S)
    rates, weights = cases.site_rates(C)
    pattern_weights = np.arange(P) % 3 + 1.0
    model.setdefault("death_rate", 0.8)
    model.setdefault("lam", 1.6)
    als = ALSTreeLikelihood.create(tree, states, pattern_weights, freqs, rates, weights, library=library, resource_list=resource_list,
                                   base_generator=base, mutation_rate=0.9, rescale=rescale,
                                   branch_rates=np.linspace(0.6, 1.4, tree.node_count), **model)
    if partial_tips:
        for t, part in cases.tips_as_partials(states, S, [0, tips // 2, tips - 1], seed=70 + seed).items():
            als.set_tip_partials(t, part)
    return als


def yardstick(als):
    """-> (long-double pattern values, their bound, long-double terms [row][P], their bound) from what the engine reads back."""
    partials, scales = als.read_back()
    extant = ref.tip_extant(als.tip_states, als.tip_partials, als.S, als.death_state)
    _, incl = ref.inclusion(als.tree, extant)
    logw = [np.log(ref.node_survival_probability(als.tree, n, als.mu, als.average_rate(), als.branch_rates))
            for n in range(als.tree.node_count)]
    order = als.tree.postorder()
    out = {}
    for dt in (np.float64, np.longdouble):
        terms, operand = ref.log_terms(als.tree, order, partials, scales, incl, als.freqs, als.tl.cat_weights, logw, dt)
        out[dt] = (terms, operand, ref.log_cum(terms, dt))
    t64, _, v64 = out[np.float64]
    tld, operand, vld = out[np.longdouble]
    with np.errstate(invalid="ignore"):
        largest = np.where(np.isfinite(tld), np.abs(tld), 0).max(axis=0)
    return vld, ref.bound(v64, vld, largest), tld, ref.bound(t64, tld, operand)


def held_to(value, yard, bound):
    """the largest |value - yardstick| as a fraction of the bound; -inf must be -inf exactly"""
    yard64 = np.asarray(yard, dtype=np.float64)
    assert np.array_equal(np.isneginf(value), np.isneginf(yard64))
    finite = np.isfinite(yard64)
    diff = np.abs(value[finite].astype(np.longdouble) - np.asarray(yard)[finite]).astype(np.float64)
    assert np.all(diff <= bound[finite]), float((diff / bound[finite]).max())
    exact = bound[finite] == 0.0                              # (a value of exactly 0 from operands that are all 0)
    return float((diff[~exact] / bound[finite][~exact]).max()) if np.any(~exact) else 0.0


def root_value(als):
    out = np.zeros(1)
    als.beagle.calculateRootLogLikelihoods([als.tl.node_buffer_index(als.tree.root)], [0], [0], [NONE], 1, out)
    return out[0]


CASES = [
    ("binary-9", 9, "random", 33, 2, 1, False, False),
    ("three-12-scaled", 12, "random", 130, 3, 4, True, True),
    ("five-9", 9, "random", 257, 5, 1, True, False),
    ("t32-12-scaled-one-pattern", 12, "random", 1, 21, 4, False, True),
    ("t32-9-partial-tips", 9, "random", 130, 21, 1, True, False),
    ("ladder-40", 40, "ladder", 257, 2, 4, False, True),
    ("walk-12", 12, "random", 257, 4, 4, False, False),
    ("walk-9-scaled", 9, "random", 33, 4, 1, True, True),
]


@pytest.mark.parametrize("name,tips,kind,P,S,C,partial_tips,rescale", CASES, ids=[c[0] for c in CASES])
def test_against_the_long_double_yardstick(name, tips, kind, P, S, C, partial_tips, rescale):
    als = build(tips, kind, P, S, C, partial_tips, rescale)
    als.prune()
    before = root_value(als)
    stats0 = als.beagle.nodePatternStats()
    value = als.log_pattern_device(node_terms=True)
    terms, total, rc = als.last["terms"], als.last["sum"], als.last["rc"]
    stats1 = als.beagle.nodePatternStats()
    assert rc == 0 and np.all(np.isfinite(value))
    assert stats1["calls"] == stats0["calls"] + 1 and stats1["rows"] == stats0["rows"] + 2 * tips - 1
    if name == "walk-12":
        # the 4-state walk leaves nodes unstored when nothing rescales: the call has them written, as a read-back does
        assert stats1["materialised"] > stats0["materialised"]

    vld, vbound, tld, tbound = yardstick(als)
    ratio_v = held_to(value, vld, vbound)
    ratio_t = held_to(terms, tld, tbound)
    print("%s: largest error as a fraction of the bound: pattern values %.3g, node terms %.3g" % (name, ratio_v, ratio_t))
    # the weighted sum: the values' own bounds, and one rounding per addition of the P products (all of one sign or not)
    weighted = als.pattern_weights.astype(np.longdouble) * vld
    sum_bound = float(np.sum(als.pattern_weights * vbound)) + (P + 1) * np.finfo(np.float64).eps * float(np.sum(np.abs(weighted)))
    assert abs(total - float(np.sum(weighted))) <= sum_bound

    # the same bits from a second call, with and without the node terms; nothing of the instance has changed
    again = als.log_pattern_device(node_terms=True)
    assert np.array_equal(again, value) and np.array_equal(als.last["terms"], terms) and als.last["sum"] == total
    assert np.array_equal(als.log_pattern_device(), value) and als.last["sum"] == total
    after = root_value(als)
    assert after == before or (np.isnan(after) and np.isnan(before))

    # the full likelihood against the read-back route, on the engine and on the CPU oracle
    readback = als.log_pattern_readback()
    oracle = build(tips, kind, P, S, C, partial_tips, rescale, library=helpers.oracle_library())
    oracle.prune()
    oracle_value = oracle.log_pattern_readback()
    for observation, integrate, lists in SETTINGS:
        for x in (als, oracle):
            x.observation, x.integrate_gain_rate, x.include, x.exclude = observation, integrate, list(lists[0]), list(lists[1])
        lnl = als.finish(value)
        assert np.isfinite(lnl)
        assert abs(lnl - als.finish(readback)) <= 1e-10 * abs(lnl)
        assert abs(lnl - oracle.finish(oracle_value)) <= 1e-10 * abs(lnl)
    als.observation, als.integrate_gain_rate, als.include, als.exclude = "anyTip", False, [], []
    assert als.getLogLikelihood() == pytest.approx(als.finish(value), rel=1e-12)      # (a second pruning pass: the walk may round differently)
    als.close(); oracle.close()


def test_underflow_ladder_stays_finite():
    """The ladder on which the reference's linear-space sum is 0 in float64 (tests/test_stochastic_dollo_host.py)."""
    tips = cases.UNDERFLOW_LADDER_TIPS
    tree = cases.ladder(tips)
    states = np.ones((tips, 3), dtype=np.int32)
    states[:, 0] = 0
    states[:2, 1] = 0
    states[-1, 2] = 0
    als = ALSTreeLikelihood.create(tree, states, np.ones(3), [1.0, 0.0], [1.0], [1.0], death_rate=1.0, lam=1.0, rescale=True)
    als.prune()
    value = als.log_pattern_device(node_terms=True)
    assert als.last["rc"] == 0 and np.all(np.isfinite(value)) and value[0] < np.log(np.finfo(np.float64).tiny)
    vld, vbound, tld, tbound = yardstick(als)
    held_to(value, vld, vbound)
    held_to(als.last["terms"], tld, tbound)
    partials, scales = als.read_back()
    extant = ref.tip_extant(states, {}, 2, 1)
    _, incl = ref.inclusion(tree, extant)
    logw = [np.log(ref.node_survival_probability(tree, n, 1.0, 1.0)) for n in range(tree.node_count)]
    linear = ref.linear_cum(tree, partials, scales, incl, als.freqs, [1.0], logw, np.float64)
    assert linear[0] == 0.0                                   # what the reference would have taken the logarithm of
    lnl = als.finish(value)
    assert np.isfinite(lnl) and abs(lnl - als.finish(als.log_pattern_readback())) <= 1e-10 * abs(lnl)
    als.close()


def test_pattern_sum_is_the_tree_weight():
    """tests/test_stochastic_dollo_host.py::test_pattern_sum_is_the_tree_weight on the device."""
    tree = cases.eight_tip_tree()
    states = cases.all_extant_patterns(8)
    als = ALSTreeLikelihood.create(tree, states, np.ones(255), [1.0, 0.0], [1.0], [1.0], death_rate=0.7, lam=1.3)
    als.prune()
    value = als.log_pattern_device()
    expect = ref.tree_weight_sum(tree, 0.7, 1.0)
    assert abs(np.exp(value).sum() - expect) <= 1e-13 * expect
    als.close()


def forest_rows(als):
    """The node list without the root: two subtrees, so a pattern extant in both is included in no row."""
    rows, logw, order = als.node_rows()
    assert order[-1] == als.tree.root
    return rows[:-1].copy(), logw[:-1].copy(), order[:-1]


def test_minus_infinity_exactly_where_no_node_is_included():
    als = build(9, "random", 130, 2, 1, False, False)
    als.prune()
    rows, logw, order = forest_rows(als)
    stats0 = als.beagle.nodePatternStats()
    value, terms, total, rc = als.beagle.nodePatternLikelihoods(rows, logw, als.death_state, node_terms=True)
    extant = ref.tip_extant(als.tip_states, {}, 2, 1)
    below, _ = ref.inclusion(als.tree, extant)
    total_extant = extant.sum(axis=0)
    included = below[order] >= total_extant[None, :]
    nowhere = ~included.any(axis=0)
    assert nowhere.any() and not nowhere.all()
    assert np.array_equal(np.isneginf(value), nowhere) and np.all(np.isfinite(value[~nowhere]))
    # a term is -inf where the row is excluded — and where its site likelihood is 0: a tip in the death state (frequency 0), which is
    # included only in a pattern with no extant tip at all
    dead_tip = (order < als.tree.tip_count)[:, None] & (als.tip_states[np.minimum(order, als.tree.tip_count - 1)] == als.death_state)
    assert (included & dead_tip).any()
    assert np.array_equal(np.isneginf(terms), ~included | dead_tip) and np.all(np.isfinite(terms[included & ~dead_tip]))
    assert rc == -8 and total == -np.inf                       # the sum is not finite; the outputs are written all the same
    assert als.beagle.nodePatternStats()["empty_patterns"] == stats0["empty_patterns"] + int(nowhere.sum())
    # a pattern with one included row is that row's term exactly
    single = (included & ~dead_tip).sum(axis=0) == 1
    assert single.any()
    assert np.array_equal(value[single], np.where(included & ~dead_tip, terms, 0.0).sum(axis=0)[single])
    als.close()


def test_pattern_chunks_give_the_same_bits():
    als = build(12, "random", 700, 3, 2, True, True)
    als.prune()
    value = als.log_pattern_device(node_terms=True)
    terms, total = als.last["terms"], als.last["sum"]
    os.environ["BEAGLE_MI355_NODEPATTERN_CHUNK"] = "256"
    try:
        chunked = als.log_pattern_device(node_terms=True)
    finally:
        os.environ.pop("BEAGLE_MI355_NODEPATTERN_CHUNK")
    assert np.array_equal(chunked, value) and np.array_equal(als.last["terms"], terms) and als.last["sum"] == total
    als.close()


def test_three_shards_equal_one_instance_per_pattern():
    """(as tests/test_gpu_sharded_instance.py creates them: three shards on the one device)"""
    single = build(12, "random", 1030, 3, 2, False, True)
    old = os.environ.get("BEAGLE_MI355_SHARDS")
    os.environ["BEAGLE_MI355_SHARDS"] = "3"
    try:
        g = len(bm.beagle.engine().resource_list()) - 2
        multi = build(12, "random", 1030, 3, 2, False, True, resource_list=(g + 1,))
    finally:
        if old is None:
            os.environ.pop("BEAGLE_MI355_SHARDS", None)
        else:
            os.environ["BEAGLE_MI355_SHARDS"] = old
    out = []
    for als in (single, multi):
        als.prune()
        value = als.log_pattern_device(node_terms=True)
        out.append((value, als.last["terms"], als.last["sum"], als.last["rc"]))
    assert out[0][3] == 0 and out[1][3] == 0
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
    assert out[1][2] == pytest.approx(out[0][2], rel=1e-13)     # the shards' sums, added in shard order
    assert multi.beagle.nodePatternStats()["calls"] == 3
    single.close(); multi.close()


def raw_call(als, rows, logw, death, w_idx=0, f_idx=0, flags=0, nodes_null=False, weights_null=False, out_null=False, count=None):
    f = als.beagle._ext("beagleMi355NodePatternLikelihoods", [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                                              C.c_int, C.c_void_p, C.c_void_p, C.c_void_p])
    rows = np.ascontiguousarray(rows, dtype=np.int32)
    logw = np.ascontiguousarray(logw, dtype=np.float64)
    out = np.full(als.P, 123.0)
    total = C.c_double(0.0)
    rc = f(als.beagle.instance, None if nodes_null else rows.ctypes.data, None if weights_null else logw.ctypes.data,
           rows.shape[0] if count is None else count, death, w_idx, f_idx, flags, None if out_null else out.ctypes.data, None,
           C.addressof(total))
    return rc, out


def test_refusals():
    als = build(9, "random", 33, 3, 1, False, True)
    als.prune()
    rows, logw, order = als.node_rows()
    good, out = raw_call(als, rows, logw, 2)
    assert good == 0 and np.all(np.isfinite(out))

    def refused(code, rows=rows, **kw):
        rc, out = raw_call(als, rows, logw, kw.pop("death", 2), **kw)
        assert rc == code, (rc, kw)
        assert np.all(out == 123.0)

    def changed(r, c, v):
        bad = rows.copy()
        bad[r, c] = v
        return bad

    internal = int(np.argmax(rows[:, 2] >= 0))                 # the first internal row
    refused(-5, nodes_null=True)
    refused(-5, weights_null=True)
    refused(-5, out_null=True)
    refused(-5, count=0)
    refused(-5, flags=1)
    refused(-5, death=-1)
    refused(-5, death=3)
    refused(-5, w_idx=-1)
    refused(-5, f_idx=99)
    refused(-5, rows=changed(0, 0, -1))                        # a bad buffer index
    refused(-5, rows=changed(0, 0, 10 ** 6))
    refused(-5, rows=changed(internal, 1, 10 ** 6))            # a bad scale buffer index
    refused(-5, rows=changed(internal, 2, internal))           # a child that is not an earlier row
    refused(-5, rows=changed(internal, 2, -1))                 # one child only
    refused(-5, rows=changed(internal, 2, rows[internal, 3]))  # the same child twice
    refused(-5, rows=changed(len(rows) - 1, 2, rows[internal, 2]))     # a row that is a child of two rows
    refused(-5, rows=changed(internal, 0, rows[0, 0]))         # an internal row over compact tip states
    again, out = raw_call(als, rows, logw, 2)
    assert again == 0 and np.all(np.isfinite(out))
    als.close()

    # a buffer nothing was ever written to: the same list before any pruning pass
    fresh = build(9, "random", 33, 3, 1, False, False)
    rc, out = raw_call(fresh, rows, logw, 2)
    assert rc == -5 and np.all(out == 123.0)
    fresh.close()

    # partitioned instances and BASTA instances
    b = bm.beagle.Beagle(2, 3, 2, 3, 16, 1, 3, 1, 2)
    for t in range(2):
        b.setTipStates(t, np.zeros(16, dtype=np.int32))
    b.setPatternWeights(np.ones(16))
    b.setPatternPartitions(2, np.repeat(np.arange(2, dtype=np.int32), 8))
    tip_rows = np.array([[0, -1, -1, -1], [1, -1, -1, -1]], dtype=np.int32)
    with pytest.raises(bm.beagle.BeagleException) as e:
        b.nodePatternLikelihoods(tip_rows, np.zeros(2), 2)
    assert e.value.code == -7
    b.finalize()
    b = bm.beagle.Beagle(0, 8, 0, 3, 1, 2, 4, 1, 1)
    b.allocateCoalescentBuffers(5, 4, 12, 1)
    with pytest.raises(bm.beagle.BeagleException) as e:
        b.nodePatternLikelihoods(tip_rows, np.zeros(2), 2)
    assert e.value.code == -7
    b.finalize()
