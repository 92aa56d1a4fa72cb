"""Node-height gradients and diagonal Hessians in one call (include/beagle_mi355.h beagleMi355NodeHeightDerivatives) on the HIP
engine, against the numpy restatement of DiscreteTraitNodeHeightDelegate.getNodeDerivatives (tests/node_height_reference.py) run
on what the CPU oracle reads back after the identical call sequence.  The restatement itself is pinned on the CPU tier against
finite differences of the oracle's log-likelihood (tests/test_node_height_host.py); here the bound is the gradient path's 1e-10."""
import os

import numpy as np
import pytest

import beast_mcmc_amd as bm
import helpers
import node_height_reference as nr
from beast_mcmc_amd.nodeheight import NodeHeightGradient

pytestmark = pytest.mark.gpu

REL_TOL = 1e-10


def close(a, b, what):
    a, b = np.asarray(a, dtype=float).ravel(), np.asarray(b, dtype=float).ravel()
    scale = max(1.0, float(np.max(np.abs(b))))
    err = float(np.max(np.abs(a - b))) / scale
    assert err <= REL_TOL, (what, err)


def clock_rates(T, seed):
    return np.random.default_rng(seed).uniform(0.5, 2.0, size=2 * T - 1)        # non-unit rates on every branch


def pair(wl, seed, oracle_lib, **kw):
    rates = clock_rates(wl.tree.tip_count, seed)
    return NodeHeightGradient(wl, rates=rates, **kw), NodeHeightGradient(wl, rates=rates, library=oracle_lib, **kw)


@pytest.mark.parametrize("S,C,T,P,rescale", [
    (4, 4, 9, 300, False),       # 4-state kernel, two workgroups, the second one ragged
    (4, 1, 40, 257, False),      # one category, a deeper tree, one pattern past a workgroup
    (4, 3, 25, 257, True),       # post-order partials with scale factors (every ratio is scale-free)
    (4, 2, 2, 1, False),         # the root alone, both children tips, one pattern
    (7, 2, 6, 50, False),        # general kernel, plain layout
    (20, 2, 8, 100, False),      # general kernel, T32 layout, two workgroups
    (61, 1, 6, 70, False),       # T32 layout, 61 states
])
def test_one_call_matches_the_restatement_on_the_oracle(S, C, T, P, rescale, oracle_lib):
    wl = helpers.random_workload(T, P, S, C, seed=300 + S + T)
    g, o = pair(wl, 11 + T, oracle_lib, rescale=rescale)
    lnl, first, second = g.derivatives()
    lo = o.prepare()
    fo, so = nr.from_plan(o)
    assert first.shape == second.shape == (T - 1,)
    assert helpers.rel_err(lnl, lo) <= REL_TOL
    close(first, fo, "first")
    close(second, so, "second")
    # either output alone
    rows, rates = g.node_rows()
    f1, none = g.b.nodeHeightDerivatives(rows, rates, 0, first=True, second=False)
    assert none is None
    close(f1, fo, "first alone")
    none, s1 = g.b.nodeHeightDerivatives(rows, rates, 0, first=False, second=True)
    assert none is None
    close(s1, so, "second alone")
    # the same bits from a second call, and the likelihood path is undisturbed: the next evaluation gives the bits it gives on a twin
    # instance that was never asked for the derivatives (with rescaling, an instance's second evaluation runs another plan than its
    # first and agrees with it to rounding only, call or no call)
    again = g.b.nodeHeightDerivatives(rows, rates, 0)
    assert np.array_equal(again[0], first) and np.array_equal(again[1], second)
    twin = NodeHeightGradient(wl, rates=g.rates, rescale=rescale)
    assert twin.prepare() == lnl
    assert g.log_likelihood() == twin.log_likelihood()
    g.close(); o.close(); twin.close()


def test_chain_of_evaluations_with_a_held_list_and_unstored_subtrees(oracle_lib):
    """From the second evaluation of a chain on, the 4-state post-order passes leave short subtrees unstored and the pre-order list
    is held back: the call runs the list and materialises what it reads, every time with the oracle's numbers."""
    wl = helpers.random_workload(33, 333, 4, 4, seed=41)
    g, o = pair(wl, 5, oracle_lib)
    rng = np.random.default_rng(2)
    for step in range(3):
        if step:
            node = int(rng.integers(g.T, g.N))
            h = helpers.proposed_height(wl.tree, node, rng)
            g.set_height(node, h); o.set_height(node, h)
        late = g.b.gradientStats()["late"]
        lnl, first, second = g.derivatives()
        assert g.b.gradientStats()["late"] == late + 1, step       # the list was held back until the call ran it
        lo = o.prepare()
        fo, so = nr.from_plan(o)
        assert helpers.rel_err(lnl, lo) <= REL_TOL
        close(first, fo, "first, evaluation %d" % step)
        close(second, so, "second, evaluation %d" % step)
        assert g.log_likelihood() == lnl
    # first = the chain rule over the sums of calculateEdgeDifferentials (DiscreteTraitNodeHeightDelegate.java:69-85)
    _, grad = g.gradient()
    close(first, g.first_from_branch_gradient(grad), "first from the branch gradient")
    g.close(); o.close()


@pytest.mark.parametrize("S,C,T,P", [(4, 2, 10, 130), (20, 1, 6, 40)])
def test_tips_as_partials_and_a_missing_tip(S, C, T, P, oracle_lib):
    wl = helpers.random_workload(T, P, S, C, seed=77 + S)
    wl.tip_states[1][:] = S                                        # one tip unknown at every pattern
    wl.tip_states[2][::3] = S + 1                                  # any state >= S is missing
    g, o = pair(wl, 3, oracle_lib)
    rng = np.random.default_rng(9)
    sent = {0: np.eye(S)[np.minimum(wl.tip_states[0], S - 1)], 3: rng.uniform(0.1, 1.0, size=(P, S))}     # exact states; ambiguity
    for tip, x in sent.items():
        g.b.setTipPartials(tip, x.ravel()); o.b.setTipPartials(tip, x.ravel())
    lnl, first, second = g.derivatives()
    lo = o.prepare()
    fo, so = nr.from_plan(o, compact=set(range(T)) - set(sent))
    assert helpers.rel_err(lnl, lo) <= REL_TOL
    close(first, fo, "first")
    close(second, so, "second")
    g.close(); o.close()


def test_sharded_handle_adds_its_shards(oracle_lib):
    old = os.environ.get("BEAGLE_MI355_SHARDS")
    os.environ["BEAGLE_MI355_SHARDS"] = "3"
    try:
        wl = helpers.random_workload(12, 700, 4, 4, seed=19)
        rates = clock_rates(12, 19)
        all_gpus = len(bm.beagle.engine().resource_list()) - 1
        m = NodeHeightGradient(wl, rates=rates, resource_list=(all_gpus,))
        s = NodeHeightGradient(wl, rates=rates)
        lm, fm, sm = m.derivatives()
        ls, fs, ss = s.derivatives()
        assert helpers.rel_err(lm, ls) <= REL_TOL
        close(fm, fs, "first, sharded")
        close(sm, ss, "second, sharded")
        o = NodeHeightGradient(wl, rates=rates, library=oracle_lib)
        o.prepare()
        fo, so = nr.from_plan(o)
        close(fm, fo, "first, sharded, against the oracle")
        close(sm, so, "second, sharded, against the oracle")
        m.close(); s.close(); o.close()
    finally:
        if old is None:
            os.environ.pop("BEAGLE_MI355_SHARDS", None)
        else:
            os.environ["BEAGLE_MI355_SHARDS"] = old


def test_errors():
    wl = helpers.random_workload(6, 90, 4, 2, seed=5)
    g = NodeHeightGradient(wl, rates=clock_rates(6, 5))
    g.prepare()
    rows, rates = g.node_rows()

    def code(r, **kw):
        with pytest.raises(bm.beagle.BeagleException) as e:
            g.b.nodeHeightDerivatives(r, rates, **kw)
        return e.value.code

    for column in range(8):
        bad = rows.copy(); bad[1, column] = 10 ** 6
        assert code(bad) == -5, column
    for column in range(7):
        bad = rows.copy(); bad[0, column] = -1
        assert code(bad) == -5, column
    bad = rows.copy(); bad[:, 7] = np.where(bad[:, 7] < 0, -2, bad[:, 7])         # only -1 names the root
    assert code(bad) == -5
    bad = rows.copy(); bad[0, 0] = 0                                              # pre(i) holds compact tip states
    assert code(bad) == -5
    assert code(rows, categoryWeightsIndex=7) == -5
    assert code(rows, first=False, second=False) == -5
    first, second = g.b.nodeHeightDerivatives(rows, rates)                        # and the instance still answers
    assert np.all(np.isfinite(first)) and np.all(np.isfinite(second))
    # a partitioned instance, more than 64 states: not built
    g.b.setPatternPartitions(2, np.arange(90) // 45)
    assert code(rows) == -7
    g.close()
    big = bm.beagle.Beagle(2, 6, 2, 70, 8, 1, 4, 1, 0)
    with pytest.raises(bm.beagle.BeagleException) as e:
        big.nodeHeightDerivatives([[2, 0, 0, 2, 1, 1, 2, -1]], [[1.0, 1.0, 0.0]])
    assert e.value.code == -7
    big.finalize()
