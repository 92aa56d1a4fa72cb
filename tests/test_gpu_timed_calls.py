"""The kernel timer (include/beagle_mi355.h beagleMi355KernelTimer) around the one-call entry points that take an event pair of their
own — node-height derivatives, node posteriors, placement scores: a timed call contributes exactly one pair, whatever the number of
chunks it runs in, the pair stands for the call's own launches, a sampled timer takes every N-th call, and a call whose list is
refused before anything runs leaves the timer's books as they were.

Not tested: an error return after the pair was taken.  None can be reached without provoking a device fault."""
import functools

import numpy as np
import pytest

import beast_mcmc_amd as bm
import helpers
import test_gpu_node_height as th
import test_gpu_node_posteriors as tn
import test_gpu_placement as tp
from beast_mcmc_amd.nodeheight import NodeHeightGradient

pytestmark = pytest.mark.gpu

T, P, C = 8, 300, 2          # 300 patterns: more than two 128-pattern workgroups, the last one ragged
STATES = [4, 20]             # the walk and the 4-state kernels; the general kernels
KINDS = ["heights", "heights_first", "posteriors", "placement"]


class Call:
    """One entry point on an evaluated instance: call() and refused() make a valid call and one whose list names a buffer out of
    range; launches() is the call's own running launch count."""

    def __init__(self, b, call, refused, launches):
        self.b, self.call, self._refused, self.launches = b, call, refused, launches

    def refused(self):
        with pytest.raises(bm.beagle.BeagleException) as e:
            self._refused()
        assert e.value.code == -5


def heights(S, second):
    wl = helpers.random_workload(T, P, S, C, seed=300 + S + T)
    g = NodeHeightGradient(wl, rates=th.clock_rates(T, 11 + T))
    g.prepare()
    rows, rates = g.node_rows()
    bad = rows.copy(); bad[1, 0] = 10 ** 6
    # one chunk of T - 1 nodes: the derivative kernel (general: its products first, another for the second derivatives) and the final sum
    per_call = 2 if S == 4 else (4 if second else 3)
    done = [0]

    def call():
        g.b.nodeHeightDerivatives(rows, rates, 0, first=True, second=second)
        done[0] += per_call

    return Call(g.b, call, lambda: g.b.nodeHeightDerivatives(bad, rates, 0, first=True, second=second), lambda: done[0])


def posteriors(S):
    g = tn.build(S, C, P, T=T)
    g.prepare()
    rows = g.rows()
    bad = rows.copy(); bad[1, 0] = 10 ** 6
    kw = dict(full=True, map=True, totals=True, categories=True)
    return Call(g.b, lambda: g.b.nodePosteriors(rows, 0, **kw), lambda: g.b.nodePosteriors(bad, 0, **kw),
                lambda: g.b.nodePosteriorStats()["launches"])


def placement(S):
    g = tp.build(S, C, P, T)
    g.prepare()
    rows = tp.candidate_list(g, 8)
    bad = rows.copy(); bad[1, 0] = 10 ** 6
    table = tp.code_table(S, np.random.default_rng(S))
    pats, codes = tp.queries(S, P, 50, 5, seed=S + P)
    return Call(g.b, lambda: g.b.placementScores(rows, pats, codes, table), lambda: g.b.placementScores(bad, pats, codes, table),
                lambda: g.b.placementStats()["launches"])


@functools.lru_cache(maxsize=None)
def evaluated(kind, S):
    """The instance after one post-order and one pre-order pass, both outside every timed window."""
    if kind == "posteriors":
        return posteriors(S)
    if kind == "placement":
        return placement(S)
    return heights(S, second=kind == "heights")


def timed(c, work, every=1):
    """-> (timed calls, ms, timed launches, the calls' own launches) of work() under kernelTimer(every)."""
    c.b.kernelTimer(every)
    c.b.kernelTimerCalls()
    before = c.launches()
    work()
    own = c.launches() - before
    calls = c.b.kernelTimerCalls()
    ms, launches = c.b.kernelTimer(0)
    print("timed calls %d, %.4f ms, launches %d, the calls' own %d" % (calls, ms, launches, own))
    return calls, ms, launches, own


@pytest.mark.parametrize("S", STATES)
@pytest.mark.parametrize("kind", KINDS)
def test_one_call_one_pair_with_its_own_launches(kind, S):
    c = evaluated(kind, S)
    calls, ms, launches, own = timed(c, c.call)
    assert calls == 1 and ms > 0 and own > 0 and launches == own


@pytest.mark.parametrize("S", STATES)
@pytest.mark.parametrize("kind,env", [("posteriors", {"BEAGLE_MI355_NODE_POSTERIOR_CHUNK": "2"}),
                                      ("placement", {"BEAGLE_MI355_PLACEMENT_CHUNK": "3", "BEAGLE_MI355_PLACEMENT_QUERY_CHUNK": "2"})])
def test_several_chunks_are_still_one_pair(kind, env, S):
    c = evaluated(kind, S)
    _, _, _, one_chunk = timed(c, c.call)
    with tp.environment(**env):
        calls, ms, launches, own = timed(c, c.call)
    assert own > one_chunk                                  # (the call did run in several chunks)
    assert calls == 1 and ms > 0 and launches == own


@pytest.mark.parametrize("S", STATES)
@pytest.mark.parametrize("kind", KINDS)
def test_a_sampled_timer_takes_every_third_call(kind, S):
    c = evaluated(kind, S)

    def six():
        for _ in range(6):
            c.call()

    calls, ms, launches, own = timed(c, six, every=3)
    assert calls == 2 and ms > 0 and own % 6 == 0 and launches == own // 3


@pytest.mark.parametrize("S", STATES)
@pytest.mark.parametrize("kind", KINDS)
def test_a_refused_list_leaves_the_books_alone(kind, S):
    c = evaluated(kind, S)

    def refused_then_valid():
        c.refused()
        c.call()

    calls, ms, launches, own = timed(c, refused_then_valid)
    assert calls == 1 and ms > 0 and own > 0 and launches == own
