"""The two caps of memory definitions and the long definitions a list only reads.

A full evaluation whose operation list has come before is planned once more under a longer cap (csrc/planner.h memStepCapSeen:
BEAGLE_MI355_MEM_DEF_SEEN_STEPS) and stores fewer nodes from then on; while full evaluations are all the engine is asked for, a NEW
closed list — the lists behind a flip of the scale buffers — gets the longer cap at once (planner.h preferSeenCap); lists seen for the
first time otherwise, partial updates among them, keep the short one (BEAGLE_MI355_MEM_DEF_STEPS).  A long definition that a list READS
without producing its stored operand — a branch move passing the node as a sibling — is given real data once, by a materialisation in
front of the move's own program, instead of being walked inside every move that passes it (csrc/engine_internal.h memDefInlineSteps,
planner.h longMemoryOperands: BEAGLE_MI355_MEM_DEF_INLINE_STEPS).

Values.  The node's value is what its definition evaluates to, step by step with per-node factors, whether a materialisation or the move's
own program runs those steps, and a double read back from memory is the double that was stored: with the same caps, lnL, site values and
the partials read back are BIT-IDENTICAL with first-read storing on (threshold below the long cap) and off (at it: never).  A change of cap
regroups the folded factors (DESIGN.md 4.1 "Values"): against the CPU oracle every lnL and site value holds tests/test_gpu_parity.py's bound.

Shapes (tips, patterns, categories).  Small: (96, 2049, 1), (96, 1000, 4) — buffers of 64 KiB to 2 MiB, where a definition
holds eight steps: the caps are set to 2 and 8, the threshold to 0 and 2; both leave a partial last pattern group.  Shipped:
(400, 16385, 4) — a buffer just over 2 MiB, where the engine's own constants act with nothing set: caps 8 and 24, threshold 8.

The chain (every call goes to the engine and to the oracle alike): ten full evaluations on alternating buffer flips, under DYNAMIC with
a rescaling frequency of six, so that write-mode evaluations and flips of the scale buffers — new lists — fall among them and among
the moves; a node-height move of every internal node below the root in turn, every second one restored — every memory-defined node is passed as
a sibling by one of them —; setTipStates of one tip; four moves; setTransitionMatrix straight into
the slot of a branch and a read-back of partials before any list has run (a definition keeps its matrix snapshots); a model move; four
moves; a model move on a list the engine has not seen; site values; partials read back right behind that full evaluation (memory-defined
nodes are materialised for it)."""
import os

import numpy as np
import pytest

import helpers
from beast_mcmc_amd.treelikelihood import BeagleTreeLikelihood, RESCALE_DYNAMIC, RESCALE_NONE

pytestmark = pytest.mark.gpu
NONE = -1
REL_TOL = 1e-10          # tests/test_gpu_parity.py REL_TOL
SMALL = [(96, 2049, 1), (96, 1000, 4)]
SHIPPED = (400, 16385, 4)
SWITCHES = ("BEAGLE_MI355_MEM_DEF_STEPS", "BEAGLE_MI355_MEM_DEF_SEEN_STEPS", "BEAGLE_MI355_MEM_DEF_INLINE_STEPS", "BEAGLE_MI355_REPEATS_ANY_SIZE",
            "BEAGLE_MI355_NO_FAST_WALK", "BEAGLE_MI355_NO_MEM_DEFS", "BEAGLE_MI355_WALK_SPIN_US")
TWO_CAPS = {"BEAGLE_MI355_MEM_DEF_STEPS": "2", "BEAGLE_MI355_MEM_DEF_SEEN_STEPS": "8", "BEAGLE_MI355_REPEATS_ANY_SIZE": "1"}
FULL_EVALUATIONS = 10
_workloads, _reference = {}, {}


def workload(shape):
    if shape not in _workloads:
        T, P, C = shape
        _workloads[shape] = helpers.random_workload(T, P, 4, C, seed=300 + T + P)
    return _workloads[shape]


def chain(tl, wl, scheme, counters):
    """The module docstring's chain.  Returns (lnLs, site values, {node: partials}, stored nodes of each of the ten full evaluations, stored
    nodes over the sweep of moves behind them)."""
    raw = helpers.raw_binding(tl)
    tree, rng = wl.tree, np.random.default_rng(17)
    height = np.array(tree.height, dtype=float)
    parent = {int(ch): n for n in range(wl.tip_count, tree.node_count) for ch in (tree.left[n], tree.right[n])}
    models = [tl.model_handle(wl.eig, wl.freqs, wl.cat_rates * f, wl.cat_weights) for f in (1.0, 1.1)]
    sample = list(range(wl.tip_count, tree.node_count, 1 if wl.pattern_count < 4096 else 5))
    if scheme == RESCALE_DYNAMIC:
        tl.set_rescaling_frequency(6)
    lnl, per_eval = [], []
    for k in range(FULL_EVALUATIONS):
        if counters:
            raw.kernelTimer(True)
        if k:
            tl.makeDirty()
        lnl.append(tl.getLogLikelihood())
        if counters:
            per_eval.append(raw.walkStats()["stored"])

    def moves(k, nodes=None):
        for i in range(k):
            node = nodes[i] if nodes else int(rng.integers(wl.tip_count, tree.node_count))
            while node not in parent:
                node = int(rng.integers(wl.tip_count, tree.node_count))
            lo = max(height[int(tree.left[node])], height[int(tree.right[node])])      # (accepted heights: every branch stays positive)
            h = lo + (height[parent[node]] - lo) * float(rng.uniform(0.05, 0.95))
            tl.storeState()
            tl.set_node_height(node, h)
            lnl.append(tl.getLogLikelihood())
            if i % 2:
                tl.restoreState()
                tl.restore_node_height(node, float(height[node]))
                lnl.append(tl.getLogLikelihood())
            else:
                height[node] = h
    if counters:
        raw.kernelTimer(True)
    swept = [n for n in range(wl.tip_count, tree.node_count) if n in parent]      # every node but the root: every sibling is passed
    moves(len(swept), swept)
    move_stored = raw.walkStats()["stored"] if counters else None
    raw.setTipStates(3, rng.integers(0, 5, size=wl.pattern_count).astype(np.int32))
    tl.makeDirty(); lnl.append(tl.getLogLikelihood())
    moves(4)
    # a matrix written straight into a branch's slot: nothing has run since, so every buffer still holds what its operation gave it
    raw.setTransitionMatrix(tl.node_matrix_index(5), np.tile(np.full((4, 4), 0.25), (wl.category_count, 1, 1)))
    before = {n: raw.getPartials(tl.node_buffer_index(n), NONE).copy() for n in sample[::3]}
    tl.makeDirty(); lnl.append(tl.getLogLikelihood())
    tl.storeState(); tl.apply_model(models[1]); lnl.append(tl.getLogLikelihood())
    moves(4)
    tl.storeState(); tl.apply_model(models[0]); lnl.append(tl.getLogLikelihood())
    sites = tl.getSiteLogLikelihoods().copy()
    partials = {n: raw.getPartials(tl.node_buffer_index(n), NONE).copy() for n in sample}
    partials.update({-1 - n: v for n, v in before.items()})
    return lnl, sites, partials, per_eval, move_stored


def run(shape, scheme, env, library=None):
    wl = workload(shape)
    for k in SWITCHES:
        os.environ.pop(k, None)
    os.environ.update(env)                # (read at instance creation)
    try:
        tl = BeagleTreeLikelihood(wl, rescaling=scheme, delay_rescaling=False, **({"library": library} if library else {}))
        out = chain(tl, wl, scheme, counters=library is None)
        tl.close()
        return out
    finally:
        for k in SWITCHES:
            os.environ.pop(k, None)


def oracle(shape, scheme, oracle_lib):
    if (shape, scheme) not in _reference:
        _reference[(shape, scheme)] = run(shape, scheme, {}, library=oracle_lib)
    return _reference[(shape, scheme)]


def same_bits(a, b, what):
    assert a[0] == b[0], (what, a[0], b[0])
    assert np.array_equal(a[1], b[1]), what
    for n in a[2]:
        assert np.array_equal(a[2][n], b[2][n]), (what, n)


def holds_oracle_bounds(a, ref):
    assert len(a[0]) == len(ref[0])
    for x, y in zip(a[0], ref[0]):
        assert np.isfinite(y) and helpers.rel_err(x, y) <= REL_TOL, (x, y)
    assert np.max(np.abs(a[1] - ref[1]) / np.maximum(np.abs(ref[1]), 1e-300)) <= REL_TOL
    for n in ref[2]:
        scale = np.maximum(np.abs(ref[2][n]).max(axis=(0, 2), keepdims=True), 1e-300)
        assert np.max(np.abs(a[2][n] - ref[2][n]) / scale) <= REL_TOL, n


def ran_as_meant(on, never, off, what):
    """Definitions were made, lists that came again were planned under the long cap — the new lists among them at once —, and long
    definitions were stored when a move first read them."""
    print("%s: stored per full evaluation %s (no memory definitions: %s); over the sweep of moves %d, never storing on a first read %d"
          % (what, on[3], off[3] if off else "-", on[4], never[4]))
    short, long_ = on[3][0], on[3][-1]
    assert long_ < short                                  # the first evaluation's list is new: short cap; the last one's has come before
    # evaluations 5 to 10: every list has come before or is new in a run of full evaluations — none is planned under the short cap
    assert max(on[3][4:]) < short
    assert on[4] > never[4]                               # a definition stored on its first read is a store more
    assert on[3] == never[3]                              # (the threshold acts on lists that read from outside only)
    if off:
        assert off[3][-1] > long_ and off[3][0] >= short


@pytest.mark.parametrize("kernel", ["fast", "cpp"])
@pytest.mark.parametrize("scheme", [RESCALE_NONE, RESCALE_DYNAMIC])
@pytest.mark.parametrize("shape", SMALL)
def test_first_read_storing_keeps_every_bit(shape, scheme, kernel, oracle_lib):
    env = dict(TWO_CAPS, **({"BEAGLE_MI355_NO_FAST_WALK": "1"} if kernel == "cpp" else {}))
    never = run(shape, scheme, dict(env, BEAGLE_MI355_MEM_DEF_INLINE_STEPS="8"))
    ref = oracle(shape, scheme, oracle_lib)
    off = run(shape, scheme, dict(env, BEAGLE_MI355_NO_MEM_DEFS="1")) if kernel == "fast" else None
    for threshold in ("0", "2"):
        on = run(shape, scheme, dict(env, BEAGLE_MI355_MEM_DEF_INLINE_STEPS=threshold))
        ran_as_meant(on, never, off, "%s scheme %d %s threshold %s" % (shape, scheme, kernel, threshold))
        same_bits(on, never, threshold)
        holds_oracle_bounds(on, ref)


def test_shipped_caps_and_threshold(oracle_lib):
    """Nothing set: a buffer over 2 MiB gets the caps 8 and 24 and the threshold 8.  Against the threshold at the long cap (never), against
    memory definitions off, against the oracle; and the same bits with the walk's wait for other slices cut to nothing
    (BEAGLE_MI355_WALK_SPIN_US=0: every workgroup computes what it would wait for)."""
    never = run(SHIPPED, RESCALE_DYNAMIC, {"BEAGLE_MI355_MEM_DEF_INLINE_STEPS": "24"})
    on = run(SHIPPED, RESCALE_DYNAMIC, {})
    off = run(SHIPPED, RESCALE_DYNAMIC, {"BEAGLE_MI355_NO_MEM_DEFS": "1"})
    ran_as_meant(on, never, off, "%s shipped" % (SHIPPED,))
    same_bits(on, never, "shipped")
    holds_oracle_bounds(on, oracle(SHIPPED, RESCALE_DYNAMIC, oracle_lib))
    same_bits(run(SHIPPED, RESCALE_DYNAMIC, {"BEAGLE_MI355_WALK_SPIN_US": "0"}), on, "no waiting")


def test_one_cap_everywhere_when_only_the_first_is_set():
    """BEAGLE_MI355_MEM_DEF_STEPS alone is one cap for every list (the sweeps of profiles/): no list is planned twice."""
    one = run(SMALL[1], RESCALE_NONE, {"BEAGLE_MI355_MEM_DEF_STEPS": "8", "BEAGLE_MI355_REPEATS_ANY_SIZE": "1"})
    assert len(set(one[3])) == 1, one[3]
