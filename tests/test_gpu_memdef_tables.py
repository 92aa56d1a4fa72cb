"""Class tables for the plain clades INSIDE memory definitions (beast-mcmc_amd/csrc/planner.h RepeatRun sub-runs, WalkPlanner::memDefTables;
DESIGN.md 4.1 "Tables inside memory definitions").  A memory definition that is evaluated from memory — a slice above the one that stored
its operand — used to stay in the walk at full width with every clade of tips hanging off its path; now each such clade is evaluated once
per distinct sub-pattern like any other, and a list that will be compressed is cut by what that leaves.  Nothing changes in what is
computed: lnL, site values and every node's partials must be BIT-IDENTICAL to BEAGLE_MI355_NO_MEMDEF_TABLES=1 (the behaviour before) and to
BEAGLE_MI355_NO_REPEATS=1, bit-identical to the C++ kernel (BEAGLE_MI355_NO_FAST_WALK=1) with BEAGLE_MI355_NO_SLICE_SUMS=1 on both sides —
the way tests/test_gpu_walk_kernels.py and tests/test_gpu_table_row_ids.py set the two kernels against each other —, and agree with the CPU
oracle at tests/test_gpu_parity.py's bound (1e-10 relative).

Shapes (tips x patterns x categories): 48 x 129 x 1, 96 x 300 x 4 and 200 x 1000 x 4 with BEAGLE_MI355_REPEATS_ANY_SIZE=1 and
BEAGLE_MI355_MEM_DEF_STEPS=8 (the engine leaves both features off at these buffer sizes; a definition of eight steps holds "stored operand
over a clade of three tips"), and 400 x 16 385 x 4 — a buffer just over 2 MiB — at the shipped constants with nothing set, evaluated often
enough for its lists to come a second time and be planned under the longer cap.  Every node's partials are compared at the small shapes,
every fifth node's at the large one (2 MiB each), as tests/test_gpu_memdef_first_read.py does.

The workloads are seeded (SEEDS below: helpers.random_workload's seed, root-to-tip distance and kind of tree) and chosen so that EVERY case takes at least
one sub-run — a condition of the test, read from the engine's counter (beagleMi355RepeatSubRunStats), not a result."""
import os

import numpy as np
import pytest

import beast_mcmc_amd as bm
import helpers
from beast_mcmc_amd.treelikelihood import BeagleTreeLikelihood, RESCALE_DYNAMIC

pytestmark = pytest.mark.gpu
NONE = bm.beagle.NONE
REL_TOL = 1e-10          # tests/test_gpu_parity.py REL_TOL
SWITCHES = ("BEAGLE_MI355_REPEATS_ANY_SIZE", "BEAGLE_MI355_NO_REPEATS", "BEAGLE_MI355_NO_MEMDEF_TABLES", "BEAGLE_MI355_NO_FAST_WALK",
            "BEAGLE_MI355_MEM_DEF_STEPS", "BEAGLE_MI355_MEM_DEF_SEEN_STEPS", "BEAGLE_MI355_NO_SLICE_SUMS")
SMALL = [(48, 129, 1), (96, 300, 4), (200, 1000, 4)]
SHIPPED = (400, 16385, 4)
SHAPES = SMALL + [SHIPPED]
# shape -> (seed of helpers.random_workload, root-to-tip distance, kind of tree): see the module docstring.  (At the large shape a coalescent
# tree compresses to less than a slice and a half of the walk and is not cut at all — no definition is read from memory; a Yule tree is.)
SEEDS = {(48, 129, 1): (503, 0.15, "coalescent"), (96, 300, 4): (502, 0.15, "coalescent"), (200, 1000, 4): (506, 0.15, "coalescent"),
         SHIPPED: (550, 0.5, "yule")}
_workloads, _runs = {}, {}


def workload(shape):
    if shape not in _workloads:
        seed, depth, kind = SEEDS[shape]
        _workloads[shape] = helpers.random_workload(shape[0], shape[1], 4, shape[2], seed=seed, unknown_fraction=0.01, root_to_tip=depth,
                                                    tree_kind=kind)
    return _workloads[shape]


def sample(wl):
    return list(range(wl.tip_count, wl.tree.node_count, 1 if wl.pattern_count < 4096 else 5))


def counters(raw):
    s = dict(raw.walkStats(), **raw.repeatStats())
    s.update(raw.repeatSubRunStats())
    return s


def evaluate(tl, wl, count):
    """A first (write-mode) evaluation and three read-mode ones, on both buffer flips — the third list is the first one come again: planned
    under the longer cap where there are two —, then a model move.  Returns (lnLs, [site values], {node: partials}, counters)."""
    raw = helpers.raw_binding(tl)
    if count:
        raw.kernelTimer(True)
    other = tl.model_handle(wl.eig, wl.freqs, wl.cat_rates * 1.1, wl.cat_weights)
    lnl = [tl.getLogLikelihood()]
    for k in range(3):
        tl.makeDirty()
        lnl.append(tl.getLogLikelihood())
    tl.storeState(); tl.apply_model(other); lnl.append(tl.getLogLikelihood())
    sites = [tl.getSiteLogLikelihoods().copy()]
    stats = counters(raw) if count else {}
    partials = {n: raw.getPartials(tl.node_buffer_index(n), NONE).copy() for n in sample(wl)}
    return lnl, sites, partials, stats


def chain(tl, wl, count):
    """Model moves — two closed lists in alternation, which come again and are planned under the longer cap —, a branch move that is accepted
    (its full evaluation is a new list: the short cap again), one that is rejected, and model moves again, one of them rejected."""
    raw = helpers.raw_binding(tl)
    if count:
        raw.kernelTimer(True)
    tree, rng = wl.tree, np.random.default_rng(23)
    models = [tl.model_handle(wl.eig, wl.freqs, wl.cat_rates * f, wl.cat_weights) for f in (1.0, 1.1)]
    lnl, sites = [tl.getLogLikelihood()], []
    for k in range(4):
        tl.storeState(); tl.apply_model(models[(k + 1) % 2]); lnl.append(tl.getLogLikelihood())
    sites.append(tl.getSiteLogLikelihoods().copy())
    for move in range(2):                                # a branch move accepted, one rejected
        node = int(rng.integers(wl.tip_count, tree.node_count - 1))
        tl.storeState()
        tl.set_node_height(node, helpers.proposed_height(tree, node, rng))
        lnl.append(tl.getLogLikelihood())
        if move == 1:
            tl.restoreState()
            tl.restore_node_height(node, float(tree.height[node]))
            lnl.append(tl.getLogLikelihood())
    for k in range(4):
        tl.storeState(); tl.apply_model(models[(k + 1) % 2]); lnl.append(tl.getLogLikelihood())
        if k == 1:
            tl.restoreState(); tl.apply_model(models[k % 2]); lnl.append(tl.getLogLikelihood())
    sites.append(tl.getSiteLogLikelihoods().copy())
    stats = counters(raw) if count else {}
    partials = {n: raw.getPartials(tl.node_buffer_index(n), NONE).copy() for n in sample(wl)}
    return lnl, sites, partials, stats


def run(shape, env, library=None, what=evaluate):
    key = (shape, tuple(sorted(env.items())), library, what.__name__)
    if key in _runs:
        return _runs[key]
    wl = workload(shape)
    for k in SWITCHES:
        os.environ.pop(k, None)
    # (read at instance creation; the large shape runs at the engine's own constants)
    os.environ.update(env if shape == SHIPPED else dict(env, BEAGLE_MI355_REPEATS_ANY_SIZE="1", BEAGLE_MI355_MEM_DEF_STEPS="8"))
    try:
        tl = BeagleTreeLikelihood(wl, rescaling=RESCALE_DYNAMIC, delay_rescaling=False, **({"library": library} if library else {}))
        out = what(tl, wl, library is None)
        tl.close()
    finally:
        for k in SWITCHES:
            os.environ.pop(k, None)
    _runs[key] = out
    return out


def same_bits(a, b, what):
    assert a[0] == b[0], (what, a[0], b[0])
    assert len(a[1]) == len(b[1])
    for x, y in zip(a[1], b[1]):
        assert np.array_equal(x, y), what
    for n in a[2]:
        assert np.array_equal(a[2][n], b[2][n]), (what, n)


def holds_oracle_bound(on, ref):
    assert len(on[0]) == len(ref[0])
    for a, b in zip(on[0], ref[0]):
        assert np.isfinite(b) and helpers.rel_err(a, b) <= REL_TOL, (a, b)
    for x, y in zip(on[1], ref[1]):
        assert np.max(np.abs(x - y) / np.maximum(np.abs(y), 1e-300)) <= REL_TOL
    for n in ref[2]:
        scale = np.maximum(np.abs(ref[2][n]).max(axis=(0, 2), keepdims=True), 1e-300)
        assert np.max(np.abs(on[2][n] - ref[2][n]) / scale) <= REL_TOL, n


@pytest.mark.parametrize("shape", SHAPES)
def test_sub_runs_keep_every_bit(shape, oracle_lib):
    on = run(shape, {})
    s = on[3]
    print("%s: %s" % (shape, s))
    assert s["sub_runs"] > 0 and s["sub_run_micro_ops"] >= s["sub_runs"], "no sub-run taken: the seed does not make the case"
    assert s["repeat_clades"] > s["sub_runs"] and s["walks"] > 0 and s["fast_walks"] == s["walks"]
    switch = run(shape, {"BEAGLE_MI355_NO_MEMDEF_TABLES": "1"})
    print("%s with the switch: %s" % (shape, switch[3]))
    assert switch[3]["sub_runs"] == 0 and switch[3]["table_reads"] > 0
    same_bits(on, switch, "against BEAGLE_MI355_NO_MEMDEF_TABLES=1")
    off = run(shape, {"BEAGLE_MI355_NO_REPEATS": "1"})
    assert off[3]["table_reads"] == 0 and off[3]["sub_runs"] == 0
    same_bits(on, off, "against BEAGLE_MI355_NO_REPEATS=1")
    holds_oracle_bound(on, run(shape, {}, library=oracle_lib))


@pytest.mark.parametrize("shape", SHAPES)
def test_the_cpp_kernel_reads_the_same_bits(shape):
    """Against BEAGLE_MI355_NO_FAST_WALK=1 with BEAGLE_MI355_NO_SLICE_SUMS=1 on both sides (the two kernels cut a write-mode program into
    different slices, whose per-slice sums of factors round differently: tests/test_gpu_table_row_ids.py)."""
    sums_off = {"BEAGLE_MI355_NO_SLICE_SUMS": "1"}
    on = run(shape, sums_off)
    slow = run(shape, dict(sums_off, BEAGLE_MI355_NO_FAST_WALK="1"))
    print("%s: sub-runs %d on the assembly loop, %d on the C++ kernel" % (shape, on[3]["sub_runs"], slow[3]["sub_runs"]))
    assert on[3]["sub_runs"] > 0 and on[3]["fast_walks"] == on[3]["walks"] > 0 and slow[3]["fast_walks"] == 0
    same_bits(on, slow, "against BEAGLE_MI355_NO_FAST_WALK=1")


@pytest.mark.parametrize("shape", [(200, 1000, 4), SHIPPED])
def test_a_chain_across_the_switch_of_caps(shape, oracle_lib):
    on = run(shape, {}, what=chain)
    print("%s: %s" % (shape, on[3]))
    assert on[3]["sub_runs"] > 0 and on[3]["fast_walks"] == on[3]["walks"]
    switch = run(shape, {"BEAGLE_MI355_NO_MEMDEF_TABLES": "1"}, what=chain)
    assert switch[3]["sub_runs"] == 0
    same_bits(on, switch, "the chain against BEAGLE_MI355_NO_MEMDEF_TABLES=1")
    same_bits(on, run(shape, {"BEAGLE_MI355_NO_REPEATS": "1"}, what=chain), "the chain against BEAGLE_MI355_NO_REPEATS=1")
    holds_oracle_bound(on, run(shape, {}, library=oracle_lib, what=chain))
