"""Class-table operands of the assembly walk loop read through packed class ids (kernels.h WK_TAB): a clade's row vector
holds one uint16 class id per pattern, the loop requests a lane's two ids (one dword) two stages ahead, right behind the
micro-operation's fetch, and the table blocks are left with the row loads — a first child's in the middle of the stage before, behind
that stage's wait (kernels.h walkStageWaits, tableIds; a slice's first two micro-operations load their ids where they use them).  Nothing changes in what is computed: lnL, site values and every node's partials must be
BIT-IDENTICAL to BEAGLE_MI355_NO_REPEATS=1 and to the C++ kernel (BEAGLE_MI355_NO_FAST_WALK=1, which reads the same packed format
without a prefetch; see test_the_cpp_kernel_reads_the_same_bits for how the two kernels are set against each other), and agree with the CPU oracle at tests/test_gpu_parity.py's bound (1e-10 relative).

Shapes (tips x patterns x categories): 48 x 129 x 1 (a ragged last group, one wave per workgroup), 48 x 300 x 4, 96 x 1000 x 4; DYNAMIC
and unscaled.  BEAGLE_MI355_REPEATS_ANY_SIZE=1 as in tests/test_gpu_repeats.py (the engine leaves the feature off at these buffer sizes).

The workloads are seeded (SEEDS below: helpers.random_workload's seed, the root-to-tip distance of the simulated alignment and the class
limit) and chosen so that the cases together hold every arrangement the id prefetch has to get right — asserted from the engine's counters in
test_the_cases_hold_every_arrangement, as conditions of the test, not as results:
  * a micro-operation with both children from tables (ids in both tip-state registers of a slot, the second table's address as a distance);
  * a table read under a memory definition;
  * a table first child directly behind a micro-operation whose own first child comes from memory (four loads between ids and rows);
  * a table first child directly behind a fused cherry (three more loads in the fetch in front of the ids);
  * a table with more than 256 classes (the high byte of an id)."""
import os

import numpy as np
import pytest

import beast_mcmc_amd as bm
import helpers
from beast_mcmc_amd.treelikelihood import BeagleTreeLikelihood, RESCALE_DYNAMIC, RESCALE_NONE

pytestmark = pytest.mark.gpu
NONE = bm.beagle.NONE
REL_TOL = 1e-10          # tests/test_gpu_parity.py REL_TOL, as tests/test_gpu_repeats.py
SWITCHES = ("BEAGLE_MI355_REPEATS_ANY_SIZE", "BEAGLE_MI355_NO_REPEATS", "BEAGLE_MI355_REPEAT_MAX_FRAC", "BEAGLE_MI355_NO_FAST_WALK",
            "BEAGLE_MI355_MEM_DEF_STEPS", "BEAGLE_MI355_NO_SLICE_SUMS")
SHAPES = [(48, 129, 1), (48, 300, 4), (96, 1000, 4)]
# shape -> (seed of helpers.random_workload, root-to-tip distance, the class limit as a fraction of the pattern count): see the module docstring
SEEDS = {(48, 129, 1): (412, 0.5, 0.1), (48, 300, 4): (416, 0.15, 0.04), (96, 1000, 4): (411, 3.0, 0.9)}
_workloads, _runs = {}, {}


def workload(shape):
    if shape not in _workloads:
        seed, depth, _ = SEEDS[shape]
        _workloads[shape] = helpers.random_workload(shape[0], shape[1], 4, shape[2], seed=seed, unknown_fraction=0.01, root_to_tip=depth)
    return _workloads[shape]


def frac(shape):
    return {"BEAGLE_MI355_REPEAT_MAX_FRAC": repr(SEEDS[shape][2])}


def evaluate(tl, wl, counters):
    """A first (write-mode or unscaled) evaluation, read-mode evaluations on both buffer flips, a model move.
    Returns (lnLs, [site values], {node: partials}, counters)."""
    raw = helpers.raw_binding(tl)
    if counters:
        raw.kernelTimer(True)
    other = tl.model_handle(wl.eig, wl.freqs, wl.cat_rates * 1.1, wl.cat_weights)
    lnl = [tl.getLogLikelihood()]
    for k in range(3):
        tl.makeDirty()
        lnl.append(tl.getLogLikelihood())
    tl.storeState(); tl.apply_model(other); lnl.append(tl.getLogLikelihood())
    sites = [tl.getSiteLogLikelihoods().copy()]
    stats = {}
    if counters:
        stats = dict(raw.walkStats(), **raw.repeatStats())
        stats.update(raw.tableOperandStats())
    partials = {n: raw.getPartials(tl.node_buffer_index(n), NONE).copy() for n in range(wl.tip_count, wl.tree.node_count)}
    return lnl, sites, partials, stats


def chain(tl, wl, counters):
    """Store / restore with rejected branch moves in between, two closed lists in alternation (two models), then new states for a tip
    (the indices and tables are rebuilt).  Returns what evaluate() returns, with site values at three points."""
    raw = helpers.raw_binding(tl)
    if counters:
        raw.kernelTimer(True)
    tree, rng = wl.tree, np.random.default_rng(17)
    models = [tl.model_handle(wl.eig, wl.freqs, wl.cat_rates * f, wl.cat_weights) for f in (1.0, 1.1)]
    lnl, sites = [tl.getLogLikelihood()], []
    tl.makeDirty(); lnl.append(tl.getLogLikelihood())
    for move in range(4):                                # branch moves: rejected, accepted, rejected, rejected
        node = int(rng.integers(wl.tip_count, tree.node_count))
        tl.storeState()
        tl.set_node_height(node, helpers.proposed_height(tree, node, rng))
        lnl.append(tl.getLogLikelihood())
        if move != 1:
            tl.restoreState()
            tl.restore_node_height(node, float(tree.height[node]))
            lnl.append(tl.getLogLikelihood())
    sites.append(tl.getSiteLogLikelihoods().copy())
    for k in range(6):                                   # two closed lists in alternation; every third one is rejected
        tl.storeState(); tl.apply_model(models[(k + 1) % 2]); lnl.append(tl.getLogLikelihood())
        if k % 3 == 2:
            tl.restoreState(); tl.apply_model(models[k % 2]); lnl.append(tl.getLogLikelihood())
    sites.append(tl.getSiteLogLikelihoods().copy())
    stats = {}
    if counters:
        stats["alternating"] = dict(raw.walkStats(), **raw.tableOperandStats())
        raw.kernelTimer(True)
    raw.setTipStates(3, np.random.default_rng(18).integers(0, 5, size=wl.pattern_count).astype(np.int32))
    for k in range(3):
        tl.makeDirty(); lnl.append(tl.getLogLikelihood())
    sites.append(tl.getSiteLogLikelihoods().copy())
    if counters:
        stats["after_new_states"] = dict(raw.walkStats(), **raw.tableOperandStats())
    partials = {n: raw.getPartials(tl.node_buffer_index(n), NONE).copy() for n in range(wl.tip_count, tree.node_count)}
    return lnl, sites, partials, stats


def run(shape, scheme, env, library=None, what=evaluate):
    key = (shape, scheme, tuple(sorted(env.items())), library, what.__name__)
    if key in _runs:
        return _runs[key]
    wl = workload(shape)
    for k in SWITCHES:
        os.environ.pop(k, None)
    # (read at instance creation; memory definitions are off at these sizes too: BEAGLE_MI355_MEM_DEF_STEPS turns them on)
    os.environ.update(dict(env, BEAGLE_MI355_REPEATS_ANY_SIZE="1", BEAGLE_MI355_MEM_DEF_STEPS="8"))
    try:
        tl = BeagleTreeLikelihood(wl, rescaling=scheme, delay_rescaling=False, **({"library": library} if library else {}))
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


@pytest.mark.parametrize("scheme", [RESCALE_DYNAMIC, RESCALE_NONE])
@pytest.mark.parametrize("shape", SHAPES)
def test_packed_ids_keep_every_bit(shape, scheme, oracle_lib):
    on = run(shape, scheme, frac(shape))
    s = on[3]
    print("%s scheme %d: %s" % (shape, scheme, s))
    assert s["table_reads"] > 0 and s["repeat_clades"] > 0 and s["table_first_children"] > 0
    assert s["walks"] > 0 and s["fast_walks"] == s["walks"]
    off = run(shape, scheme, {"BEAGLE_MI355_NO_REPEATS": "1"})
    assert off[3]["table_reads"] == 0 and off[3]["table_first_children"] == 0
    same_bits(on, off, "against BEAGLE_MI355_NO_REPEATS=1")
    ref = run(shape, scheme, {}, library=oracle_lib)
    assert len(on[0]) == len(ref[0])
    for a, b in zip(on[0], ref[0]):
        assert np.isfinite(b) and helpers.rel_err(a, b) <= REL_TOL, (a, b)
    for x, y in zip(on[1], ref[1]):
        assert np.max(np.abs(x - y) / np.maximum(np.abs(y), 1e-300)) <= REL_TOL
    for n in ref[2]:
        scale = np.maximum(np.abs(ref[2][n]).max(axis=(0, 2), keepdims=True), 1e-300)
        assert np.max(np.abs(on[2][n] - ref[2][n]) / scale) <= REL_TOL, n


def differences(a, b):
    """(lnLs equal, per site vector: (values that differ, largest relative difference), nodes whose partials differ)"""
    return (a[0] == b[0], [(int(np.count_nonzero(x != y)), float(np.max(np.abs(x - y) / np.abs(y)))) for x, y in zip(a[1], b[1])],
            [n for n in a[2] if not np.array_equal(a[2][n], b[2][n])])


@pytest.mark.parametrize("scheme", [RESCALE_DYNAMIC, RESCALE_NONE])
@pytest.mark.parametrize("shape", SHAPES)
def test_the_cpp_kernel_reads_the_same_bits(shape, scheme):
    """lnL, site values and every node's partials of the assembly loop against BEAGLE_MI355_NO_FAST_WALK=1, bit for bit — the two
    kernels set against each other the way tests/test_gpu_walk_kernels.py sets them: with BEAGLE_MI355_NO_SLICE_SUMS=1 on both sides.
    A DYNAMIC chain's first evaluation rescales in write mode, and by default its cumulative factors are summed from per-slice products;
    the two kernels cut a program into different slices, so that sum — nothing a class table touches — rounds differently in the last
    bit whichever kernel reads the tables, with BEAGLE_MI355_NO_REPEATS=1 as well (measured here: 37 of 129, 84 of 300, 331 of 1000 site
    values, at most 3.6e-16 relative).  tests/test_gpu_slice_sums.py holds the two kernels' slice sums to rounding; so does this test,
    at that file's bounds, for the default settings: partials bit for bit, lnL to 1e-13 and site values to 1e-12 relative — and
    everything bit for bit where nothing is rescaled."""
    sums_off = dict(frac(shape), BEAGLE_MI355_NO_SLICE_SUMS="1")
    on = run(shape, scheme, sums_off)
    slow = run(shape, scheme, dict(sums_off, BEAGLE_MI355_NO_FAST_WALK="1"))
    assert slow[3]["table_reads"] > 0 and slow[3]["fast_walks"] == 0 and on[3]["fast_walks"] == on[3]["walks"] > 0
    assert on[3]["table_reads"] == run(shape, scheme, frac(shape))[3]["table_reads"]          # the same programs as the default run's
    d0 = differences(on, slow)
    # the default settings: slice sums on
    on1 = run(shape, scheme, frac(shape))
    slow1 = run(shape, scheme, dict(frac(shape), BEAGLE_MI355_NO_FAST_WALK="1"))
    d1 = differences(on1, slow1)
    print("%s scheme %d: without slice sums %s; default settings %s" % (shape, scheme, d0, d1))
    same_bits(on, slow, "against BEAGLE_MI355_NO_FAST_WALK=1")
    assert not d1[2]
    if scheme == RESCALE_NONE:
        same_bits(on1, slow1, "against BEAGLE_MI355_NO_FAST_WALK=1, default settings")
    else:
        for a, b in zip(on1[0], slow1[0]):
            assert helpers.rel_err(a, b) <= 1e-13, (a, b)
        for x, y in zip(on1[1], slow1[1]):
            assert np.max(np.abs(x - y) / np.abs(y)) <= 1e-12


def test_the_cases_hold_every_arrangement():
    """The conditions of the module docstring, from the engine's counters over the cases of test_packed_ids_keep_every_bit."""
    total = {}
    for shape in SHAPES:
        for scheme in (RESCALE_DYNAMIC, RESCALE_NONE):
            s = run(shape, scheme, frac(shape))[3]
            for k in ("two_table_nodes", "tables_under_definitions", "behind_memory_first_child", "behind_fused_cherry"):
                total[k] = total.get(k, 0) + s[k]
            total["max_classes"] = max(total.get("max_classes", 0), s["max_classes"])
    print(total)
    assert total["two_table_nodes"] > 0
    assert total["tables_under_definitions"] > 0
    assert total["behind_memory_first_child"] > 0
    assert total["behind_fused_cherry"] > 0
    assert total["max_classes"] > 256


def test_a_chain_of_rejected_moves_alternating_lists_and_new_tip_states():
    shape = (48, 300, 4)
    on = run(shape, RESCALE_DYNAMIC, frac(shape), what=chain)
    off = run(shape, RESCALE_DYNAMIC, {"BEAGLE_MI355_NO_REPEATS": "1"}, what=chain)
    print({k: (v["table_reads"], v["table_first_children"]) for k, v in on[3].items()})
    for phase in ("alternating", "after_new_states"):
        assert on[3][phase]["table_reads"] > 0 and on[3][phase]["fast_walks"] == on[3][phase]["walks"], phase
        assert off[3][phase]["table_reads"] == 0, phase
    same_bits(on, off, "the chain against BEAGLE_MI355_NO_REPEATS=1")
