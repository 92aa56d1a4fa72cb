"""Repeated sub-patterns (csrc/planner.h RepeatIndex): a cached read-mode (or unscaled) full evaluation evaluates a clade
of compact tips that it would evaluate inside its consumer's program ONCE PER DISTINCT SUB-PATTERN — class-table programs in a launch in
front of the walk — and the consumer reads the pattern's class row (kernels.h WK_TAB).  Every pattern goes through the arithmetic it
went through, on the same matrices and folded reciprocals, so everything must be BIT-IDENTICAL to BEAGLE_MI355_NO_REPEATS=1: lnL, site
values and every node's partials, with folded factors and with BEAGLE_MI355_NO_SCALE_FOLD=1, on the assembly loop and on the C++
kernel (BEAGLE_MI355_NO_FAST_WALK=1); and agree with the CPU oracle at tests/test_gpu_parity.py's bound (1e-10 relative).

Shapes: 24 and 48 taxa; (patterns, categories) = (129, 1), (300, 4), (1000, 4) — no multiple of 128, one to eight pattern groups,
partials buffers of 4 KB to 128 KB, where the engine leaves the feature off: BEAGLE_MI355_REPEATS_ANY_SIZE=1 is set for the whole
module —; ~1 % missing states.  At 129 x 1 definitions hold two steps (many nodes over TWO table clades), at 1000 x 4 eight (clades of up to
nine tips, hundreds of classes: more than one 128-row group per class-table program).  The class limit is BEAGLE_MI355_REPEAT_MAX_FRAC.

The chain: a DYNAMIC (or unscaled) chain across its write-mode first evaluation (not compressed: write mode), read-mode evaluations on
both buffer flips, a model move, an accepted branch move, a rejected one (restore), new tip states for one tip (the indices are
rebuilt), partials uploaded for a tip inside a would-be clade (it must not be compressed: such a list is not compressed at all)."""
import os

import numpy as np
import pytest

import beast_mcmc_amd as bm
import helpers
from beast_mcmc_amd.treelikelihood import BeagleTreeLikelihood, RESCALE_DYNAMIC, RESCALE_NONE

pytestmark = pytest.mark.gpu
NONE = bm.beagle.NONE
REL_TOL = 1e-10          # tests/test_gpu_parity.py REL_TOL
SWITCHES = ("BEAGLE_MI355_REPEATS_ANY_SIZE", "BEAGLE_MI355_NO_REPEATS", "BEAGLE_MI355_REPEAT_MAX_FRAC", "BEAGLE_MI355_NO_SCALE_FOLD",
            "BEAGLE_MI355_NO_FAST_WALK", "BEAGLE_MI355_NO_SLICE_SUMS", "BEAGLE_MI355_MEM_DEF_STEPS", "BEAGLE_MI355_REPEAT_CAPACITY")
SHAPES = [(24, 129, 1), (24, 300, 4), (48, 1000, 4), (48, 129, 1)]
_cache = {}


def workload(T, P, C):
    """Seeded.  Two cherries with disjoint surroundings — the lowest ancestor with at least as many tips as a definition can hold (ten where
    a partials buffer is 64 KiB or more: definitions of eight steps; four below: two steps).  Every tip of the first surrounding is
    constant: whatever definition holds that cherry is a clade with ONE class.  In the second only the cherry's two tips vary, uniformly
    at random: whatever definition holds it has exactly the classes of the cherry (counted by classes() below)."""
    if (T, P, C) not in _cache:
        wl = helpers.random_workload(T, P, 4, C, seed=100 + T + P, unknown_fraction=0.01, root_to_tip=0.15)
        tree, rng = wl.tree, np.random.default_rng(3)
        cherries = [n for n in range(tree.tip_count, tree.node_count) if int(tree.left[n]) < tree.tip_count and int(tree.right[n]) < tree.tip_count]
        parent = {int(ch): n for n in range(tree.tip_count, tree.node_count) for ch in (tree.left[n], tree.right[n])}
        reach = 10 if C * P * 32 >= (64 << 10) else 4

        def below(n):
            return [n] if n < tree.tip_count else below(int(tree.left[n])) + below(int(tree.right[n]))

        def surroundings(cherry):
            x = cherry
            while len(below(x)) < reach and x in parent:
                x = parent[x]
            return set(below(x))
        first = cherries[0]
        second = [ch for ch in cherries[1:] if not (surroundings(ch) & surroundings(first))][-1]
        a, b = int(tree.left[first]), int(tree.right[first])
        c, d = int(tree.left[second]), int(tree.right[second])
        for t in surroundings(first) | surroundings(second):
            wl.tip_states[t, :] = t % 4
        wl.tip_states[c, :] = rng.integers(0, 5, size=P)
        wl.tip_states[d, :] = rng.integers(0, 5, size=P)
        _cache[(T, P, C)] = (wl, (a, b), (c, d))
    return _cache[(T, P, C)]


def chain(tl, wl, special, new_states, tip_partials, counters=True):
    """The module docstring's chain.  Returns (lnLs, site values, {node: partials}, stats per phase)."""
    raw = helpers.raw_binding(tl)
    if counters:
        raw.kernelTimer(True)
    tree, rng = wl.tree, np.random.default_rng(8)
    models = [tl.model_handle(wl.eig, wl.freqs, wl.cat_rates * f, wl.cat_weights) for f in (1.0, 1.1)]
    lnl, stats = [tl.getLogLikelihood()], {}
    for k in range(3):                                   # read mode, both buffer flips
        tl.makeDirty()
        lnl.append(tl.getLogLikelihood())
    tl.storeState(); tl.apply_model(models[1]); lnl.append(tl.getLogLikelihood())          # a model move
    if counters:
        stats["steady"] = raw.walkStats()
        stats["steady_consumers"] = raw.repeatStats()
    for move in range(2):                                # a branch move, accepted; another, rejected
        node = int(rng.integers(wl.tip_count, wl.tree.node_count))
        tl.storeState()
        tl.set_node_height(node, helpers.proposed_height(tree, node, rng))
        lnl.append(tl.getLogLikelihood())
        if move == 1:
            tl.restoreState()
            tl.restore_node_height(node, float(tree.height[node]))
            lnl.append(tl.getLogLikelihood())
    tl.storeState(); tl.apply_model(models[0]); lnl.append(tl.getLogLikelihood())          # a full evaluation on a list not seen before
    sites = [tl.getSiteLogLikelihoods().copy()]
    raw.setTipStates(special[1], new_states)             # new data for a tip of the one-class cherry: the indices are rebuilt
    tl.makeDirty(); lnl.append(tl.getLogLikelihood())
    tl.makeDirty(); lnl.append(tl.getLogLikelihood())
    sites.append(tl.getSiteLogLikelihoods().copy())
    if counters:
        raw.kernelTimer(True)
    tl.makeDirty(); lnl.append(tl.getLogLikelihood())
    if counters:
        stats["after_new_states"] = raw.walkStats()
    raw.setTipPartials(special[0], tip_partials)         # the cherry's other tip holds uploaded partials: no table for that clade
    tl.makeDirty(); lnl.append(tl.getLogLikelihood())
    if counters:
        raw.kernelTimer(True)
    tl.makeDirty(); lnl.append(tl.getLogLikelihood())
    sites.append(tl.getSiteLogLikelihoods().copy())
    if counters:
        stats["with_tip_partials"] = raw.walkStats()
        stats["end"] = raw.repeatStats()
    partials = {n: raw.getPartials(tl.node_buffer_index(n), NONE).copy() for n in range(wl.tip_count, wl.tree.node_count)}
    return lnl, sites, partials, stats


def run(shape, scheme, env, library=None):
    wl, special, _ = workload(*shape)
    rng = np.random.default_rng(5)
    new_states = rng.integers(0, 5, size=wl.pattern_count).astype(np.int32)
    tip_partials = rng.uniform(0.05, 1.0, size=(wl.pattern_count, 4))
    for k in SWITCHES:
        os.environ.pop(k, None)
    # (read at instance creation; memory definitions are off at these sizes too: BEAGLE_MI355_MEM_DEF_STEPS turns them on)
    os.environ.update(dict(env, BEAGLE_MI355_REPEATS_ANY_SIZE="1", BEAGLE_MI355_MEM_DEF_STEPS="8"))
    try:
        tl = BeagleTreeLikelihood(wl, rescaling=scheme, delay_rescaling=False, **({"library": library} if library else {}))
        out = chain(tl, wl, special, new_states, tip_partials, counters=library is None)
        tl.close()
        return out
    finally:
        for k in SWITCHES:
            os.environ.pop(k, None)


def same_bits(a, b, what):
    assert a[0] == b[0], (what, a[0], b[0])
    for x, y in zip(a[1], b[1]):
        assert np.array_equal(x, y), what
    for n in a[2]:
        assert np.array_equal(a[2][n], b[2][n]), (what, n)


@pytest.mark.parametrize("scheme", [RESCALE_NONE, RESCALE_DYNAMIC])
@pytest.mark.parametrize("shape", SHAPES)
def test_class_tables_keep_every_bit(shape, scheme, oracle_lib):
    frac = {"BEAGLE_MI355_REPEAT_MAX_FRAC": "1/2"}
    on = run(shape, scheme, frac)
    off = run(shape, scheme, {"BEAGLE_MI355_NO_REPEATS": "1"})
    s_on, s_off = on[3], off[3]
    print("%s scheme %d: steady %s; after new tip states %s; with tip partials %s" % (shape, scheme, s_on["steady"], s_on["after_new_states"], s_on["with_tip_partials"]))
    # the feature ran where it is expected to, on the assembly loop, and not at all with the switch off
    for phase in ("steady", "after_new_states"):
        assert s_on[phase]["table_reads"] > 0 and s_on[phase]["repeat_clades"] > 0 and s_on[phase]["table_rows"] > 0, phase
        assert s_off[phase]["table_reads"] == 0 and s_off[phase]["repeat_clades"] == 0 and s_off[phase]["table_rows"] == 0, phase
        assert s_on[phase]["walks"] > 0 and s_on[phase]["fast_walks"] == s_on[phase]["walks"], phase
        assert s_on[phase]["walks"] == s_off[phase]["walks"] and s_on[phase]["stored"] == s_off[phase]["stored"], phase
        assert s_on[phase]["micro_ops"] < s_off[phase]["micro_ops"], phase
    # a tip with uploaded partials inside a would-be clade: nothing that holds it is taken from a table — the list is no closed list of
    # compact tips any more, so its plan is not a cached one and nothing of it is compressed
    assert s_on["with_tip_partials"]["table_reads"] == 0 and s_on["with_tip_partials"]["repeat_clades"] == 0
    assert s_on["with_tip_partials"]["micro_ops"] == s_off["with_tip_partials"]["micro_ops"]
    same_bits(on, off, "folded factors")
    # per-node factors
    # (without a fold every read-mode micro-operation pays for itself, so under DYNAMIC no run qualifies: nothing is compressed there and
    # the comparison says only that the switch changes nothing; the unscaled scheme compresses as with folding)
    per_node = run(shape, scheme, dict(frac, BEAGLE_MI355_NO_SCALE_FOLD="1"))
    if scheme == RESCALE_NONE:
        assert per_node[3]["steady"]["table_reads"] == s_on["steady"]["table_reads"] > 0
    else:
        assert per_node[3]["steady"]["table_reads"] == 0
    same_bits(per_node, run(shape, scheme, {"BEAGLE_MI355_NO_REPEATS": "1", "BEAGLE_MI355_NO_SCALE_FOLD": "1"}), "per-node factors")
    # the C++ kernel reads the same tables to the same bits
    slow = run(shape, scheme, dict(frac, BEAGLE_MI355_NO_FAST_WALK="1"))
    assert slow[3]["steady"]["table_reads"] > 0 and slow[3]["steady"]["fast_walks"] == 0
    same_bits(slow, run(shape, scheme, {"BEAGLE_MI355_NO_REPEATS": "1", "BEAGLE_MI355_NO_FAST_WALK": "1"}), "k_walk4")
    # the oracle
    ref = run(shape, scheme, {}, library=oracle_lib)
    assert len(on[0]) == len(ref[0])
    for a, b in zip(on[0], ref[0]):
        assert np.isfinite(b) and helpers.rel_err(a, b) <= REL_TOL, (a, b)
    for x, y in zip(on[1], ref[1]):
        assert np.max(np.abs(x - y) / np.maximum(np.abs(y), 1e-300)) <= REL_TOL
    for n in ref[2]:
        scale = np.maximum(np.abs(ref[2][n]).max(axis=(0, 2), keepdims=True), 1e-300)
        assert np.max(np.abs(on[2][n] - ref[2][n]) / scale) <= REL_TOL, n


def classes(wl, tips):
    s = np.minimum(wl.tip_states[list(tips), :], 4)
    return len(np.unique(s, axis=1).T)


@pytest.mark.parametrize("shape", [(48, 1000, 4), (24, 300, 4), (48, 129, 1)])
def test_the_class_limit(shape):
    """One class, just under the class count D of the random cherry's clade, exactly D, half the patterns.  The clade with D classes has
    its table at a limit of D and none at D - 1 (through the engine's conversion of BEAGLE_MI355_REPEAT_MAX_FRAC to a class count); the
    constant clade has its table at a limit of one class; at 1000 patterns some table has more than 128 rows.  The same bits at every limit."""
    wl, (a, b), (c, d) = workload(*shape)
    P = wl.pattern_count
    D = classes(wl, (c, d))
    assert classes(wl, (a, b)) == 1 and 4 < D <= 25 < P // 2
    off = run(shape, RESCALE_DYNAMIC, {"BEAGLE_MI355_NO_REPEATS": "1"})
    seen = {}
    for limit in (1, D - 1, D, P // 2):
        on = run(shape, RESCALE_DYNAMIC, {"BEAGLE_MI355_REPEAT_MAX_FRAC": repr((limit + 0.5) / P)})
        same_bits(on, off, "limit %d" % limit)
        seen[limit] = on[3]["steady"]
    print("%s: classes of the random cherry %d; per limit %s" % (shape, D, {k: (v["repeat_clades"], v["table_rows"], v["table_reads"]) for k, v in seen.items()}))
    # the steady bracket holds four compressed evaluations (three read-mode ones and the model move's)
    assert seen[1]["repeat_clades"] >= 4
    assert seen[1]["repeat_clades"] <= seen[1]["table_rows"] <= 8 * seen[1]["repeat_clades"]          # one class: one row per micro-operation, eight of them at most
    assert seen[1]["repeat_clades"] <= seen[D - 1]["repeat_clades"] <= seen[P // 2]["repeat_clades"]
    # exactly at the limit: the clade of D classes is a table in each of the four evaluations; one class fewer allowed: it is not
    assert seen[D]["repeat_clades"] >= seen[D - 1]["repeat_clades"] + 4
    if shape[1] == 1000:
        # clades of up to nine tips under the limit of 500: some program has more than 128 class rows (two groups of a slice)
        assert seen[P // 2]["table_rows"] > 128 * seen[P // 2]["repeat_clades"]


def test_two_table_children_and_tables_under_memory_definitions():
    """The two rarer consumers of a class table occur, in programs whose values test_class_tables_keep_every_bit holds to the bit: a
    node BOTH of whose children are read from tables (one as first, one as second operand), and a step of a memory definition — a node
    defined over one stored child, not stored itself — whose other child is a table clade."""
    two, under = {}, {}
    for shape in SHAPES:
        r = run(shape, RESCALE_DYNAMIC, {"BEAGLE_MI355_REPEAT_MAX_FRAC": "1/2"})[3]["steady_consumers"]
        two[shape], under[shape] = r["two_table_nodes"], r["tables_under_definitions"]
    print("two-table nodes %s; table clades under memory definitions %s" % (two, under))
    assert two[(24, 129, 1)] > 0 and two[(48, 129, 1)] > 0          # definitions of two steps: many nodes over two of them
    assert sum(under.values()) > 0


@pytest.mark.parametrize("shape", [(48, 1000, 4), (24, 129, 1)])
def test_a_chain_across_index_resets(shape):
    """The class index keeps a bounded number of clades and drops everything past it (a long chain of topology moves gets there).  With a
    capacity of four clades every list the engine resolves after the first finds the index over its capacity: indices, tables and kept
    programs go, in the middle of the chain, and come back.  The same bits, and the chain is compressed all the same."""
    off = run(shape, RESCALE_DYNAMIC, {"BEAGLE_MI355_NO_REPEATS": "1"})
    small = run(shape, RESCALE_DYNAMIC, {"BEAGLE_MI355_REPEAT_MAX_FRAC": "1/2", "BEAGLE_MI355_REPEAT_CAPACITY": "4"})
    usual = run(shape, RESCALE_DYNAMIC, {"BEAGLE_MI355_REPEAT_MAX_FRAC": "1/2"})
    print("%s: resets %d (usual capacity %d), clades indexed %d / %d" % (shape, small[3]["end"]["index_resets"], usual[3]["end"]["index_resets"],
                                                                         small[3]["end"]["clades_indexed"], usual[3]["end"]["clades_indexed"]))
    assert small[3]["end"]["index_resets"] >= 2 and usual[3]["end"]["index_resets"] == 0
    assert small[3]["end"]["clades_indexed"] > usual[3]["end"]["clades_indexed"]
    for phase in ("steady", "after_new_states"):
        assert small[3][phase]["table_reads"] == usual[3][phase]["table_reads"] > 0, phase
    same_bits(small, off, "capacity 4")
