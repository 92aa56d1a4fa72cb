"""Compressed evaluations cut by their remaining work (csrc/planner.h WalkPlanner::repeatWeights, csrc/engine_walk.cpp walkRepeatChunkOps,
DESIGN.md 4.1): a list whose plain definitions will be taken from class tables is cut into slices by what is left of it in the walk, not
by its length.  The cut decides where slices end and nothing else: with BEAGLE_MI355_NO_REPEAT_SLICING=1 — the cut of the uncompressed
list — every pattern goes through the same arithmetic.

Shapes (taxa, patterns, categories): (48, 129, 1), (48, 300, 4), (96, 1000, 4) — one to eight pattern groups, no multiple of 128,
partials buffers of 4 KB to 128 KB (BEAGLE_MI355_REPEATS_ANY_SIZE=1 for the whole module: the engine leaves compression off at these
sizes), ~1 % missing states.  48 and 96 taxa are the smallest lists the cut by length divides at all (from 32 operations, slices of 24
micro-operations at least): below that the two cuts are the same one walk.  The class limit is half the patterns, as in
tests/test_gpu_repeats.py, so that most plain definitions are compressed.

Each shape runs the chain of tests/test_gpu_repeats.py (the write-mode first evaluation, read mode on both buffer flips, a model move, an
accepted and a rejected branch move, a full evaluation on a new list, new tip states, uploaded tip partials) once per cut:
  * with BEAGLE_MI355_NO_SCALE_FOLD=1 and BEAGLE_MI355_NO_SLICE_SUMS=1 lnL, site values and every node's partials are bit-identical;
  * with defaults they agree to 1e-12 relative;
  * either cut is within 1e-10 of the CPU oracle (REL_TOL of tests/test_gpu_parity.py);
  * the same on the C++ kernel (BEAGLE_MI355_NO_FAST_WALK=1), where the new cut does not apply;
  * every shape compresses clades under both cuts, and at 96 taxa the two cuts launch different numbers of slices."""
import os

import numpy as np
import pytest

import beast_mcmc_amd as bm
import helpers
from beast_mcmc_amd.treelikelihood import BeagleTreeLikelihood, RESCALE_DYNAMIC

pytestmark = pytest.mark.gpu
NONE = bm.beagle.NONE
REL_TOL = 1e-10          # tests/test_gpu_parity.py REL_TOL
CUT_TOL = 1e-12          # the two cuts against each other, defaults
SWITCHES = ("BEAGLE_MI355_REPEATS_ANY_SIZE", "BEAGLE_MI355_NO_REPEAT_SLICING", "BEAGLE_MI355_REPEAT_MAX_FRAC", "BEAGLE_MI355_NO_SCALE_FOLD",
            "BEAGLE_MI355_NO_FAST_WALK", "BEAGLE_MI355_NO_SLICE_SUMS", "BEAGLE_MI355_MEM_DEF_STEPS")
SHAPES = [(48, 129, 1), (48, 300, 4), (96, 1000, 4)]
PARENT = {"BEAGLE_MI355_NO_REPEAT_SLICING": "1"}
STRICT = {"BEAGLE_MI355_NO_SCALE_FOLD": "1", "BEAGLE_MI355_NO_SLICE_SUMS": "1"}
SLOW = {"BEAGLE_MI355_NO_FAST_WALK": "1"}
_workloads, _oracle = {}, {}


def workload(T, P, C):
    if (T, P, C) not in _workloads:
        wl = helpers.random_workload(T, P, 4, C, seed=300 + T + P, unknown_fraction=0.01, root_to_tip=0.15)
        rng = np.random.default_rng(5)
        _workloads[(T, P, C)] = (wl, rng.integers(0, 5, size=P).astype(np.int32), rng.uniform(0.05, 1.0, size=(P, 4)))
    return _workloads[(T, P, C)]


def chain(tl, wl, new_states, tip_partials, counters):
    """Returns (lnLs, site values, {node: partials}, slices of the walk behind every evaluation, class-table counters of the steady state)."""
    raw = helpers.raw_binding(tl)
    tree, rng = wl.tree, np.random.default_rng(8)
    models = [tl.model_handle(wl.eig, wl.freqs, wl.cat_rates * f, wl.cat_weights) for f in (1.0, 1.1)]
    lnl, slices, sites = [], [], []

    def evaluate():
        lnl.append(tl.getLogLikelihood())
        if counters:
            slices.append(raw.walkLaunchInfo()["slices"])
    if counters:
        raw.kernelTimer(True)
    evaluate()                                           # write mode (DYNAMIC): not compressed, cut by its length
    for k in range(3):                                   # read mode, both buffer flips
        tl.makeDirty()
        evaluate()
    tl.storeState(); tl.apply_model(models[1]); evaluate()          # a model move
    steady = raw.walkStats() if counters else None
    for move in range(2):                                # a branch move, accepted; another, rejected
        node = int(rng.integers(wl.tip_count, wl.tree.node_count))
        tl.storeState()
        tl.set_node_height(node, helpers.proposed_height(tree, node, rng))
        evaluate()
        if move == 1:
            tl.restoreState()
            tl.restore_node_height(node, float(tree.height[node]))
            evaluate()
    tl.storeState(); tl.apply_model(models[0]); evaluate()          # a full evaluation on a list not seen before
    sites.append(tl.getSiteLogLikelihoods().copy())
    raw.setTipStates(3, new_states)                      # new tip states: indices and tables are rebuilt
    tl.makeDirty(); evaluate()
    tl.makeDirty(); evaluate()
    sites.append(tl.getSiteLogLikelihoods().copy())
    raw.setTipPartials(5, tip_partials)                  # uploaded partials for a tip: such a list is no closed list of compact tips
    tl.makeDirty(); evaluate()
    sites.append(tl.getSiteLogLikelihoods().copy())
    partials = {n: raw.getPartials(tl.node_buffer_index(n), NONE).copy() for n in range(wl.tip_count, wl.tree.node_count)}
    return lnl, sites, partials, slices, steady


def run(shape, env, library=None):
    wl, new_states, tip_partials = workload(*shape)
    for k in SWITCHES:
        os.environ.pop(k, None)
    # (read at instance creation; memory definitions are off at these sizes too: BEAGLE_MI355_MEM_DEF_STEPS turns them on)
    os.environ.update(dict(env, BEAGLE_MI355_REPEATS_ANY_SIZE="1", BEAGLE_MI355_MEM_DEF_STEPS="8", BEAGLE_MI355_REPEAT_MAX_FRAC="1/2"))
    try:
        tl = BeagleTreeLikelihood(wl, rescaling=RESCALE_DYNAMIC, delay_rescaling=False, **({"library": library} if library else {}))
        out = chain(tl, wl, new_states, tip_partials, counters=library is None)
        tl.close()
        return out
    finally:
        for k in SWITCHES:
            os.environ.pop(k, None)


def oracle(shape, oracle_lib):
    if shape not in _oracle:
        _oracle[shape] = run(shape, {}, library=oracle_lib)
    return _oracle[shape]


def same_bits(a, b, what):
    assert a[0] == b[0], (what, a[0], b[0])
    for x, y in zip(a[1], b[1]):
        assert np.array_equal(x, y), what
    for n in a[2]:
        assert np.array_equal(a[2][n], b[2][n]), (what, n)


def worst(a, b):
    """Largest relative difference of lnL, site values and partials (a node's partials relative to the pattern's largest entry)."""
    w = max(helpers.rel_err(x, y) for x, y in zip(a[0], b[0]))
    for x, y in zip(a[1], b[1]):
        w = max(w, float(np.max(np.abs(x - y) / np.maximum(np.abs(y), 1e-300))))
    for n in b[2]:
        scale = np.maximum(np.abs(b[2][n]).max(axis=(0, 2), keepdims=True), 1e-300)
        w = max(w, float(np.max(np.abs(a[2][n] - b[2][n]) / scale)))
    return w


@pytest.mark.parametrize("kernel", ["assembly", "c++"])
@pytest.mark.parametrize("shape", SHAPES)
def test_the_cut_changes_no_value(shape, kernel, oracle_lib):
    base = SLOW if kernel == "c++" else {}
    ref = oracle(shape, oracle_lib)
    strict_new, strict_old = run(shape, dict(base, **STRICT)), run(shape, dict(base, **STRICT, **PARENT))
    same_bits(strict_new, strict_old, "per-node factors, no slice sums")
    new, old = run(shape, base), run(shape, dict(base, **PARENT))
    between = worst(new, old)
    to_oracle = {name: worst(r, ref) for name, r in (("new", new), ("old", old), ("strict new", strict_new), ("strict old", strict_old))}
    print("%s %s: slices per evaluation new %s, old %s; steady-state clades new %d, old %d; the two cuts differ by %.3g; against the oracle %s"
          % (shape, kernel, new[3], old[3], new[4]["repeat_clades"], old[4]["repeat_clades"], between, to_oracle))
    assert len(new[0]) == len(ref[0]) and all(np.isfinite(x) for x in ref[0])
    assert between <= CUT_TOL
    for name, err in to_oracle.items():
        assert err <= REL_TOL, name
    # both cuts compress: four evaluations of the steady bracket read class tables, at least one clade each
    for r in (new, old):
        assert r[4]["repeat_clades"] >= 4 and r[4]["table_reads"] >= 4
    # the write-mode first evaluation and the list with uploaded tip partials are cut by their length under either switch
    assert new[3][0] == old[3][0] and new[3][-1] == old[3][-1]
    if kernel == "assembly" and shape[0] == 96:
        # the read-mode evaluations really ran as another number of slices (evaluations 1 .. 3: read mode on both buffer flips)
        assert all(s > 0 for s in new[3][1:4] + old[3][1:4])
        assert new[3][1:4] != old[3][1:4] and sum(new[3][1:4]) < sum(old[3][1:4])
    if kernel == "c++":
        assert new[3] == old[3]                          # (no one-launch walk there: the cut is the uncompressed list's)
