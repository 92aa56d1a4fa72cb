"""Memory definitions (csrc/planner.h memStepCap): a node over ONE stored internal node and a tip or a small clade is defined over
that stored node instead of being stored itself, and a program that produces the stored node evaluates the definition right
behind it, from registers.  BEAGLE's semantics must survive that — a buffer keeps the value its operation gave it — and so must
the values: with per-node scale factors (BEAGLE_MI355_NO_SCALE_FOLD=1) to the last bit against the same engine with
BEAGLE_MI355_NO_MEM_DEFS=1, with folded factors against the CPU oracle at the bounds tests/test_gpu_parity.py holds the same
quantities to (1e-10 relative: lnL, site values, partials per pattern relative to the pattern's largest entry).

Shapes: 4 states x 4 categories x 300 patterns (no multiple of 128: a ragged last group; a partials buffer of 38 KB, where the engine
leaves the feature off and definitions hold two steps at most — BEAGLE_MI355_MEM_DEF_STEPS forces it on), 64 tips (63 operations: the
planner cuts the program into slices), a coalescent tree and a caterpillar, whose every spine node has one stored child.

Bit-equality and the cumulative scale buffer: under ALWAYS and DYNAMIC rescaling the site values carry the cumulative buffer, which by
default is formed from the write-mode walk's per-SLICE products of factors (BEAGLE_MI355_NO_SLICE_SUMS: "agrees to
rounding, a few ulp of the cumulative value") — and fewer stored nodes cut the program into other slices.  So with
BEAGLE_MI355_NO_SCALE_FOLD=1 alone every node's partials are bit-identical under every scheme, lnL and site values are under NONE, and
under the rescaling schemes they agree to 1e-13 (measured on an MI355X: lnL equal, site values within 2.9e-16 relative); with
BEAGLE_MI355_NO_SLICE_SUMS=1 on top — the setting every bit-equality test of this suite uses — all three are bit-identical."""
import os

import numpy as np
import pytest

import beast_mcmc_amd as bm
import helpers
from beast_mcmc_amd.inputs import substmodel
from beast_mcmc_amd.treelikelihood import BeagleTreeLikelihood, RESCALE_ALWAYS, RESCALE_DYNAMIC, RESCALE_NONE

pytestmark = pytest.mark.gpu
NONE = bm.beagle.NONE
REL_TOL = 1e-10          # tests/test_gpu_parity.py REL_TOL
T, P, C = 64, 300, 4
SWITCHES = ("BEAGLE_MI355_MEM_DEF_STEPS", "BEAGLE_MI355_NO_MEM_DEFS", "BEAGLE_MI355_NO_SCALE_FOLD", "BEAGLE_MI355_NO_SLICE_SUMS")
ROUNDING = 1e-13         # tests/test_gpu_switches.py: lnL and site lnL of two paths that agree "to rounding"


@pytest.fixture(scope="module")
def workloads():
    return {kind: helpers.random_workload(T, P, 4, C, seed=41, tree_kind=kind) for kind in ("coalescent", "caterpillar")}


def sequence(tl, wl, counters=True):
    """Two full evaluations on flipped indices, three branch moves (the second rejected), then every internal node's partials — a
    memory-defined node, its stored operand and the root among them.  Returns (lnLs, site values, {node: partials}, counters)."""
    raw = helpers.raw_binding(tl)
    if counters:
        raw.kernelTimer(True)
    tree, rng = wl.tree, np.random.default_rng(8)
    lnl = [tl.getLogLikelihood()]
    tl.makeDirty()
    lnl.append(tl.getLogLikelihood())
    for move in range(3):
        node = int(rng.integers(wl.tip_count, wl.tree.node_count))
        tl.storeState()
        tl.set_node_height(node, helpers.proposed_height(tree, node, rng))
        lnl.append(tl.getLogLikelihood())
        if move == 1:
            tl.restoreState()
            tl.restore_node_height(node, float(tree.height[node]))
            lnl.append(tl.getLogLikelihood())
    sites = tl.getSiteLogLikelihoods().copy()
    stats = raw.walkStats() if counters else None
    partials = {n: raw.getPartials(tl.node_buffer_index(n), NONE).copy() for n in range(wl.tip_count, wl.tree.node_count)}
    return lnl, sites, partials, stats


def run(wl, scheme, env, library=None):
    for k in SWITCHES:
        os.environ.pop(k, None)
    os.environ.update(env)                # (read at instance creation)
    try:
        tl = BeagleTreeLikelihood(wl, rescaling=scheme, delay_rescaling=False, **({"library": library} if library else {}))
        out = sequence(tl, wl, counters=library is None)
        tl.close()
        return out
    finally:
        for k in SWITCHES:
            os.environ.pop(k, None)


@pytest.mark.parametrize("scheme", [RESCALE_NONE, RESCALE_DYNAMIC, RESCALE_ALWAYS])
@pytest.mark.parametrize("kind", ["coalescent", "caterpillar"])
def test_memory_definitions_keep_every_value(kind, scheme, workloads, oracle_lib):
    wl = workloads[kind]
    on = run(wl, scheme, {"BEAGLE_MI355_MEM_DEF_STEPS": "8", "BEAGLE_MI355_NO_SCALE_FOLD": "1"})
    off = run(wl, scheme, {"BEAGLE_MI355_NO_MEM_DEFS": "1", "BEAGLE_MI355_NO_SCALE_FOLD": "1"})
    site_diff = float(np.max(np.abs(on[1] - off[1]) / np.abs(off[1])))
    print("%s, scheme %d: stored %d with memory definitions, %d without; lnL %r / %r; site values differ by %.3g relative at most"
          % (kind, scheme, on[3]["stored"], off[3]["stored"], on[0], off[0], site_diff))
    # fewer stored nodes, everything on the assembly loop
    assert 0 < on[3]["stored"] < off[3]["stored"]
    assert on[3]["walks"] > 0 and on[3]["fast_walks"] == on[3]["walks"]
    # per-node factors: every node's partials bit for bit; the values that carry the cumulative buffer as the module docstring says
    for n in on[2]:
        assert np.array_equal(on[2][n], off[2][n]), n
    if scheme == RESCALE_NONE:
        assert on[0] == off[0] and np.array_equal(on[1], off[1])
    else:
        assert all(helpers.rel_err(a, b) <= ROUNDING for a, b in zip(on[0], off[0])) and site_diff <= ROUNDING
        per_node = {"BEAGLE_MI355_NO_SCALE_FOLD": "1", "BEAGLE_MI355_NO_SLICE_SUMS": "1"}
        on2 = run(wl, scheme, dict(per_node, BEAGLE_MI355_MEM_DEF_STEPS="8"))
        off2 = run(wl, scheme, dict(per_node, BEAGLE_MI355_NO_MEM_DEFS="1"))
        assert on2[3]["stored"] == on[3]["stored"]
        assert on2[0] == off2[0] and np.array_equal(on2[1], off2[1])
        for n in on2[2]:
            assert np.array_equal(on2[2][n], off2[2][n]), n
    # folded factors: the oracle, at the parity suite's bounds
    folded = run(wl, scheme, {"BEAGLE_MI355_MEM_DEF_STEPS": "8"})
    ref = run(wl, scheme, {}, library=oracle_lib)
    assert 0 < folded[3]["stored"] < off[3]["stored"] and folded[3]["fast_walks"] == folded[3]["walks"]
    assert len(folded[0]) == len(ref[0])
    for a, b in zip(folded[0], ref[0]):
        assert np.isfinite(b) and helpers.rel_err(a, b) <= REL_TOL, (a, b)
    assert np.max(np.abs(folded[1] - ref[1]) / np.maximum(np.abs(ref[1]), 1e-300)) <= REL_TOL
    for n in ref[2]:
        scale = np.maximum(np.abs(ref[2][n]).max(axis=(0, 2), keepdims=True), 1e-300)
        assert np.max(np.abs(folded[2][n] - ref[2][n]) / scale) <= REL_TOL, n


def test_overwritten_operand_leaves_its_reader_alone(engine_lib, oracle_lib, monkeypatch):
    """Raw calls.  Tips 0..5; 6 = (0, 1) and 7 = (6, 2) stay definitions over tips (two steps at this size), 8 = (7, 3) is stored,
    9 = (8, 4) is defined over the stored 8, 10 = (9, 5) ends the list and is stored.  Then an updatePartials on buffer 8 ALONE: buffer 9
    keeps the value its own operation gave it."""
    monkeypatch.setenv("BEAGLE_MI355_MEM_DEF_STEPS", "8")
    rng = np.random.default_rng(12)
    states = rng.integers(0, 5, size=(6, P)).astype(np.int32)
    eig = substmodel.gtr([1.0, 3.0, 0.7, 1.1, 4.0, 1.0], np.array([0.3, 0.2, 0.25, 0.25]))

    def make(lib):
        b = bm.beagle.Beagle(6, 11, 6, 4, P, 1, 12, C, 1, library=lib)
        for t in range(6):
            b.setTipStates(t, states[t])
        b.setEigenDecomposition(0, eig.evec, eig.ievc, eig.evals)
        b.setCategoryRates([0.1, 0.5, 1.0, 2.4])
        b.updateTransitionMatrices(0, list(range(12)), None, None, list(0.05 + 0.03 * np.arange(12)), 12)
        return b

    g, o = make(engine_lib), make(oracle_lib)
    try:
        g.kernelTimer(True)
        ops = [6, NONE, NONE, 0, 0, 1, 1,   7, NONE, NONE, 6, 6, 2, 2,   8, NONE, NONE, 7, 7, 3, 3,   9, NONE, NONE, 8, 8, 4, 4,   10, NONE, NONE, 9, 9, 5, 5]
        for b in (g, o):
            b.updatePartials(ops, 5, NONE)
        assert g.walkStats()["stored"] == 2                      # 8 and 10: 9 is a definition over 8
        for b in (g, o):
            b.updatePartials([8, NONE, NONE, 0, 10, 1, 11], 1, NONE)
        for x in (9, 8, 10, 7):
            a, b = g.getPartials(x, NONE), o.getPartials(x, NONE)
            scale = np.maximum(np.abs(b).max(axis=(0, 2), keepdims=True), 1e-300)
            assert np.max(np.abs(a - b) / scale) <= REL_TOL, x
        # ... and an upload over the operand of a definition made again
        for b in (g, o):
            b.updatePartials(ops, 5, NONE)
            b.setPartials(8, np.full((C, P, 4), 0.25))
        a, b = g.getPartials(9, NONE), o.getPartials(9, NONE)
        assert np.max(np.abs(a - b) / np.maximum(np.abs(b).max(axis=(0, 2), keepdims=True), 1e-300)) <= REL_TOL
    finally:
        g.finalize(); o.finalize()


def test_twenty_states_keep_every_node_stored(oracle_lib):
    """The T32 walk (16..20 states) is left as it was: the same counters and the same value with the feature asked for and switched off."""
    wl = helpers.random_workload(40, 300, 20, 4, seed=43)
    asked = run(wl, RESCALE_ALWAYS, {"BEAGLE_MI355_MEM_DEF_STEPS": "8"})
    off = run(wl, RESCALE_ALWAYS, {"BEAGLE_MI355_NO_MEM_DEFS": "1"})
    assert asked[3] == off[3] and asked[0] == off[0]
    ref = run(wl, RESCALE_ALWAYS, {}, library=oracle_lib)
    for a, b in zip(asked[0], ref[0]):
        assert helpers.rel_err(a, b) <= REL_TOL
