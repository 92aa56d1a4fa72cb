"""Chains that change the topology (tests/topology_chains.py) on the engine, its twins and the CPU oracle in lockstep.

Every other chain in this suite keeps its tree: height moves, model moves and restores on a topology joined once.  A narrow exchange or a
prune-and-regraft does what none of them does — one buffer flip of a node is defined over other children than the other flip, a restore
brings back a buffer whose definition names children the next proposal overwrites, the root becomes another node and another buffer
index, a memory definition's stored operand is rewritten from another subtree, a closed list comes that the plan cache has never seen
(and comes again), and the class index takes in the clades of two paths to the root until it reaches its capacity in the middle of the
chain.  tests/native/plan_harness.h scenarioTopology holds the planner to list-order evaluation through such chains, bitwise, on the CPU;
here the whole engine runs them.

Per (shape, seed, scheme) the same records run step by step on
  * the engine on the row's environment,
  * its twins — instances created under switches whose rows in tests/test_gpu_switches.py, or whose own tests, promise the same bits:
    BEAGLE_MI355_COPY_ENGINE_UPLOADS=1 + BEAGLE_MI355_NO_PLAN_CACHE=1 everywhere; in the compressed rows also BEAGLE_MI355_NO_REPEATS=1
    (tests/test_gpu_repeats.py) and BEAGLE_MI355_NO_MEMDEF_TABLES=1 (tests/test_gpu_memdef_tables.py); and for shape (4, 4, 96, 300) the
    assembly loop against BEAGLE_MI355_NO_FAST_WALK=1 with BEAGLE_MI355_NO_SLICE_SUMS=1 on both sides, as tests/test_gpu_memdef_tables.py
    sets the two kernels against each other,
  * the CPU oracle,
and at every step the return codes are equal, every read of the engine equals every twin's bit for bit, and is within the project's bounds
of the oracle's: lnL (every step) and site values (every fifth) 1e-10 relative, node partials (every current node buffer, unscaled, at two
seeded checkpoints and at the end — after a restore: the restored flips) within 1e-10 of each pattern's largest entry, log scale factors
(every current scale buffer and the cumulative one) 1e-10 (tests/test_gpu_parity.py REL_TOL, tests/call_sequences.py deviation).
tests/test_topology_chains_host.py measures that the oracle is within 1e-11 of its long-double mode on every read of every chain here.
One parametrisation per row takes no checkpoint reads, so that nothing is materialised for the test's sake: lnL and the end state only.

Rows (tests/test_topology_chains_host.py SHAPES; 60 proposals a chain, 28 of them topology moves; schemes NONE and DYNAMIC with
delay_rescaling off and a rescaling frequency of 7, ALWAYS on the first and last row):
  4-state walk, defaults      (4, 4, 12, 130), (4, 3, 9, 257); four seeds
  class tables + memory definitions + sub-runs   tips x patterns x categories (24, 129, 1), (48, 1000, 4), (96, 300, 4) under
                              BEAGLE_MI355_REPEATS_ANY_SIZE=1, BEAGLE_MI355_MEM_DEF_STEPS=8, BEAGLE_MI355_REPEAT_MAX_FRAC=1/2; two seeds; (24, 129, 1)
                              once more with BEAGLE_MI355_REPEAT_CAPACITY=4
  shipped constants           400 tips x 16385 patterns x 4 categories, a Yule tree, 20 proposals, lnL and every fifth node; two seeds
  T32 walk / T64 walk / general kernel / level kernels   (20, 2, 8, 33), (61, 1, 6, 37), (7, 2, 8, 67), (80, 1, 6, 23); two seeds

Route evidence (conditions, not results; counters summed over a shape's seeds and schemes): on 4 states one-launch walks ran and a root
call was answered inside the walk's launch in an evaluation whose root is not the node the chain began with; in the compressed rows
table_reads > 0 and repeat_clades > 0 in the evaluation right behind an accepted topology move, mem_reads > 0, clades_indexed grows in
those evaluations, sub_runs > 0 on (96, 300, 4), index_resets >= 2 under capacity 4 and == 0 without, and every table counter of the
BEAGLE_MI355_NO_REPEATS=1 twin is 0; on 20 and 61 states walks > 0.  No chain seed had to be replaced; the WORKLOAD of (96, 300, 4) is
drawn with seed 502, the one tests/test_gpu_memdef_tables.py makes its sub-run case with on this shape — under the rule's seed no chain
took a sub-run (topology_chains.WORKLOAD_SEEDS).  Reached, in one run on an MI355X: root calls inside the walk's launch on another root
171 / 236 on the two first shapes; (24, 129, 1) 22 table reads behind topology moves, 580 memory reads, 2 clades indexed there;
(48, 1000, 4) 19 / 563 / 10; (96, 300, 4) 200 / 1604 / 54 and 21 sub-runs; 11 index resets under capacity 4 (121 table reads), none
without; the shipped shape 14 table reads and 4 sub-runs behind topology moves at the engine's own constants; walks 588 (20 states) and
284 (61 states).

Gradients behind topology moves (part of the same driver): shapes (4, 4, 12, 130) and (20, 2, 8, 33), unscaled, seeds 1 and 2; on 4 states
30 pre-order lists answered while held and 26 run late, gradients taken on 9 and 15 different sets of cherries.

What these chains found: BEAGLE_MI355_NO_PLAN_CACHE=1 did NOT keep the bits of a DYNAMIC chain whose closed lists have 16 operations or
more — the engine folds reciprocal scale factors and reads class tables in KEPT plans only, and with the switch no plan was kept (lnL
differed in its last bits, 1.8e-12 of -2e3, from the first read-mode model move on; tests/test_gpu_switches.py never saw it because its
chain uploads partials for two tips, whose lists are never kept).  With the switch the planner now plans every list from scratch and
still keeps a closed list's plan (planner.cpp cacheStep; tests/native/plan_harness.h topologyWithoutPlanCache holds the plans to the
cached ones byte for byte).

Every chain prints its wall time.  Measured on an MI355X, one run, per chain (60 proposals; engine, twins and oracle): 0.03 .. 0.07 s on
the small shapes (0.36 s for the first of the process), 0.06 .. 0.07 s at (24, 129, 1) with five instances, 0.12 .. 0.15 s at
(48, 1000, 4), 0.08 .. 0.19 s at (96, 300, 4), and 0.47 .. 0.65 s for the 20 proposals of 400 tips x 16385 patterns — the longest, far
below the 10 s at which it would have had to be shortened.  The whole module: 10 s.
"""
import collections
import os
import time

import numpy as np
import pytest

import beast_mcmc_amd as bm
import topology_chains as tc
from test_topology_chains_host import (CASES, COMPRESSED, GRADIENT_SHAPES, OTHER_KERNELS, SEEDS, SCHEMES, SHAPES, SHIPPED, WALK4, case_id,
                                       node_stride, records)

pytestmark = pytest.mark.gpu

TWIN_ENV = {"BEAGLE_MI355_COPY_ENGINE_UPLOADS": "1", "BEAGLE_MI355_NO_PLAN_CACHE": "1"}
COMPRESSED_ENV = {"BEAGLE_MI355_REPEATS_ANY_SIZE": "1", "BEAGLE_MI355_MEM_DEF_STEPS": "8", "BEAGLE_MI355_REPEAT_MAX_FRAC": "1/2"}
CAPACITY_ENV = dict(COMPRESSED_ENV, BEAGLE_MI355_REPEAT_CAPACITY="4")
SWITCHES = ("BEAGLE_MI355_COPY_ENGINE_UPLOADS", "BEAGLE_MI355_NO_PLAN_CACHE", "BEAGLE_MI355_REPEATS_ANY_SIZE", "BEAGLE_MI355_MEM_DEF_STEPS",
            "BEAGLE_MI355_REPEAT_MAX_FRAC", "BEAGLE_MI355_REPEAT_CAPACITY", "BEAGLE_MI355_NO_REPEATS", "BEAGLE_MI355_NO_MEMDEF_TABLES",
            "BEAGLE_MI355_NO_FAST_WALK", "BEAGLE_MI355_NO_SLICE_SUMS")


def created_under(env, make):
    """make() with exactly the BEAGLE_MI355_* switches `env` of this module's in force (the engine reads them at instance creation)"""
    old = {k: os.environ.pop(k, None) for k in SWITCHES}
    os.environ.update(env)
    try:
        return make()
    finally:
        for k in SWITCHES:
            os.environ.pop(k, None)
            if old[k] is not None:
                os.environ[k] = old[k]


def environment(shape):
    return dict(COMPRESSED_ENV) if shape in COMPRESSED else {}


def twins_for(shape, env):
    twins = [("uploads by the copy engine, no plan cache", dict(env, **TWIN_ENV))]
    if shape in COMPRESSED:
        twins.append(("BEAGLE_MI355_NO_REPEATS=1", dict(env, BEAGLE_MI355_NO_REPEATS="1")))
        twins.append(("BEAGLE_MI355_NO_MEMDEF_TABLES=1", dict(env, BEAGLE_MI355_NO_MEMDEF_TABLES="1")))
    return twins


def fail(what, shape, seed, scheme, step, recs, tmp_path):
    path = str(tmp_path / ("chain_%s_seed%d_%s.json" % (tc.shape_id(shape), seed, tc.SCHEME_NAMES[scheme])))
    tc.dump(path, shape, seed, scheme, recs)
    raise AssertionError("shape %s seed %d scheme %s step %d %s: %s\nreplay: python tests/topology_chains.py --replay %s"
                         % (shape, seed, tc.SCHEME_NAMES[scheme], step, "(before the chain)" if step < 0 else tc.describe(recs[step]), what, path))


def lockstep(shape, seed, scheme, oracle_lib, tmp_path, env=None, twins=None, checkpoints=True, gradients=False):
    """-> the engine's route counters over the chain.  gradients: the pre-order list, the root's pre-order partial and the edge sums of the
    current tree behind every fourth proposal, every pre-order partial at the end (topology_chains.Driver.gradient)"""
    recs = records(shape, seed, scheme, checkpoints)
    env = environment(shape) if env is None else env
    twins = twins_for(shape, env) if twins is None else twins
    instances, total = [], collections.Counter()
    started = time.perf_counter()
    try:
        eng = created_under(env, lambda: tc.create(shape, bm.beagle.Beagle, gradients=gradients))
        instances.append(eng)
        sides = []
        for name, tenv in twins:
            t = created_under(tenv, lambda: tc.create(shape, bm.beagle.Beagle, gradients=gradients))
            instances.append(t)
            sides.append((name, t, tc.Driver(t, shape, scheme)))
        ora = tc.create(shape, bm.beagle.Beagle, library=oracle_lib, gradients=gradients)
        instances.append(ora)
        de, do = tc.Driver(eng, shape, scheme), tc.Driver(ora, shape, scheme)
        first_root = de.tree.root
        worst = collections.defaultdict(float)

        def drain(prefix=None):
            """the walk counters since the last drain into `total` (and under `prefix`), then restarted"""
            stats = dict(eng.walkStats(), **eng.repeatSubRunStats())
            for k in ("walks", "fast_walks", "mem_reads", "table_reads", "repeat_clades", "table_rows", "sub_runs"):
                total[k] += stats[k]
                if prefix:
                    total[prefix + k] += stats[k]
            eng.kernelTimerRestart()

        behind_topology = False
        for step, rec in enumerate([None] + recs, start=-1):
            kw = {} if rec is None else {"node_stride": node_stride(shape), "gradients": gradients}
            if behind_topology:
                drain()
                indexed = eng.repeatStats()["clades_indexed"]
            fused = eng.rootFusedCount()
            rc_e, got = tc.run_step(de, rec, first=rec is None, **kw)
            if de.evaluated_root != first_root:               # (the proposal's root, whether or not it is accepted)
                total["root_fused_after_root_change"] += eng.rootFusedCount() - fused
            total["root_fused"] += eng.rootFusedCount() - fused
            if behind_topology:
                drain("behind_topology_")
                total["clades_indexed_behind_topology"] += eng.repeatStats()["clades_indexed"] - indexed
            behind_topology = rec is not None and rec["move"] in tc.TOPOLOGY_MOVES and rec["accept"]
            rc_o, want = tc.run_step(do, rec, first=rec is None, **kw)
            for name, _, dt in sides:
                rc_t, same = tc.run_step(dt, rec, first=rec is None, **kw)
                if rc_t != rc_e:
                    fail("return codes engine %d, twin (%s) %d" % (rc_e, name, rc_t), shape, seed, scheme, step, recs, tmp_path)
                if len(same) != len(got):
                    fail("%d reads on the engine, %d on its twin (%s)" % (len(got), len(same), name), shape, seed, scheme, step, recs, tmp_path)
                for k, ((kind, a), (_, b)) in enumerate(zip(got, same)):
                    if not np.array_equal(a, b):
                        fail("read %d (%s): the engine and its twin (%s) differ, by at most %.3e" % (k, kind, name, float(np.max(np.abs(a - b)))),
                             shape, seed, scheme, step, recs, tmp_path)
            if rc_e != rc_o:
                fail("return codes engine %d, oracle %d" % (rc_e, rc_o), shape, seed, scheme, step, recs, tmp_path)
            if len(got) != len(want):
                fail("%d reads on the engine, %d on the oracle" % (len(got), len(want)), shape, seed, scheme, step, recs, tmp_path)
            for k, ((kind, a), (_, b)) in enumerate(zip(got, want)):
                d = tc.deviation(kind, a, b)
                worst[kind] = max(worst[kind], d) if d == d else d
                if not d <= tc.BOUND:
                    fail("read %d (%s): engine against oracle %.3e, bound %.0e" % (k, kind, d, tc.BOUND), shape, seed, scheme, step, recs, tmp_path)
        drain()
        rep = eng.repeatStats()
        total["clades_indexed"], total["index_resets"] = rep["clades_indexed"], rep["index_resets"]
        grad = eng.gradientStats()
        total["gradient_held_answered"], total["gradient_late"], total["cherry_sets"] = grad["fused"] + grad["walked"], grad["late"], len(de.cherry_sets)
        info = eng.walkLaunchInfo()
        total["one_launch_walks"] = info["ticket_walks"] + info["flag_walks"]
        for name, t, _ in sides:
            if "NO_REPEATS" in name:
                off = t.repeatStats()
                total["no_repeats_twin_tables"] = off["table_rows"] + off["table_reads"] + off["repeat_clades"] + off["clades_indexed"]
        print("%s%s%s%s: %d proposals, %d instances, %.2f s; largest deviation from the oracle by kind of read: %s; counters %s"
              % (case_id((shape, seed, scheme)), "" if checkpoints else ", no checkpoint reads", ", gradients" if gradients else "", "".join(" %s=%s" % (k[13:], v) for k, v in sorted(env.items())),
                 len(recs), len(instances), time.perf_counter() - started, ", ".join("%s %.1e" % kv for kv in sorted(worst.items())), dict(total)))
        return total
    finally:
        for b in instances:
            b.finalize()


_counters = {}


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_engine_twins_and_oracle_in_lockstep(case, oracle_lib, tmp_path):
    _counters[case] = None                                   # (failed, unless the next line returns: not run a second time below)
    _counters[case] = lockstep(*case, oracle_lib, tmp_path)


@pytest.mark.parametrize("shape", [s for s in SHAPES if s[0] in (4, 20, 61)], ids=tc.shape_id)
def test_the_chains_take_the_routes_they_are_for(shape, oracle_lib, tmp_path):
    """Conditions, not results: the counters of the routes this module exists for, summed over the shape's seeds and schemes (a chain the
    test above has not run is run here; one that failed there counts nothing)."""
    total = collections.Counter()
    for seed in SEEDS[shape]:
        for scheme in SCHEMES[shape]:
            case = (shape, seed, scheme)
            if case not in _counters:
                _counters[case] = lockstep(*case, oracle_lib, tmp_path)
            total.update(_counters[case] or {})
    print("shape %s: %s" % (shape, dict(total)))
    if shape[0] != 4:
        assert total["walks"] > 0, dict(total)
        return
    assert total["one_launch_walks"] > 0 and total["root_fused_after_root_change"] > 0, dict(total)
    if shape in COMPRESSED:
        assert total["behind_topology_table_reads"] > 0 and total["behind_topology_repeat_clades"] > 0, dict(total)
        assert total["mem_reads"] > 0 and total["clades_indexed_behind_topology"] > 0, dict(total)
        assert total["index_resets"] == 0 and total["no_repeats_twin_tables"] == 0, dict(total)
        if shape == (4, 4, 96, 300, "compressed"):
            assert total["sub_runs"] > 0, dict(total)


def test_the_class_index_is_dropped_at_its_capacity_inside_a_chain(oracle_lib, tmp_path):
    """(24, 129, 1) under BEAGLE_MI355_REPEAT_CAPACITY=4: the index reaches its capacity and is dropped at least twice over the two seeds,
    tables are read all the same, and every bit stays that of the twins (which share the capacity) and within bounds of the oracle."""
    total = collections.Counter()
    for seed in SEEDS[COMPRESSED[0]]:
        total.update(lockstep(COMPRESSED[0], seed, tc.SCHEME_DYNAMIC, oracle_lib, tmp_path, env=CAPACITY_ENV))
    print("capacity 4: %s" % dict(total))
    assert total["index_resets"] >= 2 and total["table_reads"] > 0 and total["no_repeats_twin_tables"] == 0, dict(total)


def test_assembly_loop_and_cpp_kernel_keep_the_same_bits_through_a_chain(oracle_lib, tmp_path):
    """(4, 4, 96, 300): the assembly loop against BEAGLE_MI355_NO_FAST_WALK=1, BEAGLE_MI355_NO_SLICE_SUMS=1 on both sides."""
    shape = COMPRESSED[2]
    env = dict(COMPRESSED_ENV, BEAGLE_MI355_NO_SLICE_SUMS="1")
    for scheme in (tc.SCHEME_NONE, tc.SCHEME_DYNAMIC):
        total = lockstep(shape, 1, scheme, oracle_lib, tmp_path, env=env, twins=[("BEAGLE_MI355_NO_FAST_WALK=1", dict(env, BEAGLE_MI355_NO_FAST_WALK="1"))])
        assert total["fast_walks"] > 0 and total["table_reads"] > 0, dict(total)


@pytest.mark.parametrize("shape", [WALK4[0], COMPRESSED[2], SHIPPED, OTHER_KERNELS[0]], ids=tc.shape_id)
def test_chains_without_checkpoint_reads(shape, oracle_lib, tmp_path):
    """Nothing is materialised for the test's sake: lnL at every step (and the site values every fifth), node buffers at the end only."""
    lockstep(shape, 2, tc.SCHEME_DYNAMIC, oracle_lib, tmp_path, checkpoints=False)


@pytest.mark.parametrize("shape", GRADIENT_SHAPES, ids=tc.shape_id)
def test_gradients_behind_topology_moves(shape, oracle_lib, tmp_path):
    """Unscaled chains, seeds 1 and 2: behind every fourth proposal, accepted or rejected, the whole-tree pre-order list of the CURRENT
    topology over the current buffer flips, the root's pre-order partial and calculateEdgeDifferentials on every branch; the edge sums
    against the oracle as tests/test_gpu_gradients.py ``close`` compares them, every pre-order partial at the end, the twin bit for bit.
    On 4 states a pre-order list was answered while held and one was run late by a later call, and the gradients were taken on more
    than one set of cherries — the nodes a gradient chain's post-order lists leave unstored (BEAGLE_MI355_GRADIENT_VIRTUAL, default)."""
    total = collections.Counter()
    for seed in (1, 2):
        total.update(lockstep(shape, seed, tc.SCHEME_NONE, oracle_lib, tmp_path, gradients=True))
    print("shape %s, gradients: %s" % (shape, dict(total)))
    assert total["cherry_sets"] >= 4
    if shape[0] == 4:
        assert total["gradient_held_answered"] > 0 and total["gradient_late"] > 0, dict(total)
