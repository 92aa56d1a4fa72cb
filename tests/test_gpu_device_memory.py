"""The instance's grow-on-demand device buffers (csrc/engine_internal.h DevBuf, growDevice): growing one changes no result, a call
that needs no growth changes no byte of beagleMi355DeviceBytes, and an instance gives back what it took.

Every case makes a second call need more than the first, which is all a growth path asks for; the shapes are the smallest that reach
the path in question (the general layout, the 4-state walk, the T32 level path with cherry tables)."""
import ctypes as C
import os

import numpy as np
import pytest

import beast_mcmc_amd as bm
import helpers
from beast_mcmc_amd.ancestral import AncestralStateSampler
from beast_mcmc_amd.gradient import BranchGradient
from beast_mcmc_amd.markovjumps import MarkovJumpsSampler
from beast_mcmc_amd.treelikelihood import RESCALE_ALWAYS, BeagleTreeLikelihood

pytestmark = pytest.mark.gpu
NONE = bm.beagle.NONE


def evaluated(wl, **kw):
    tl = BeagleTreeLikelihood(wl, **kw)
    tl.getLogLikelihood()
    return tl


def general_workload():
    """7 states, 2 categories, 8 tips, 50 patterns: the general layout, no virtual buffers — nothing but scratch allocates after the
    first evaluation"""
    return helpers.random_workload(8, 50, 7, 2, seed=17)


def test_ancestral_scratch_growth():
    wl = general_workload()
    tl = evaluated(wl)
    sampler = AncestralStateSampler(tl)
    raw = sampler.beagle
    rows, _ = sampler.node_list()
    prefix, P = rows[:3], wl.pattern_count                  # (a prefix of a pre-order list is a list: parents come first)
    first = raw.sampleAncestralStates(prefix, 0, 0, 11)
    bytes_prefix = raw.deviceBytes()
    full = raw.sampleAncestralStates(rows, 0, 0, 11)
    bytes_full = raw.deviceBytes()
    again = raw.sampleAncestralStates(prefix, 0, 0, 11)
    assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1])
    assert raw.deviceBytes() == bytes_full                  # no growth, no byte

    def layout(n):                                          # states [n][P] to 256 bytes | categories [P] ints | error word
        return ((n * P + 255) & ~255) + 4 * P + 4
    assert bytes_full - bytes_prefix == layout(len(rows)) - layout(3)
    fresh = evaluated(wl)
    expect = AncestralStateSampler(fresh).beagle.sampleAncestralStates(rows, 0, 0, 11)
    assert np.array_equal(full[0], expect[0]) and np.array_equal(full[1], expect[1])
    tl.close(); fresh.close()


def test_markov_jump_scratch_growth():
    wl = general_workload()
    tl = evaluated(wl)
    S = wl.state_count
    one, three = MarkovJumpsSampler(tl), MarkovJumpsSampler(tl)       # two register sets over the same instance
    one.add_register("all", np.ones((S, S)))
    three.add_register("all", np.ones((S, S)))
    three.add_register("upper", np.triu(np.ones((S, S)), 1))
    three.add_register("reward", np.linspace(0.5, 2.0, S), kind="rewards", scale_by_time=True)
    a = one.sample(5)
    b = three.sample(5)
    bytes_three = one.beagle.deviceBytes()
    c = one.sample(5)
    for key in ("branch", "pattern", "tree"):
        assert np.array_equal(a[key], c[key]), key
    assert b["branch"].shape[0] == 3
    assert one.beagle.deviceBytes() == bytes_three
    tl.close()


# seeds of test_uniformized_event_list_growth: the second draws more events than the first (asserted there)
EVENT_SEEDS = (3, 4)


def test_uniformized_event_list_growth():
    wl = helpers.random_workload(8, 50, 4, 2, seed=23)
    tl = evaluated(wl)
    s = MarkovJumpsSampler(tl)
    s.add_register("all", np.ones((4, 4)))
    first = s.sample(EVENT_SEEDS[0], uniformization=True, history=True)["events"]
    second = s.sample(EVENT_SEEDS[1], uniformization=True, history=True)["events"]
    print("events: %d then %d" % (len(first["height"]), len(second["height"])))
    assert len(second["height"]) > len(first["height"])     # the event list had to grow
    third = s.sample(EVENT_SEEDS[0], uniformization=True, history=True)["events"]
    for key in ("node", "pattern", "height", "states"):
        assert np.array_equal(first[key], third[key]), key
    tl.close()


def partition_round_trip(wl):
    """4 states, write-mode rescaling on every evaluation: one partition, two, one again.  The slice-sum vectors, the flag block, the
    kept device programs and the matrix block are all re-made on the way.  -> (the driver, lnL before, with two partitions, after)"""
    tl = BeagleTreeLikelihood(wl, rescaling=RESCALE_ALWAYS, delay_rescaling=False)
    raw = helpers.raw_binding(tl)
    tl.getLogLikelihood()
    tl.makeDirty()
    before = tl.getLogLikelihood()
    P = wl.pattern_count
    raw.setPatternPartitions(2, np.repeat(np.array([0, 1], dtype=np.int32), [P // 2 + 3, P - P // 2 - 3]))
    tl.makeDirty()
    two = tl.getLogLikelihood()
    raw.setPatternPartitions(1, np.zeros(P, dtype=np.int32))
    tl.makeDirty()
    after = tl.getLogLikelihood()
    return tl, raw, before, two, after


def walk_workload():
    return helpers.random_workload(9, 300, 4, 4, seed=41)


def test_partition_round_trip_is_bit_exact():
    tl, raw, before, two, after = partition_round_trip(walk_workload())
    assert after == before
    assert helpers.rel_err(two, before) <= 1e-12            # (the same sum in two pieces)
    info = raw.walkLaunchInfo()
    assert info["ticket_walks"] + info["flag_walks"] > 0
    tl.close()


def test_cherry_tables_grow(engine_lib, monkeypatch):
    """61 states, 6 tips, 70 patterns: a caterpillar (one cherry), then a balanced tree (three) — the column tables of the virtual
    cherries grow between the two lists."""
    # (read at creation: 21..64 states run level by level instead of as the walk, and leave tip-tip nodes unstored — the one
    # combination that builds the tables)
    monkeypatch.setenv("BEAGLE_MI355_NO_T64_WALK", "1")
    monkeypatch.setenv("BEAGLE_MI355_CHERRY61", "1")
    S, T, P, C = 61, 6, 70, 2
    wl = helpers.random_workload(T, P, S, C, seed=61)
    caterpillar = [6, 0, 1,  7, 6, 2,  8, 7, 3,  9, 8, 4,  10, 9, 5]
    balanced = [6, 0, 1,  7, 2, 3,  8, 4, 5,  9, 6, 7,  10, 9, 8]

    def instance():
        b = bm.beagle.Beagle(T, 2 * T - 1, T, S, P, 1, 2 * T - 1, C, 0, library=engine_lib)
        for t in range(T):
            b.setTipStates(t, wl.tip_states[t])
        b.setPatternWeights(wl.weights)
        b.setEigenDecomposition(0, wl.eig.evec, wl.eig.ievc, wl.eig.evals)
        b.setCategoryRates(wl.cat_rates); b.setCategoryWeights(0, wl.cat_weights); b.setStateFrequencies(0, wl.freqs)
        b.updateTransitionMatrices(0, list(range(10)), None, None, list(np.linspace(0.05, 0.4, 10)), 10)
        return b

    def evaluate(b, tree):
        ops = []
        for k in range(0, len(tree), 3):
            d, l, r = tree[k:k + 3]
            ops += [d, NONE, NONE, l, l, r, r]
        b.updatePartials(ops, len(ops) // 7, NONE)
        out = [0.0]
        b.calculateRootLogLikelihoods([10], [0], [0], [NONE], 1, out)
        return out[0]

    b, fresh = instance(), instance()
    try:
        first = evaluate(b, caterpillar)
        bytes_one = b.deviceBytes()
        second = evaluate(b, balanced)
        assert b.deviceBytes() > bytes_one                  # the tables of three cherries do not fit what one cherry took
        assert np.isfinite(first) and second == evaluate(fresh, balanced)
    finally:
        b.finalize(); fresh.finalize()


def free_device_memory():
    """hipMemGetInfo's free bytes — what torch.cuda.mem_get_info() returns — asked of the HIP runtime the engine links.  torch ships a
    runtime of its own; two of them in one process do not get along (whichever is loaded second finds no device, or a later load of
    the system's library fails), so this process asks the one it already has."""
    hip = C.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))
    free, total = C.c_size_t(), C.c_size_t()
    assert hip.hipDeviceSynchronize() == 0
    assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return free.value


# What torch.cuda.mem_get_info() reports free after the 2nd iteration minus after the 10th of lifecycle(), measured on an MI355X with
# the engine as it was before the buffers moved to one owner (0 bytes, twice), and the step in which that figure moves: a hipMalloc
# of 2 MiB + 1 takes 4 MiB off it, one of 1 MiB or less nothing (profiles/device_memory_refactor.txt)
PARENT_DRIFT_BYTES = 0
ALLOCATION_GRANULE_BYTES = 2 << 20


def lifecycle(iterations=10):
    """create / exercise / finalize: the partition round trip, one getPartials, one edge-gradient call.  -> free device memory after
    the 2nd and after the last iteration"""
    wl = walk_workload()
    free = {}
    for it in range(1, iterations + 1):
        tl, raw, before, _, after = partition_round_trip(wl)
        assert after == before
        assert np.isfinite(raw.getPartials(tl.root_buffer_index(), NONE)).all()
        tl.close()
        g = BranchGradient(wl, rescale=True)
        lnl, grad, per = g.gradient(per_pattern=True)
        assert np.isfinite(lnl) and np.isfinite(grad).all() and np.isfinite(per).all()
        g.close()
        free[it] = free_device_memory()
    return free[2], free[iterations]


def test_instances_give_back_what_they_took():
    """Ten instances in a row leave the device's free memory where two left it.  Measured on an MI355X, free memory after the 2nd
    iteration minus after the 10th: 0 bytes with the engine before this change (308388298752 both times, two runs; it frees everything
    too, so that is the noise floor of the runtime's allocator, not a budget) and 0 bytes with this one (two runs).  The bound is the
    former plus one allocation granule, 2 MiB."""
    second, last = lifecycle()
    drift = second - last
    print("free after iteration 2: %d, after iteration 10: %d, drift %d bytes" % (second, last, drift))
    assert drift <= PARENT_DRIFT_BYTES + ALLOCATION_GRANULE_BYTES
