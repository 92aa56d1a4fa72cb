"""The switches of the product library that no other test sets, each held to the default path and to the oracle.

5.1 promises that every switch leaves the results unchanged: bit for bit, or "to rounding" where its row says so.  Several switches
are the only way into a shipped kernel or branch at some state count (BEAGLE_MI355_NO_MFMA: the plain-layout VALU kernels at 16..64
states, and the samplers reading plain-layout partials there).  SWITCHES below is the one table of what is tested: per switch the
values, where it takes effect, the promise, the scenarios it runs in and how a case proves that the switched path really ran.

Every case runs a scenario on an instance created under the switch, again on the default path and once on the CPU oracle.  'bits':
every output equal (np.array_equal); 'rounding': lnL and site lnL to 1e-13 relative, node partials to 1e-12 of each pattern's largest
entry (the suite's per-(category, state) max-normalisation), log scale factors to 1e-12.  The oracle: 1e-10, as everywhere else.
Both engine sides run with BEAGLE_MI355_NO_SLICE_SUMS=1 (the cumulative buffer from the per-node factors: the per-slice products
depend on how a program is cut into slices, which several of these switches change; tests/test_gpu_slice_sums.py holds them).

PRE_TWO_PASS, EDGE_TWO_STEP and RESCALE_TWO_PASS are read into function-local statics: fixed at the first use in a process.  Their
cases run the scenario in a fresh child process with the switch set from the start; the parent computes the default path and the
oracle and compares.

test_every_product_switch_is_exercised_by_a_gpu_test (CPU tier) keeps the list honest: a switch added to 5.1 without a GPU test
fails there.
"""
import contextlib
import ctypes as C
import os
import re
import subprocess
import sys
from collections import namedtuple

import numpy as np
import pytest

import beast_mcmc_amd as bm
import helpers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.join(ROOT, "tests")
NONE = bm.beagle.NONE
SW = "BEAGLE_MI355_"
REL_TOL = 1e-10

Switch = namedtuple("Switch", "values where promise scenarios evidence")

# name (without BEAGLE_MI355_) -> what is tested.  evidence: how a case shows that the switched path ran ('none: ...' where no counter
# the engine exports tells the two paths apart; the case then asserts what it can of the preconditions).
SWITCHES = {
    "NO_MFMA": Switch(("1",), "16..64 states (plain layout instead of the T32 tiles)", "rounding",
                      ("likelihood", "gradient", "partitions", "samplers"),
                      "deviceBytes: the plain layout's buffers (no 32-pattern tiles; no pattern count here is a multiple of 32), "
                      "and walkStats: walks == 0 (the level kernels) where the default ran the T32 / T64 walk"),
    "NO_LAUNCH_FUSION": Switch(("1",), "4 states (root kernel, held walks, fused transition kernels, by-partition roots)", "rounding",
                               ("likelihood", "gradient", "partitions", "uploads"),
                               "rootFusedCount() == 0 and partition_roots_in_walk == 0 where the default counts them (the kernel "
                               "timer brackets pruning launches only, so the extra root launch is not in its count)"),
    "COPY_ENGINE_UPLOADS": Switch(("1",), "every instance (small host arrays)", "bits", ("likelihood", "partitions", "uploads"),
                                  "none: no exported counter sees how an upload travels"),
    "NO_PLAN_CACHE": Switch(("1",), "4 states (walk planner)", "bits", ("likelihood", "partitions"),
                            "none: the planner's cache hits are printed by HOST_TIMING only"),
    "NO_WALK_FUSION": Switch(("1",), "4 states, one-launch walk", "bits", ("likelihood", "partitions"),
                             "walkLaunchInfo: no ticket or flag walk, walkStats: walks > 0"),
    "NO_LOAD_SKIP": Switch(("1",), "4 states, read-mode programs on the assembly loop", "bits", ("likelihood",),
                           "none: the tip-load flags live in the device program; walkStats counts the same tip vectors either way"),
    "NO_XCD_MAP": Switch(("1",), "4 states, ticket launches of >= 16 slices the chip holds at once", "bits", ("likelihood", "partitions"),
                         "none: the grid layout is not exported; the case asserts that a ticket launch of >= 16 slices ran"),
    "NO_FUSED_GRADIENT": Switch(("1",), "4 states, pre-order lists", "rounding", ("gradient",),
                                "gradientStats: by_operation > 0, fused == 0"),
    "NO_PRE_WALK": Switch(("1",), "4 states, held pre-order lists", "rounding", ("gradient",), "gradientStats: walked == 0"),
    "PRE_TWO_PASS": Switch(("1",), "16..64 states, pre-order operations (read once per process)", "rounding", ("gradient",),
                           "none: pre-order launches are outside the kernel timer; gradientStats counts 4 states only"),
    "EDGE_TWO_STEP": Switch(("1", "2"), "16..64 states, edge derivatives (read once per process)", "rounding", ("gradient",),
                            "none: edge-derivative launches are outside the kernel timer; gradientStats counts 4 states only"),
    "RESCALE_TWO_PASS": Switch(("1",), "16..20 states, <= 4 categories, write-mode levels without virtual cherries "
                               "(with NO_T32_WRITE_WALK=1; read once per process)", "bits", ("likelihood",),
                               "none: the extra k_rescaleTiled launch is inside a level of the kernel timer's count; the case "
                               "asserts that the write-mode evaluation ran level by level (walks == 0, a launch per level)"),
    "SHARD_SPIN_US": Switch(("0",), "the sharded handle's host threads", "bits", ("sharded",),
                            "none: no counter sees a host thread sleep"),
}

# product switches no GPU test needs to set (test_every_product_switch_is_exercised_by_a_gpu_test)
NOT_GPU_TESTED = {
    "BEAGLE_MI355_DEBUG": "diagnostics only: error text on stderr",
    "BEAGLE_MI355_HOST_TIMING": "diagnostics only: host-time report at finalize",
    "BEAGLE_MI355_COLLECTIVE": "Python veneer setting (multi-GPU all-reduce), not the library",
    "BEAGLE_MI355_COMM_INIT_TIMEOUT_S": "Python veneer setting (communicator rendezvous), not the library",
    "BEAGLE_MI355_ENGINE_LIB": "Python veneer setting (which engine build to load), not the library",
    "BEAGLE_MI355_SHARDS": "tested elsewhere: it is the sharded handle's size (tests/test_gpu_sharded_instance.py)",
}


def product_switches():
    """Every BEAGLE_MI355_* name of INTEGRATION.md 5.1 (as test_host_and_abi.py parses it)."""
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    product = text.split("**5.2 LAB builds only**")[0]
    product = product[product.index("**5.1 Switches of the product library**"):]
    return set(re.findall(r"BEAGLE_MI355_[A-Z0-9_]+", product))


def test_every_product_switch_is_exercised_by_a_gpu_test():
    """CPU tier.  Every switch of 5.1 is set by at least one tests/test_gpu_*.py, but for the listed exceptions; the table above
    names only switches of 5.1, and every switch of it gives the promise and scenarios it is tested with."""
    documented = product_switches()
    assert len(documented) >= 30, documented
    gpu_tests = ""
    for f in sorted(os.listdir(TESTS)):
        if f.startswith("test_gpu_") and f.endswith(".py"):
            gpu_tests += open(os.path.join(TESTS, f)).read()
    # (a name counts where it is spelled out, or as a key of SWITCHES: the cases below prefix those with BEAGLE_MI355_)
    mentioned = set(re.findall(r"BEAGLE_MI355_[A-Z0-9_]+", gpu_tests)) | {SW + k for k in SWITCHES}
    untested = sorted(documented - mentioned - set(NOT_GPU_TESTED))
    assert not untested, "switches of INTEGRATION.md 5.1 that no GPU test sets: %s" % untested
    assert set(NOT_GPU_TESTED) <= documented, set(NOT_GPU_TESTED) - documented
    assert {SW + k for k in SWITCHES} <= documented, {SW + k for k in SWITCHES} - documented
    for k, s in SWITCHES.items():
        assert s.promise in ("bits", "rounding") and s.values and s.scenarios and s.evidence, k
    # ... and the promise agrees with the document's row: "to rounding" there exactly where the table says 'rounding'
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for k, s in SWITCHES.items():
        row = [line for line in text.splitlines() if line.startswith("| `%s%s" % (SW, k))]
        assert len(row) == 1, k
        assert ("to rounding" in row[0]) == (s.promise == "rounding"), (k, row[0])


# -- plumbing ----------------------------------------------------------------------------------------------------------------------

@contextlib.contextmanager
def switched(env):
    """BEAGLE_MI355_<k>=<v> for every item of env (keys without the prefix) while the block runs (instances read them at creation)."""
    full = {(k if k.startswith(SW) else SW + k): str(v) for k, v in env.items()}
    old = {k: os.environ.get(k) for k in full}
    os.environ.update(full)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def norm_err(a, b):
    """max |a - b| over each pattern's largest |b| (category and state: axes -3 and -1)"""
    a, b = np.asarray(a), np.asarray(b)
    scale = np.maximum(np.abs(b).max(axis=(-3, -1), keepdims=True), 1e-300)
    return float(np.max(np.abs(a - b) / scale)) if b.size else 0.0


def site_rel(a, b):
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300))) if len(b) else 0.0


def abs_rel(a, b):
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    return float(np.max(np.abs(a - b))) / max(1.0, float(np.max(np.abs(b)))) if b.size else 0.0


def same(a, b, promise, what):
    """the switched path's outputs `a` against the default path's `b` (dicts of the same keys): 5.1's promise"""
    assert a.keys() == b.keys()
    for key in a:
        for i, (x, y) in enumerate(zip(a[key], b[key])):
            x, y = np.asarray(x, dtype=float), np.asarray(y, dtype=float)
            assert x.shape == y.shape, (what, key, i)
            if promise == "bits":
                assert np.array_equal(x, y), (what, key, i, np.argwhere(x != y)[:5])
            elif key == "lnl" or key == "site":
                assert site_rel(x.ravel(), y.ravel()) <= 1e-13, (what, key, i, site_rel(x.ravel(), y.ravel()))
            elif key == "parts":
                assert norm_err(x, y) <= 1e-12, (what, key, i, norm_err(x, y))
            else:
                assert abs_rel(x, y) <= 1e-12, (what, key, i, abs_rel(x, y))


# -- scenario 1: the likelihood chain ----------------------------------------------------------------------------------------------

from beast_mcmc_amd.treelikelihood import BeagleTreeLikelihood, RESCALE_ALWAYS, RESCALE_DYNAMIC   # noqa: E402

SCHEMES = {"dynamic": RESCALE_DYNAMIC, "always": RESCALE_ALWAYS}
# (S, T, P, C): every pattern count of the issue (1, 31 / 33, 127 / 129, > 2 048) and 1, 4, 5, 16 categories appear on both sides;
# T = 400 at 4 states gives a program of >= 16 slices of one pattern group each (NO_XCD_MAP's launches)
SHAPES4 = [(4, 48, 1, 4), (4, 40, 129, 1), (4, 64, 2100, 5), (4, 33, 31, 16), (4, 400, 100, 4)]
SHAPES_T = [(16, 20, 33, 4), (20, 24, 129, 1), (32, 16, 127, 5), (61, 10, 31, 16), (64, 12, 2100, 4)]
TIP_PARTIALS = (0, 3)


def chain_workload(S, T, P, C):
    return helpers.random_workload(T, P, S, C, seed=5100 + S + T + P + C, unknown_fraction=0.08)


def likelihood_chain(wl, scheme, env, library=None):
    """Write-mode evaluation, read-mode evaluation, storeState / node-height move / restoreState, a branch-rate move on flipped buffers,
    then lnL, site lnL, every internal node's partials and every scale buffer; two tips carry partials.  -> (outputs, evidence)."""
    with switched(env if library is None else {}):
        tl = BeagleTreeLikelihood(wl, library=library, rescaling=SCHEMES[scheme], delay_rescaling=False)
    rng = np.random.default_rng(17)
    for t in TIP_PARTIALS:
        part = rng.uniform(0.05, 1.0, size=(wl.pattern_count, wl.state_count))
        part[rng.random(wl.pattern_count) < 0.3] = 1.0
        part = np.ascontiguousarray(part)
        assert tl.h.btlSetTipPartials(tl.ptr, t, part.ctypes.data_as(C.POINTER(C.c_double))) == 0
    raw = bm.beagle.Beagle.attach(tl)
    lnl = [tl.getLogLikelihood()]                       # write mode (DYNAMIC's first evaluation rescales)
    tl.makeDirty()
    lnl.append(tl.getLogLikelihood())                   # DYNAMIC: read mode; ALWAYS: write mode again
    node = wl.tree.node_count - 3
    h = float(wl.tree.height[node])
    tl.storeState()
    tl.set_node_height(node, helpers.proposed_height(wl.tree, node, rng))
    lnl.append(tl.getLogLikelihood())
    tl.restoreState()
    tl.restore_node_height(node, h)
    lnl.append(tl.getLogLikelihood())
    tl.storeState()
    tl.set_branch_rates(rng.uniform(0.8, 1.25, wl.tree.node_count))
    lnl.append(tl.getLogLikelihood())
    nodes = list(range(wl.tree.tip_count, wl.tree.node_count))
    out = {"lnl": [np.array(lnl)], "site": [tl.getSiteLogLikelihoods().copy()]}
    if library is None:
        out["parts"] = list(raw.getPartialsBatch([tl.node_buffer_index(n) for n in nodes]))
    else:
        out["parts"] = [raw.getPartials(tl.node_buffer_index(n), NONE).copy() for n in nodes]
    out["scales"] = [raw.getLogScaleFactors(tl.node_scale_index(n)).copy() for n in nodes]
    out["scales"].append(raw.getLogScaleFactors(tl.cumulative_scale_index()).copy())
    ev = {}
    if library is None:
        ev["bytes"] = raw.deviceBytes()
        ev["root_fused"] = raw.rootFusedCount()
        ev["info"] = raw.walkLaunchInfo()
        raw.kernelTimer(True)                           # one more full evaluation, counted (the compared outputs are already read)
        tl.makeDirty()
        tl.getLogLikelihood()
        ev["stats"] = raw.walkStats()
        ev["last"] = raw.walkLaunchInfo()
        ev["launches"] = raw.kernelTimer(False)[1]
    tl.close()
    return out, ev


def against_oracle(got, ref, what):
    assert site_rel(got["lnl"][0], ref["lnl"][0]) <= REL_TOL, (what, got["lnl"][0], ref["lnl"][0])
    assert site_rel(got["site"][0], ref["site"][0]) <= REL_TOL, what
    for i, (a, b) in enumerate(zip(got["parts"], ref["parts"])):
        assert norm_err(a, b) <= REL_TOL, (what, "partials", i, norm_err(a, b))
    for i, (a, b) in enumerate(zip(got["scales"], ref["scales"])):
        assert abs_rel(a, b) <= REL_TOL, (what, "scale buffer", i, abs_rel(a, b))


_memo = {}


def memo(key, fn):
    if key not in _memo:
        _memo[key] = fn()
    return _memo[key]


BASE = {"NO_SLICE_SUMS": "1"}


def default_and_oracle(shape, scheme, oracle_lib, base=BASE):
    """the default path's (under `base`) and the oracle's chain on `shape`, computed once per module"""
    wl = memo(("wl",) + shape, lambda: chain_workload(*shape))
    dflt, dev = memo(("default", shape, scheme, tuple(sorted(base.items()))), lambda: likelihood_chain(wl, scheme, dict(base)))
    ref, _ = memo(("oracle", shape, scheme), lambda: likelihood_chain(wl, scheme, {}, library=oracle_lib))
    return dflt, dev, ref


def likelihood_case(shape, scheme, env, oracle_lib):
    dflt, dev, ref = default_and_oracle(shape, scheme, oracle_lib)
    got, ev = likelihood_chain(_memo[("wl",) + shape], scheme, dict(BASE, **env))
    return got, ev, dflt, dev, ref


LIKELIHOOD4 = ["NO_LAUNCH_FUSION", "COPY_ENGINE_UPLOADS", "NO_PLAN_CACHE", "NO_WALK_FUSION", "NO_LOAD_SKIP", "NO_XCD_MAP"]


@pytest.mark.gpu
@pytest.mark.parametrize("scheme", list(SCHEMES))
@pytest.mark.parametrize("shape", SHAPES4, ids=lambda s: "S%d-T%d-P%d-C%d" % s)
@pytest.mark.parametrize("name", LIKELIHOOD4)
def test_likelihood_chain_4_states(name, shape, scheme, oracle_lib):
    """4-state switches on the likelihood chain.  Evidence: see SWITCHES[name].evidence."""
    sw = SWITCHES[name]
    got, ev, dflt, dev, ref = likelihood_case(shape, scheme, {name: sw.values[0]}, oracle_lib)
    what = (name, shape, scheme)
    same(got, dflt, sw.promise, what)
    against_oracle(got, ref, what)
    assert dev["stats"]["walks"] > 0 and ev["stats"]["walks"] > 0                  # (the 4-state walk: where these switches act)
    if name == "NO_LAUNCH_FUSION":
        assert ev["root_fused"] == 0, ev
        if scheme == "dynamic":
            assert dev["root_fused"] > 0, dev                                    # read-mode evaluations end inside the walk
    elif name == "NO_WALK_FUSION":
        assert ev["info"]["ticket_walks"] + ev["info"]["flag_walks"] == 0, ev     # one launch per wave, every time
        assert dev["info"]["ticket_walks"] + dev["info"]["flag_walks"] > 0, dev
    elif name == "NO_XCD_MAP" and shape[1] >= 400:
        # (no counter sees the grid layout; what can be seen: the launch the switch changes did run — tickets, >= 16 slices, one group)
        assert ev["info"]["ticket_walks"] > 0 and ev["last"]["slices"] >= 16, ev


@pytest.mark.gpu
@pytest.mark.parametrize("scheme", list(SCHEMES))
@pytest.mark.parametrize("shape", SHAPES_T, ids=lambda s: "S%d-T%d-P%d-C%d" % s)
def test_likelihood_chain_no_mfma(shape, scheme, oracle_lib):
    """NO_MFMA at 16..64 states: the plain-layout VALU kernels for likelihood and rescaling, to rounding of the T32 / T64 path."""
    got, ev, dflt, dev, ref = likelihood_case(shape, scheme, {"NO_MFMA": "1"}, oracle_lib)
    what = ("NO_MFMA", shape, scheme)
    same(got, dflt, "rounding", what)
    against_oracle(got, ref, what)
    assert ev["bytes"] != dev["bytes"], (ev, dev)                               # the plain layout: no 32-pattern tiles
    assert ev["stats"]["walks"] == 0 and ev["launches"] > 1, ev                  # the level kernels, a launch per tree level
    if scheme == "dynamic" or shape[0] <= 20:
        assert dev["stats"]["walks"] > 0, dev                                   # (the default's write mode at 21..64 states runs levels too)


# -- scenario 2: the gradient chain ------------------------------------------------------------------------------------------------

from beast_mcmc_amd.gradient import BranchGradient   # noqa: E402
from beast_mcmc_amd.inputs import substmodel   # noqa: E402

GRADIENT_SHAPES = {4: (4, 25, 257), 20: (2, 8, 100), 61: (1, 6, 70)}       # S -> (C, T, P): test_gradient_matches_oracle's


def gradient_workload(S):
    C_, T, P = GRADIENT_SHAPES[S]
    return helpers.random_workload(T, P, S, C_, seed=100 + S + T)


def gradient_chain(S, env, library=None, cross=False):
    """BranchGradient(double_buffer=True): three evaluations (branch lengths moved before each), the last with second derivatives and
    per-pattern values; every pre-order partial; (cross) the cross products.  -> (outputs, gradientStats, walkStats)."""
    wl = gradient_workload(S)
    with switched(env if library is None else {}):
        g = BranchGradient(wl, double_buffer=True, library=library)
    out = {"lnl": [], "grad": []}
    for step in range(3):
        g.branch_lengths *= 1.1
        r = g.gradient(second=step == 2, per_pattern=step == 2)
        out["lnl"].append(np.array([r[0]]))
        out["grad"] += [np.asarray(x, dtype=float) for x in r[1:]]
    if cross:
        out["grad"].append(np.asarray(g.cross_products(), dtype=float))
    out["parts"] = [g.pre_partials(n).reshape(wl.category_count, wl.pattern_count, S) for n in range(g.N) if n != wl.tree.root]
    stats = walk = None
    if library is None:
        stats, walk = g.b.gradientStats(), g.b.walkStats()
    g.close()
    return out, stats, walk


def gradient_against(got, ref, promise, what):
    """(promise None: the oracle, 1e-10 as test_gradient_matches_oracle)"""
    if promise == "bits":
        same(got, ref, "bits", what)
        return
    tol = REL_TOL if promise is None else 1e-13
    for a, b in zip(got["lnl"], ref["lnl"]):
        assert helpers.rel_err(float(a[0]), float(b[0])) <= tol, (what, a, b)
    for i, (a, b) in enumerate(zip(got["grad"], ref["grad"])):
        assert abs_rel(a, b) <= (REL_TOL if promise is None else 1e-11), (what, "derivatives", i, abs_rel(a, b))
    for i, (a, b) in enumerate(zip(got["parts"], ref["parts"])):
        assert norm_err(a, b) <= (REL_TOL if promise is None else 1e-12), (what, "pre-order partials", i, norm_err(a, b))


@pytest.mark.gpu
@pytest.mark.parametrize("name,S", [("NO_FUSED_GRADIENT", 4), ("NO_PRE_WALK", 4), ("NO_LAUNCH_FUSION", 4), ("NO_MFMA", 20), ("NO_MFMA", 61)])
def test_gradient_chain(name, S, oracle_lib):
    sw = SWITCHES[name]
    cross = name == "NO_MFMA"
    got, st, walk = gradient_chain(S, {name: sw.values[0]}, cross=cross)
    dflt, dst, dwalk = memo(("gradient", S, cross), lambda: gradient_chain(S, {}, cross=cross))
    ref, _, _ = memo(("gradient-oracle", S, cross), lambda: gradient_chain(S, {}, library=oracle_lib, cross=cross))
    gradient_against(got, dflt, sw.promise, (name, S))
    gradient_against(got, ref, None, (name, S))
    if name == "NO_FUSED_GRADIENT":
        assert st["by_operation"] > 0 and st["fused"] == 0 and st["walked"] == 0, st
        assert dst["fused"] > 0 and dst["by_operation"] == 0, dst
    elif name == "NO_PRE_WALK":
        assert st["walked"] == 0 and dst["walked"] > 0, (st, dst)
    elif name == "NO_MFMA":
        assert walk["walks"] == 0 and dwalk["walks"] > 0, (walk, dwalk)


# -- scenario 3: partitioned sequences (tests/test_gpu_partition_sequences.py's harness) -------------------------------------------

import test_gpu_partition_sequences as seq   # noqa: E402


def partition_sequence(S, K, env, oracle_lib, T=10):
    """updatePartialsByPartition, a whole-range root, by-partition roots, two more evaluations: every value against the oracle
    (the harness's checks) and returned for the default-path comparison."""
    c = seq.Case(S, K, oracle_lib, env={SW + k: v for k, v in dict(BASE, **env).items()}, T=T)
    out = {"lnl": [], "site": []}
    try:
        c.update_by_partition()
        v = [0.0]
        c.eng.calculateRootLogLikelihoods([c.root()], [0], [0], [NONE], 1, v)
        site = c.eng.getSiteLogLikelihoods()
        c.check_whole(v[0], site, "whole-range root")
        out["lnl"].append(np.array(v)); out["site"].append(site)
        for parts in (list(range(K)), [K - 1, 0]):
            c.update_by_partition()
            by, tot = c.root_by_partition(parts=parts)
            site = c.eng.getSiteLogLikelihoods()
            c.check_by_partition(by, tot, parts, site, "by-partition root %s" % parts)
            out["lnl"].append(np.concatenate([by, [tot]])); out["site"].append(site)
        c.further_evaluations("switch %s" % env)
        c.update_by_partition()
        by, tot = c.root_by_partition()
        out["lnl"].append(np.concatenate([by, [tot]])); out["site"].append(c.eng.getSiteLogLikelihoods())
        ev = {"info": c.eng.walkLaunchInfo(), "root_fused": c.eng.rootFusedCount()}
    finally:
        c.close()
    return out, ev


PARTITION_CASES = [(n, 4, K) for n in ["NO_LAUNCH_FUSION", "COPY_ENGINE_UPLOADS", "NO_PLAN_CACHE", "NO_WALK_FUSION", "NO_XCD_MAP"]
                   for K in (2, 3, 9)] + [("NO_MFMA", 20, K) for K in (2, 3, 9)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,S,K", PARTITION_CASES)
def test_partitioned_sequence(name, S, K, oracle_lib):
    """K = 3 leaves partition 1 without patterns (seq.LAYOUTS); K = 9 is past the eight partitions one launch finishes."""
    sw = SWITCHES[name]
    got, ev = partition_sequence(S, K, {name: sw.values[0]}, oracle_lib)
    dflt, dev = memo(("partitions", S, K), lambda: partition_sequence(S, K, {}, oracle_lib))
    same(got, dflt, sw.promise, (name, S, K))
    if name == "NO_LAUNCH_FUSION":
        assert ev["info"]["partition_roots_in_walk"] == 0 and ev["root_fused"] == 0, ev
        if K == 2:
            assert dev["info"]["partition_roots_in_walk"] > 0, dev
    elif name == "NO_WALK_FUSION":
        assert ev["info"]["ticket_walks"] + ev["info"]["flag_walks"] == 0, ev
        assert dev["info"]["ticket_walks"] + dev["info"]["flag_walks"] > 0, dev


# -- scenario 4: uploads ----------------------------------------------------------------------------------------------------------

UPLOAD_SHAPES = {4: (8, 120000, 4), 20: (8, 24000, 1)}       # S -> (T, P, C): one tip's partials just under the ring's quarter


def upload_chain(S, env, library=None):
    """Raw calls.  Three steps, each re-sending the eigen system, category rates, category weights and state frequencies, computing the
    branch matrices, overwriting one with setTransitionMatrix and reading it back, then the pruning list and the root.  Before the
    second step every tip's partials are sent again: > 16 MiB staged between two evaluations, so that the staging ring wraps."""
    T, P, C_ = UPLOAD_SHAPES[S]
    rng = np.random.default_rng(4100 + S)
    tree = helpers.random_workload(T, 50, S, C_, seed=4100 + S).tree       # (the tips get partials: only the tree is used)
    weights = rng.integers(1, 5, size=P).astype(np.float64)
    kw = {} if library is None else {"library": library}
    with switched(dict(BASE, **env) if library is None else {}):
        b = bm.beagle.Beagle(T, 2 * T - 1, 0, S, P, 1, 2 * T - 1, C_, 0, **kw)
    out = {"lnl": [], "site": [], "mats": []}
    try:
        assert T * P * S * 8 > (16 << 20) and P * S * 8 * (C_ if S > 4 else 1) <= (4 << 20)
        b.setPatternWeights(weights)
        branches = [n for n in range(2 * T - 1) if n != tree.root]
        lens = np.array([tree.branch_length(n) for n in branches])
        ops = []
        for n in tree.postorder():
            if n >= T:
                ops += [n, NONE, NONE, int(tree.left[n]), int(tree.left[n]), int(tree.right[n]), int(tree.right[n])]
        for step in range(3):
            if step <= 1:                                              # (before step 1: the ring wraps)
                for t in range(T):
                    p = rng.uniform(0.05, 1.0, size=(P, S))
                    p[rng.random(P) < 0.03] = 1.0                     # (few: a site of ambiguous tips has lnL near 0)
                    b.setTipPartials(t, np.ascontiguousarray(p))
            if S == 4:
                pi = rng.dirichlet(np.full(4, 8.0))
                eig = substmodel.gtr(rng.gamma(2.0, 1.0, size=6) + 0.1, pi)
            else:
                eig, pi = substmodel.random_reversible(S, rng)
            rates = rng.uniform(0.2, 2.0, C_)
            weights = rng.dirichlet(np.full(C_, 3.0))
            rates = rates / float(np.dot(rates, weights))
            b.setEigenDecomposition(0, eig.evec, eig.ievc, eig.evals)
            b.setCategoryRates(rates)
            b.setCategoryWeights(0, weights)
            b.setStateFrequencies(0, pi)
            b.updateTransitionMatrices(0, branches, None, None, lens * (1.0 + 0.1 * step), len(branches))
            m = rng.dirichlet(np.ones(S), size=(C_, S))
            b.setTransitionMatrix(branches[step], np.ascontiguousarray(m))
            back = b.getTransitionMatrix(branches[step])
            assert np.array_equal(back, m), step                       # the round trip, exactly
            out["mats"].append(back)
            b.updatePartials(ops, len(ops) // 7, NONE)
            v = [0.0]
            b.calculateRootLogLikelihoods([tree.root], [0], [0], [NONE], 1, v)
            out["lnl"].append(np.array(v))
            out["site"].append(b.getSiteLogLikelihoods().copy())
        ev = {"root_fused": b.rootFusedCount()} if library is None else {}
    finally:
        b.finalize()
    return out, ev


@pytest.mark.gpu
@pytest.mark.parametrize("S", [4, 20])
@pytest.mark.parametrize("name", ["COPY_ENGINE_UPLOADS", "NO_LAUNCH_FUSION"])
def test_uploads_chain(name, S, oracle_lib):
    got, ev = upload_chain(S, {name: SWITCHES[name].values[0]})
    dflt, dev = memo(("uploads", S), lambda: upload_chain(S, {}))
    ref, _ = memo(("uploads-oracle", S), lambda: upload_chain(S, {}, library=oracle_lib))
    same(got, dflt, SWITCHES[name].promise, (name, S))
    for a, b in zip(got["lnl"], ref["lnl"]):
        assert helpers.rel_err(float(a[0]), float(b[0])) <= REL_TOL, (name, S, a, b)
    for a, b in zip(got["site"], ref["site"]):
        assert site_rel(a, b) <= REL_TOL, (name, S)
    if name == "NO_LAUNCH_FUSION":
        assert ev["root_fused"] == 0, ev
        if S == 4:
            assert dev["root_fused"] > 0, dev


# -- scenario 5: the samplers on the plain layout ---------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("S,C_,T,P", [(20, 2, 8, 100), (61, 1, 6, 70)])
def test_samplers_on_the_plain_layout(S, C_, T, P):
    """NO_MFMA: the ancestral-state and Markov-jump samplers read plain-layout partials (kernels_ancestral.hip) — the bodies of
    test_gpu_ancestral.py / test_gpu_markov_jumps.py on such an instance: states and categories identical to the host restatement
    fed this instance's own partials, jump values within test_gpu_markov_jumps.py's floors."""
    import test_gpu_ancestral as ta
    import test_gpu_markov_jumps as tm
    from beast_mcmc_amd.ancestral import AncestralStateSampler
    from beast_mcmc_amd.markovjumps import MarkovJumpsSampler
    wl = helpers.random_workload(T, P, S, C_, seed=100 + S + T)
    with switched({"NO_MFMA": "1"}):
        tl = ta.make(wl, rescaling=RESCALE_DYNAMIC, delay_rescaling=True)
    try:
        tl.getLogLikelihood()
        assert helpers.walk_stats(tl)["walks"] == 0                         # (the level kernels: no T32 / T64 walk)
        sampler = AncestralStateSampler(tl)
        for use_map in (False, True):
            states, cats = ta.check_identical(tl, sampler, 2024 + S, use_map)
        assert np.array_equal(states[:T][wl.tip_states < S], wl.tip_states[wl.tip_states < S])
    finally:
        tl.close()
    wl = helpers.random_workload(T, P, S, C_, seed=300 + S + T)
    with switched({"NO_MFMA": "1"}):
        tl = tm.make(wl, branch_rate_seed=S, rescaling=RESCALE_DYNAMIC, delay_rescaling=True)
    try:
        s = tm.three_registers(MarkovJumpsSampler(tl), S, seed=S)
        for use_map in (False, True):
            res = tm.check_against_restatement(tl, s, 77 + S, use_map)
        assert np.all(res["jumps"][0] >= 0.0) and res["jumps"][0].sum() > 0.0
    finally:
        tl.close()


# -- scenario 6: the sharded handle ----------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_shard_spin_zero_gives_the_bits_of_the_default_sharded_handle(oracle_lib):
    """SHARD_SPIN_US=0 (every shard's host thread sleeps at once) on three shards: test_sharded_instance_equals_single_instance's
    chain.  Evidence: none (no counter sees a host thread sleep)."""
    g = len(bm.beagle.engine().resource_list()) - 2
    wl = helpers.random_workload(40, 3001, 4, 4, seed=901)
    runs = []
    for env in ({"SHARDS": "3", "SHARD_SPIN_US": "0"}, {"SHARDS": "3"}):
        with switched(env):
            tl = BeagleTreeLikelihood(wl, rescaling=RESCALE_DYNAMIC, delay_rescaling=False, resource_list=(g + 1,))
        vals, sites = [], []
        for step in range(3):
            if step == 2:
                tl.storeState()
                tl.set_branch_rates(np.full(wl.tree.node_count, 1.07))
            vals.append(tl.getLogLikelihood())
            sites.append(tl.getSiteLogLikelihoods().copy())
            tl.makeDirty()
        tl.close()
        runs.append((vals, sites))
    assert runs[0][0] == runs[1][0]
    for a, b in zip(runs[0][1], runs[1][1]):
        assert np.array_equal(a, b)
    o = BeagleTreeLikelihood(wl, library=oracle_lib, rescaling=RESCALE_DYNAMIC, delay_rescaling=False)
    o.storeState(); o.set_branch_rates(np.full(wl.tree.node_count, 1.07))
    assert helpers.rel_err(runs[0][0][2], o.getLogLikelihood()) <= REL_TOL
    o.close()


# -- switches read once per process: a child process per value ---------------------------------------------------------------------

_CHILD = r"""
import sys
sys.path[:0] = [%r, %r]
import numpy as np
import test_gpu_switches as ts
kind, arg, dest = sys.argv[1], sys.argv[2], sys.argv[3]
if kind == "gradient":
    out = ts.gradient_chain(int(arg), {}, cross=True)[0]
    ev = {}
else:
    out, ev = ts.likelihood_case_child(arg)
flat = {"%%s_%%d" %% (k, i): np.asarray(v) for k, vs in out.items() for i, v in enumerate(vs)}
flat.update({"ev_" + k: np.asarray(v) for k, v in ev.items()})
np.savez(dest, **flat)
print("child ok")
"""


def run_child(tmp_path, env, kind, arg):
    dest = str(tmp_path / ("%s_%s.npz" % (kind, arg)))
    full = dict(os.environ, **{SW + k: v for k, v in env.items()})
    r = subprocess.run([sys.executable, "-c", _CHILD % (ROOT, TESTS), kind, str(arg), dest], env=full, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0 and "child ok" in r.stdout, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])
    z = np.load(dest)
    out, ev = {}, {}
    for k in z.files:
        if k.startswith("ev_"):
            ev[k[3:]] = int(z[k])
            continue
        key, i = k.rsplit("_", 1)
        out.setdefault(key, {})[int(i)] = z[k]
    return {k: [v[i] for i in sorted(v)] for k, v in out.items()}, ev


@pytest.mark.gpu
@pytest.mark.parametrize("S", [20, 61])
@pytest.mark.parametrize("name,value", [("PRE_TWO_PASS", "1"), ("EDGE_TWO_STEP", "1"), ("EDGE_TWO_STEP", "2")])
def test_gradient_switch_read_once_per_process(name, value, S, tmp_path, oracle_lib):
    """PRE_TWO_PASS / EDGE_TWO_STEP=1|2 (16..64 states, to rounding) in a child process that sets the switch before anything runs;
    the parent's default path and the oracle.  Evidence: none (pre-order and edge-derivative launches are outside the kernel timer,
    gradientStats counts 4-state lists only)."""
    got, _ = run_child(tmp_path, {name: value}, "gradient", S)
    dflt, _, _ = memo(("gradient", S, True), lambda: gradient_chain(S, {}, cross=True))
    ref, _, _ = memo(("gradient-oracle", S, True), lambda: gradient_chain(S, {}, library=oracle_lib, cross=True))
    gradient_against(got, dflt, "rounding", (name, value, S))
    gradient_against(got, ref, None, (name, value, S))


RESCALE_SHAPES = [(16, 20, 33, 4), (20, 24, 129, 1), (20, 16, 2100, 3)]


def likelihood_case_child(arg):
    """(in the child) the ALWAYS chain of RESCALE_SHAPES[arg] under NO_T32_WRITE_WALK=1, with the kernel timer's evidence"""
    shape = RESCALE_SHAPES[int(arg)]
    out, ev = likelihood_chain(chain_workload(*shape), "always", dict(BASE, NO_T32_WRITE_WALK="1"))
    return out, {"walks": ev["stats"]["walks"], "launches": ev["launches"]}


@pytest.mark.gpu
@pytest.mark.parametrize("arg", range(len(RESCALE_SHAPES)))
def test_rescale_two_pass_read_once_per_process(arg, tmp_path, oracle_lib):
    """RESCALE_TWO_PASS=1 with NO_T32_WRITE_WALK=1 (every node stored: no virtual cherries, where the switch acts) against
    NO_T32_WRITE_WALK=1 alone: the same bits (prune + k_rescaleTiled is bit-identical to k_pruneTiledWrite).  Evidence:
    none for the extra launch itself (it is part of a level in the kernel timer's count); asserted: the write-mode evaluations ran
    level by level (no walk, a launch per level), which is where the switch takes effect."""
    shape = RESCALE_SHAPES[arg]
    got, ev = run_child(tmp_path, {"RESCALE_TWO_PASS": "1"}, "likelihood", arg)
    dflt, dev, ref = default_and_oracle(shape, "always", oracle_lib, base=dict(BASE, NO_T32_WRITE_WALK="1"))
    same(got, dflt, "bits", ("RESCALE_TWO_PASS", shape))
    against_oracle(got, ref, ("RESCALE_TWO_PASS", shape))
    assert ev["walks"] == 0 and ev["launches"] > 1, ev
    assert dev["stats"]["walks"] == 0 and dev["launches"] == ev["launches"], (dev, ev)
