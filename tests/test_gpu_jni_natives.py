"""The JNI natives produce the engine's numbers: every call sequence below runs three times on separate instances — through the
Java_beagle_BeagleJNIWrapper_* natives (tests/jni_env.py JniLibrary: a JNIEnv in Python, argument types from the class file's
descriptors), through the ctypes C ABI, and through the C ABI again (the control).

Where control and C ABI agree bit for bit (the suite asserts run-to-run determinism elsewhere) the natives must agree bit for bit
too, on every array read back; an output on which the control pair itself differs is held to that pair's spread and named in
SPREAD_USED (the last test prints it).  Independently, log-likelihoods, site values, partials and gradients are held to the CPU
oracle at the parity tier's 1e-10 relative; the oracle restates no ...ByPartition call, so partitioned results are compared with
one oracle instance per partition (as tests/test_gpu_multipartition.py does).

Shapes: the small ragged ones of the parity tests — pattern counts that are no multiple of 32 or 128, three or four rate
categories, 4 states and the matrix-core path's 20.  The JNI environment traps every slot it does not implement and records it;
every sequence ends by asserting that record empty.
"""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import beast_mcmc_amd as bm
import helpers
import jni_env
from beast_mcmc_amd.gradient import BranchGradient
from beast_mcmc_amd.inputs.synth import PartitionedWorkload
from beast_mcmc_amd.multipartition import MultiPartitionTreeLikelihood

pytestmark = pytest.mark.gpu
NONE = bm.beagle.NONE
REL_TOL = 1e-10
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IP, DP = C.POINTER(C.c_int), C.POINTER(C.c_double)
CALLED = set()             # natives executed by this file's sequences
SPREAD_USED = []           # (sequence, output, spread) where the control pair differed


def _ints(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def raw(b, name, *args):
    """A C ABI function / native that beagle.Beagle has no method for, through the library the instance was made with; arrays go as
    beagle.py sends them (numpy arrays behind data_as pointers)."""
    conv = [a.ctypes.data_as(IP if a.dtype == np.int32 else DP) if isinstance(a, np.ndarray) else a for a in args]
    return b.lib.fn[name](b.instance, *conv)


def three_ways(what, sequence):
    """sequence(library) -> {output: array}.  -> the natives' outputs, after the comparison with the C ABI pair."""
    eng = bm.beagle.engine()
    jni = jni_env.JniLibrary(eng)
    a = sequence(jni)
    jni.env.assert_clean()
    CALLED.update(jni.called)
    b, c = sequence(eng), sequence(eng)
    assert sorted(a) == sorted(b) == sorted(c)
    for key in sorted(b):
        x, y, z = (np.asarray(v, dtype=np.float64) for v in (a[key], b[key], c[key]))
        assert x.shape == y.shape == z.shape, (what, key)
        print("%s %s: %d values" % (what, key, y.size))
        if np.array_equal(y, z, equal_nan=True):
            assert np.array_equal(x, y, equal_nan=True), (what, key, "natives differ from the C ABI", float(np.nanmax(np.abs(x - y))))
        else:
            spread = float(np.nanmax(np.abs(y - z)))
            SPREAD_USED.append((what, key, spread))
            assert float(np.nanmax(np.abs(x - y))) <= spread, (what, key, spread)
    return a


def close(a, b, what, per_row_axes=None):
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    assert a.shape == b.shape, what
    scale = np.maximum(np.abs(b).max(axis=per_row_axes, keepdims=True) if per_row_axes else max(1.0, float(np.max(np.abs(b)))), 1e-300)
    err = float(np.max(np.abs(a - b) / scale))
    print("%s: %.3g" % (what, err))
    assert err <= REL_TOL, (what, err)


# ---- 1. likelihood chain with rescaling ---------------------------------------------------------------------------------------
def likelihood_chain(S, library):
    T, P, Cn = 8, 77, 3
    wl = helpers.random_workload(T, P, S, Cn, seed=900 + S)
    tr = wl.tree
    N, internal = tr.node_count, tr.node_count - T
    cum, copy = internal, internal + 1
    b = bm.beagle.Beagle(T, N, T, S, P, 1, N, Cn, internal + 2, library=library)
    out = {}
    try:
        for t in range(T):
            if t % 2 == 0:
                b.setTipStates(t, wl.tip_states[t])
            else:                                            # the same tip as partials: one-hot, all ones for an unknown state
                st = np.asarray(wl.tip_states[t])
                part = np.ones((P, S))
                known = st < S
                part[known] = 0.0
                part[known, st[known]] = 1.0
                b.setTipPartials(t, part.ravel())
        if "GetTipStates" in b.lib.fn:                       # (the oracle restates none)
            out["tipStates"] = b.getTipStates(0)
        b.setPatternWeights(wl.weights)
        b.setStateFrequencies(0, wl.freqs)
        b.setCategoryRates(wl.cat_rates)
        b.setCategoryWeights(0, wl.cat_weights)
        b.setEigenDecomposition(0, wl.eig.evec, wl.eig.ievc, wl.eig.evals)
        edges = [n for n in range(N) if n != tr.root]
        # BEAST's habits: the whole branchLengths[nodeCount] whatever the count, operations[] longer than the list, null
        # derivative-index arrays
        lens = np.array([tr.branch_length(n) for n in edges] + [123.0, 456.0])
        b.updateTransitionMatrices(0, _ints(edges + [0, 0]), None, None, lens, len(edges))
        order = [n for n in tr.postorder() if n >= T]
        ops = []
        for n in order:
            l, r = int(tr.left[n]), int(tr.right[n])
            ops += [n, n - T, NONE, l, l, r, r]
        b.updatePartials(_ints(ops + [0] * 7), len(order), NONE)
        if "WaitForPartials" in b.lib.fn:                    # (the oracle restates none)
            assert raw(b, "WaitForPartials", _ints([tr.root, 0]), 1) == 0
        scale = _ints([n - T for n in order] + [0, 0])
        b.resetScaleFactors(cum)
        b.accumulateScaleFactors(scale, len(order), cum)
        lnl = [0.0]
        b.calculateRootLogLikelihoods([tr.root], [0], [0], [cum], 1, lnl)
        out["lnL"] = lnl[0]
        out["site"] = b.getSiteLogLikelihoods().copy()
        out["cumulative"] = b.getLogScaleFactors(cum)
        b.removeScaleFactors(scale[2:], 3, cum)              # a subset out ...
        out["cumulative without three"] = b.getLogScaleFactors(cum)
        out["factors of one node"] = b.getLogScaleFactors(int(scale[3]))
        b.accumulateScaleFactors(scale[2:], 3, cum)          # ... and in again
        b.copyScaleFactors(copy, cum)
        out["copied"] = b.getLogScaleFactors(copy)
        b.calculateRootLogLikelihoods([tr.root], [0], [0], [copy], 1, lnl)
        out["lnL with the copied factors"] = lnl[0]
        out["root partials"] = b.getPartials(tr.root, NONE)
        out["root partials unscaled"] = b.getPartials(tr.root, cum)
        # an internal buffer uploaded with setPartials, and the operation above it run again
        child = max(int(tr.left[tr.root]), int(tr.right[tr.root]))
        assert child >= T
        stored = b.getPartials(child, NONE)
        out["child partials"] = stored
        b.setPartials(child, (stored * 0.5).ravel())
        l, r = int(tr.left[tr.root]), int(tr.right[tr.root])
        b.updatePartials(_ints([tr.root, tr.root - T, NONE, l, l, r, r]), 1, NONE)
        b.resetScaleFactors(cum)
        b.accumulateScaleFactors(scale, len(order), cum)
        b.calculateRootLogLikelihoods([tr.root], [0], [0], [cum], 1, lnl)
        out["lnL after the upload"] = lnl[0]
        out["site after the upload"] = b.getSiteLogLikelihoods().copy()
    finally:
        b.finalize()
    return out


@functools.lru_cache(maxsize=None)
def run_likelihood_chain(S):
    return three_ways("likelihood chain S=%d" % S, functools.partial(likelihood_chain, S))


@pytest.mark.parametrize("S", [4, 20])
def test_likelihood_chain_with_rescaling(S, oracle_lib):
    a = run_likelihood_chain(S)
    o = likelihood_chain(S, oracle_lib)
    assert np.array_equal(a["tipStates"], helpers.random_workload(8, 77, S, 3, seed=900 + S).tip_states[0])
    for key in ("lnL", "lnL with the copied factors", "lnL after the upload"):
        assert np.isfinite(o[key]) and helpers.rel_err(a[key], o[key]) <= REL_TOL, (key, a[key], o[key])
    weights = helpers.random_workload(8, 77, S, 3, seed=900 + S).weights
    assert helpers.rel_err(a["lnL after the upload"], a["lnL"] + float(np.sum(weights)) * np.log(0.5)) <= REL_TOL
    for key in ("site", "site after the upload"):
        assert np.max(np.abs(a[key] - o[key]) / np.abs(o[key])) <= REL_TOL, key
    # the scaled partials and the factors depend on the rescaling rule; their product does not
    close(a["root partials unscaled"], o["root partials unscaled"], "unscaled root partials", per_row_axes=(0, 2))
    close(a["copied"], a["cumulative"], "copied factors (three removed and accumulated again in between)")
    close(a["cumulative"] - a["cumulative without three"], o["cumulative"] - o["cumulative without three"], "removed factors")


# ---- 2. partitioned instance --------------------------------------------------------------------------------------------------
SIZES = [150, 77, 41]


def partitioned_workload(S):
    tree, wls = helpers.two_partitions(S, 9, SIZES, seed=60 + S)
    return PartitionedWorkload("jni-parts-S%d" % S, tree, wls)


def changed_lengths(tree):
    """partition 1 alone gets another length on one branch under the root's larger child"""
    n = max(int(tree.left[tree.root]), int(tree.right[tree.root]))
    return n, 1.7 * tree.branch_length(n)


def partitioned(S, library):
    pw = partitioned_workload(S)
    tree, T, K = pw.tree, pw.tree.tip_count, len(pw.parts)
    out = {}
    tl = MultiPartitionTreeLikelihood(pw, library=library, native_sequence=False, always_rescale=True)
    try:
        out["by partition"], out["total"] = tl.calculate()
        out["site"] = tl.getSiteLogLikelihoods().copy()
        b, cum = tl.b, T - 1
        out["cumulative"] = b.getLogScaleFactors(cum)
        some = _ints([0, 2, 3, 99])                           # scale buffers of three internal nodes (and a tail)
        assert raw(b, "RemoveScaleFactorsByPartition", some, 3, cum, 1) == 0
        out["cumulative, three removed in partition 1"] = b.getLogScaleFactors(cum)
        b.accumulateScaleFactorsByPartition(some, 3, cum, 1)
        out["cumulative restored"] = b.getLogScaleFactors(cum)
        out["second evaluation"], out["second total"] = tl.calculate()      # (the other flip of every buffer)
    finally:
        tl.close()
    tl = MultiPartitionTreeLikelihood(pw, library=library, native_sequence=False, always_rescale=False)
    try:
        out["unscaled by partition"], out["unscaled total"] = tl.calculate()
        # a subset of the partitions updated alone: partition 1's matrix of one branch, its operation at the root
        b, k = tl.b, 1
        n, t = changed_lengths(tree)
        b.updateTransitionMatricesWithMultipleModels([k], [k], [tl.mbuf(k, n)], None, None, [t], 1)
        root = tree.root
        l, r = int(tree.left[root]), int(tree.right[root])
        ops = [tl.pbuf(root), NONE, NONE, tl.pbuf(l), tl.mbuf(k, l), tl.pbuf(r), tl.mbuf(k, r), k, NONE]
        b.updatePartialsByPartition(_ints(ops + [0] * 9), 1)
        byp, tot = np.full(K + 2, -5.5), [0.0]                 # per-partition outputs: K * count entries of a longer array
        b.calculateRootLogLikelihoodsByPartition([tl.pbuf(root)] * K, list(range(K)), list(range(K)), [NONE] * K, list(range(K)), K, 1, byp, tot)
        assert np.all(byp[K:] == -5.5)
        out["after partition 1 moved"], out["total after partition 1 moved"] = byp[:K].copy(), tot[0]
        one, tot1 = np.zeros(1), [0.0]                          # ... and that partition's root alone
        b.calculateRootLogLikelihoodsByPartition([tl.pbuf(root)], [k], [k], [NONE], [k], 1, 1, one, tot1)
        out["partition 1 alone"] = np.array([one[0], tot1[0]])
        out["site after partition 1 moved"] = tl.getSiteLogLikelihoods().copy()
    finally:
        tl.close()
    return out


def oracle_partition(w, tree, library, lengths=None):
    """One partition on an oracle instance of its own, single-partition protocol -> (lnL, site values)."""
    T, N = tree.tip_count, tree.node_count
    b = bm.beagle.Beagle(T, N, T, w.state_count, w.pattern_count, 1, N, w.category_count, 0, library=library)
    try:
        for t in range(T):
            b.setTipStates(t, w.tip_states[t])
        b.setPatternWeights(w.weights); b.setStateFrequencies(0, w.freqs)
        b.setCategoryRates(w.cat_rates); b.setCategoryWeights(0, w.cat_weights)
        b.setEigenDecomposition(0, w.eig.evec, w.eig.ievc, w.eig.evals)
        edges = [n for n in range(N) if n != tree.root]
        lens = [tree.branch_length(n) for n in edges]
        for n, t in (lengths or {}).items():
            lens[edges.index(n)] = t
        b.updateTransitionMatrices(0, edges, None, None, lens, len(edges))
        ops = []
        for n in tree.postorder():
            if n >= T:
                l, r = int(tree.left[n]), int(tree.right[n])
                ops += [n, NONE, NONE, l, l, r, r]
        b.updatePartials(ops, len(ops) // 7, NONE)
        lnl = [0.0]
        b.calculateRootLogLikelihoods([tree.root], [0], [0], [NONE], 1, lnl)
        return lnl[0], b.getSiteLogLikelihoods().copy()
    finally:
        b.finalize()


@functools.lru_cache(maxsize=None)
def run_partitioned(S):
    return three_ways("partitioned S=%d" % S, functools.partial(partitioned, S))


@pytest.mark.parametrize("S", [4, 20])
def test_partitioned_instance(S, oracle_lib):
    a = run_partitioned(S)
    pw = partitioned_workload(S)
    expect = [oracle_partition(w, pw.tree, oracle_lib) for w in pw.parts]
    lnl = np.array([e[0] for e in expect])
    sites = np.concatenate([e[1] for e in expect])
    for key in ("by partition", "second evaluation", "unscaled by partition"):
        close(a[key], lnl, key)
    for key in ("total", "second total", "unscaled total"):
        assert helpers.rel_err(a[key], float(lnl.sum())) <= REL_TOL, key
    assert np.max(np.abs(a["site"] - sites) / np.abs(sites)) <= REL_TOL
    n, t = changed_lengths(pw.tree)
    moved = oracle_partition(pw.parts[1], pw.tree, oracle_lib, lengths={n: t})
    lnl2 = lnl.copy(); lnl2[1] = moved[0]
    assert helpers.rel_err(moved[0], lnl[1]) > 1e-6                      # (the move is one)
    close(a["after partition 1 moved"], lnl2, "after partition 1 moved")
    assert helpers.rel_err(a["total after partition 1 moved"], float(lnl2.sum())) <= REL_TOL
    close(a["partition 1 alone"], [moved[0], moved[0]], "partition 1 alone")
    sites2 = np.concatenate([expect[0][1], moved[1], expect[2][1]])
    assert np.max(np.abs(a["site after partition 1 moved"] - sites2) / np.abs(sites2)) <= REL_TOL
    # removing three nodes' factors in partition 1 touches that partition's pattern range only, and accumulating restores it
    d = a["cumulative"] - a["cumulative, three removed in partition 1"]
    lo, hi = SIZES[0], SIZES[0] + SIZES[1]
    assert np.all(d[:lo] == 0) and np.all(d[hi:] == 0) and np.any(d[lo:hi] != 0)
    close(a["cumulative restored"], a["cumulative"], "cumulative factors restored")


# ---- 3. gradients -------------------------------------------------------------------------------------------------------------
def gradient(S, rescale, library):
    wl = helpers.random_workload(9, 77, S, 3, seed=700 + S)
    g = BranchGradient(wl, rescale=rescale, library=library)
    out = {}
    try:
        b, root = g.b, wl.tree.root
        out["lnL"], out["gradient"] = g.gradient()                           # null outDerivatives, null outSumSquaredDerivatives
        lnl, grad, hess, per = g.gradient(second=True, per_pattern=True)     # outDerivatives: count * P entries
        out["lnL again"], out["gradient again"], out["second derivatives"], out["per pattern"] = lnl, grad, hess, per
        out["cross products"] = g.cross_products()
        nodes = np.asarray(g.edges, dtype=np.int32)
        filled = 0.125 * np.arange(1, S * S + 1)                              # pre-filled sums: the call adds to them
        acc = filled.copy()
        b.calculateCrossProductDifferentials(g._edge_post[0], nodes + g.pre_offset, [0], [0], g.branch_lengths[nodes], len(nodes), out=acc)
        out["cross products added"] = acc - filled
        # the root's pre-order partial from setRootPrePartials, and the pre-order list run again below it
        b.setPartials(g.pre_offset + root, np.zeros(g.C * g.P * g.S))
        b.setRootPrePartials([g.pre_offset + root, 0], [0, 0], 1)
        out["root pre-order partial"] = b.getPartials(g.pre_offset + root, NONE)
        b.updatePrePartials(_ints(list(g._pre_ops) + [0] * 7), len(g._pre_ops) // 7, NONE)
        out["pre-order partials"] = np.stack([g.pre_partials(n) for n in g.edges[:4]])
        # matrices: transposed copies, sums (the gradient delegates' transposeTransitionMatrices / addTransitionMatrices)
        m0, m1 = b.getTransitionMatrix(int(nodes[0])).copy(), b.getTransitionMatrix(int(nodes[1])).copy()
        b.transposeTransitionMatrices(_ints([nodes[0], nodes[1], 0]), _ints([g.q_index, g.q2_index, 0]), 2)
        out["transposed"] = np.stack([b.getTransitionMatrix(g.q_index), b.getTransitionMatrix(g.q2_index)])
        assert np.array_equal(out["transposed"], np.stack([m0.transpose(0, 2, 1), m1.transpose(0, 2, 1)]))
        if "AddTransitionMatrices" in b.lib.fn:                                # (the oracle restates none)
            b.addTransitionMatrices(_ints([nodes[0], 0]), _ints([nodes[1], 0]), _ints([g.q_index, 0]), 1)
            out["added"] = b.getTransitionMatrix(g.q_index)
            assert np.array_equal(out["added"], m0 + m1)
    finally:
        g.close()
    return out


@functools.lru_cache(maxsize=None)
def run_gradient(S, rescale):
    return three_ways("gradient S=%d rescale=%s" % (S, rescale), functools.partial(gradient, S, rescale))


@pytest.mark.parametrize("rescale", [False, True])
@pytest.mark.parametrize("S", [4, 20])
def test_gradient(S, rescale, oracle_lib):
    a = run_gradient(S, rescale)
    o = gradient(S, rescale, oracle_lib)
    for key in ("lnL", "lnL again"):
        assert helpers.rel_err(a[key], o[key]) <= REL_TOL, key
    for key in ("gradient", "gradient again", "second derivatives", "per pattern", "cross products", "cross products added"):
        close(a[key], o[key], key)
    close(a["cross products added"], a["cross products"].ravel(), "the sums are added to what the array held")
    wl = helpers.random_workload(9, 77, S, 3, seed=700 + S)
    assert np.array_equal(a["root pre-order partial"], np.tile(wl.freqs, 77 * 3).reshape(3, 77, S))
    close(a["pre-order partials"], o["pre-order partials"], "pre-order partials", per_row_axes=(1, 3))


def pre_order_by_partition(S, library):
    """updatePrePartialsByPartition (9-int tuples): three unequal partitions of one instance, set with setPatternPartitions as
    tests/test_gpu_gradients.py does; the partitions' lists together leave what the whole-range list leaves."""
    wl = helpers.random_workload(9, 77, S, 3, seed=700 + S)
    g = BranchGradient(wl, library=library)
    out = {}
    try:
        parts = np.zeros(g.P, dtype=np.int32); parts[30:41] = 1; parts[41:] = 2
        g.b.setPatternPartitions(3, parts)
        g.gradient()
        out["whole range"] = np.stack([g.pre_partials(n) for n in g.edges])
        for n in g.edges:
            g.b.setPartials(g.pre_offset + n, np.zeros(g.C * g.P * g.S))
        ops7 = g._pre_ops.reshape(-1, 7)
        ops9 = np.concatenate([np.concatenate([ops7, np.full((len(ops7), 1), k, dtype=np.int32), np.full((len(ops7), 1), NONE, dtype=np.int32)], axis=1)
                               for k in (2, 0, 1)]).astype(np.int32)
        g.b.updatePrePartialsByPartition(_ints(list(ops9.ravel()) + [0] * 9), len(ops9))
        out["by partition"] = np.stack([g.pre_partials(n) for n in g.edges])
    finally:
        g.close()
    return out


@functools.lru_cache(maxsize=None)
def run_pre_order_by_partition(S):
    return three_ways("pre-order by partition S=%d" % S, functools.partial(pre_order_by_partition, S))


@pytest.mark.parametrize("S", [4, 20])
def test_pre_order_partials_by_partition(S, oracle_lib):
    a = run_pre_order_by_partition(S)
    assert np.array_equal(a["by partition"], a["whole range"])
    wl = helpers.random_workload(9, 77, S, 3, seed=700 + S)
    o = BranchGradient(wl, library=oracle_lib)
    o.gradient()
    close(a["whole range"], np.stack([o.pre_partials(n) for n in o.edges]), "pre-order partials", per_row_axes=(1, 3))
    o.close()


# ---- 4. matrices and the rest -------------------------------------------------------------------------------------------------
def matrices(library):
    S, P, Cn = 4, 5, 3
    rng = np.random.default_rng(44)
    b = bm.beagle.Beagle(2, 3, 2, S, P, 1, 4, Cn, 0, library=library)
    out = {}
    try:
        m = rng.random(Cn * S * S)
        b.setTransitionMatrix(2, np.concatenate([m, [-1.0, -2.0]]), 0.75)      # (a longer array; a padded value other than the default)
        back = np.full(Cn * S * S + 2, -3.0)
        assert raw(b, "GetTransitionMatrix", 2, back) == 0
        assert np.all(back[-2:] == -3.0)
        out["matrix"] = back[:-2].copy()
        assert np.array_equal(out["matrix"], m)
        if "SetCPUThreadCount" in b.lib.fn:                                    # (the oracle restates none)
            b.setCPUThreadCount(3)
    finally:
        b.finalize()
    return out


@functools.lru_cache(maxsize=None)
def run_matrices():
    from test_oracle_golden import run_epoch_convolution
    a = three_ways("matrices", matrices)
    b = three_ways("epoch convolution", lambda library: {"lnL": run_epoch_convolution(library)[0]})
    return a, b


def test_matrices_convolution_and_strings(oracle_lib):
    from test_oracle_golden import run_epoch_convolution
    _, conv = run_matrices()
    lnl, g = run_epoch_convolution(oracle_lib)
    assert abs(conv["lnL"] - g["lnL"]) < 1e-5                                  # the bound test_golden_epoch_convolution pins
    assert helpers.rel_err(conv["lnL"], lnl) <= REL_TOL
    eng = bm.beagle.engine()
    jni = jni_env.JniLibrary(eng)
    for native, function in (("getVersion", "beagleGetVersion"), ("getCitation", "beagleGetCitation")):
        f = getattr(eng.lib, function)
        f.restype = C.c_char_p
        assert jni.call(native) == f().decode() != ""
    assert jni.version == eng.version
    # calculateEdgeDerivative: declared by the class file, no caller in the reference, refused by the wrapper
    ints, dbls = np.zeros(4, dtype=np.int32), np.zeros(4)
    assert jni.call("calculateEdgeDerivative", 0, ints, ints, 1, ints, ints, 1, 1, 1, ints, 1, dbls, dbls) == -7
    jni.env.assert_clean()
    CALLED.update(jni.called)


# ---- the coverage gate --------------------------------------------------------------------------------------------------------
def test_every_native_is_executed_by_a_jni_test():
    """All 47 natives of the class file are executed by the JNI tests — this file, tests/test_jni_marshalling.py and the C++
    driver tests/native/fake_jvm.cpp — and this file alone executes all but the two that build Java objects through variadic
    slots.  A condition, not a measurement: nothing is exempt."""
    import test_jni_marshalling as marshalling
    for S in (4, 20):
        run_likelihood_chain(S); run_partitioned(S); run_pre_order_by_partition(S)
        for rescale in (False, True):
            run_gradient(S, rescale)
    run_matrices()
    test_matrices_convolution_and_strings(helpers.oracle_library())
    natives = set(jni_env.natives())
    assert len(natives) == 47
    driver = set(re.findall(r'sym<[^;]*?>\s*\(\s*"(\w+)"\s*\)', open(os.path.join(ROOT, "tests", "native", "fake_jvm.cpp")).read()))
    assert {"getResourceList", "getBenchmarkedResourceList"} <= driver <= natives
    assert CALLED | set(marshalling.MARSHALLED) | set(marshalling.OTHERS) | driver == natives
    assert natives - CALLED == {"getResourceList", "getBenchmarkedResourceList"}, sorted(natives - CALLED)
    print("outputs held to the control pair's spread instead of bit equality: %r" % (SPREAD_USED,))
