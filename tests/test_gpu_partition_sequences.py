"""Whole-range calls on partitioned instances, and by-partition calls in the orders BEAST does not use, against the CPU oracle.

BEAST's partitioned caller (MultiPartitionDataLikelihoodDelegate) issues only the ...ByPartition entry points; the BEAGLE contract
defines the whole-range ones (7-int updatePartials, accumulate/removeScaleFactors, calculateRootLogLikelihoods and the engine's
device-side root) over every pattern of an instance with any number of partitions.  Each sequence here is checked after every
root call and is followed by two ordinary by-partition evaluations (branch lengths changed), also checked: what a call leaves
behind on the instance (the root sum's last-workgroup counter, a held walk, a ticket word) shows up there.

Expected values: one oracle instance per partition (its own model), through the single-partition protocol; a whole-range sum is
their sum and its site values their concatenation.  A whole-range list with ONE model is checked against one unpartitioned oracle
instance (tests/test_multipartition_host.py checks that the two references agree).  1e-10 relative on every value; two engine
paths that must agree do so bit for bit."""
import os

import numpy as np
import pytest

import beast_mcmc_amd as bm
import helpers
from beast_mcmc_amd.inputs.synth import Workload

pytestmark = pytest.mark.gpu
NONE = bm.beagle.NONE

# partition sizes: none a multiple of 128 (the 4-state pattern groups) or 32 (the T32 tiles) but the one 64 / 128-straddling mix of K = 9;
# K = 3 leaves partition 1 without patterns; K = 9 is past the eight partitions one launch finishes (kernels.h ROOT_MAX_PARTS)
LAYOUTS = {2: ([150, 77], [0, 1]), 3: ([130, 97], [0, 2]), 9: ([37, 5, 130, 64, 1, 77, 33, 129, 20], list(range(9)))}
# ... and 80 states, past the walks: the level path (K = 2 and 3)
SHAPES_WITH_LEVELS = [(S, K) for S in (4, 20, 61) for K in (2, 3, 9)] + [(80, 2), (80, 3)]


def site_rel(a, b):
    return float(np.max(np.abs(a - b) / np.abs(b))) if len(b) else 0.0


class Case:
    """One engine instance with K partitions (each its own eigen system and category rates) and per-partition buffer sets (BEAST's partialBufferHelper[i]: set j holds internal
    node n at T + j (T - 1) + n - T), one oracle instance per non-empty partition, and — shared_model — one unpartitioned oracle
    instance over all patterns.  env: BEAGLE_MI355_* switches in force while the engine instance is created (tests/test_gpu_switches.py)."""

    def __init__(self, S, K, oracle_lib, scaling=False, seed=0, shared_model=False, sizes=None, ids=None, resource=(1,), T=10, C=4, env=None):
        sizes, ids = (sizes, ids) if sizes is not None else LAYOUTS[K]
        self.tree, wls = helpers.two_partitions(S, T, sizes, seed=seed + 31 * S + K, categories=C)
        # every partition integrates its root with the same category weights and state frequencies (a whole-range root call names
        # one set of them for all patterns); the substitution models and category rates are the partitions' own unless shared_model
        m = wls[0]
        wls = [Workload(w.name, w.tree, m.eig if shared_model else w.eig, m.freqs, m.cat_rates if shared_model else w.cat_rates,
                        m.cat_weights, w.tip_states, w.weights, S) for w in wls]
        self.S, self.K, self.T, self.C, self.wls, self.ids, self.scaling = S, K, T, C, wls, ids, scaling
        self.nodes = 2 * T - 1
        self.internal = [n for n in self.tree.postorder() if n >= T]
        self.branches = [n for n in range(self.nodes) if n != self.tree.root]
        self.lens = np.array([self.tree.branch_length(n) if n != self.tree.root else 0.0 for n in range(self.nodes)])
        self.P = sum(w.pattern_count for w in wls)
        self.ranges = {}
        off = 0
        for k, w in zip(ids, wls):
            self.ranges[k] = (off, off + w.pattern_count)
            off += w.pattern_count
        self.cum = T - 1                                        # scale buffers: 0..T-2 per node, T-1 and T cumulative
        old = {k: os.environ.get(k) for k in (env or {})}
        os.environ.update(env or {})
        try:
            self.eng = bm.beagle.Beagle(T, T + K * (T - 1), T, S, self.P, K, K * self.nodes, C, T + 1, resourceList=resource)
        finally:
            for k, v in old.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v
        self.ora = [bm.beagle.Beagle(T, 2 * T - 1, T, S, w.pattern_count, 1, self.nodes, C, T + 1, library=oracle_lib) for w in wls]
        self.whole = bm.beagle.Beagle(T, 2 * T - 1, T, S, self.P, 1, self.nodes, C, T + 1, library=oracle_lib) if shared_model else None
        e = self.eng
        for t in range(T):
            e.setTipStates(t, np.concatenate([w.tip_states[t] for w in wls]))
            for o, w in zip(self.ora, wls):
                o.setTipStates(t, w.tip_states[t])
            if self.whole:
                self.whole.setTipStates(t, np.concatenate([w.tip_states[t] for w in wls]))
        e.setPatternWeights(np.concatenate([w.weights for w in wls]))
        e.setPatternPartitions(K, np.concatenate([np.full(w.pattern_count, k, dtype=np.int32) for k, w in zip(ids, wls)]))
        for k in range(K):                                      # (an empty partition gets the first model: its indices must be valid)
            w = wls[ids.index(k)] if k in ids else wls[0]
            e.setEigenDecomposition(k, w.eig.evec, w.eig.ievc, w.eig.evals)
            e.setCategoryRatesWithIndex(k, w.cat_rates)
            e.setCategoryWeights(k, w.cat_weights)
            e.setStateFrequencies(k, w.freqs)
        for o, w in zip(self.ora + ([self.whole] if self.whole else []), wls + ([wls[0]] if self.whole else [])):
            if o is self.whole:
                o.setPatternWeights(np.concatenate([x.weights for x in wls]))
            else:
                o.setPatternWeights(w.weights)
            o.setEigenDecomposition(0, w.eig.evec, w.eig.ievc, w.eig.evals)
            o.setCategoryRates(w.cat_rates)
            o.setCategoryWeights(0, w.cat_weights)
            o.setStateFrequencies(0, w.freqs)
        self.matrices(1.0)

    def close(self):
        for b in [self.eng] + self.ora + ([self.whole] if self.whole else []):
            b.finalize()

    def buf(self, j, n):
        return n if n < self.T else self.T + j * (self.T - 1) + (n - self.T)

    def root(self, j=0):
        return self.buf(j, self.tree.root)

    def matrices(self, factor):
        K, L = self.K, [self.lens[n] * factor for n in self.branches]
        self.eng.updateTransitionMatricesWithMultipleModels([k for k in range(K) for _ in self.branches], [k for k in range(K) for _ in self.branches],
                                                            [k * self.nodes + n for k in range(K) for n in self.branches], None, None, L * K, K * len(L))
        for o in self.ora + ([self.whole] if self.whole else []):
            o.updateTransitionMatrices(0, self.branches, None, None, L, len(L))

    def ops(self, k, j, write, model=None):
        """partition k's post-order list into buffer set j (9-int) and the oracle's 7-int list (buffer set 0)"""
        m = k if model is None else model
        e9, o7 = [], []
        for n in self.internal:
            l, r = int(self.tree.left[n]), int(self.tree.right[n])
            ws = n - self.T if write else NONE
            e9 += [self.buf(j, n), ws, NONE, self.buf(j, l), m * self.nodes + l, self.buf(j, r), m * self.nodes + r, k, NONE]
            o7 += [n, ws, NONE, l, l, r, r]
        return e9, o7

    def update_by_partition(self, sets=None):
        """every partition's post-order list, node by node (partition fastest: the delegate's order), rescaling in write mode when
        scaling; partition k into buffer set sets[k] (default 0).  The oracles evaluate their partitions into set 0."""
        sets = sets or [0] * self.K
        per = [self.ops(k, sets[k], self.scaling)[0] for k in range(self.K)]
        e9 = [x for i in range(len(self.internal)) for k in range(self.K) for x in per[k][9 * i:9 * i + 9]]
        self.eng.updatePartialsByPartition(e9, len(e9) // 9)
        for i, o in enumerate(self.ora):
            o7 = self.ops(self.ids[i], 0, self.scaling)[1]
            o.updatePartials(o7, len(o7) // 7, NONE)
            if self.scaling:
                o.resetScaleFactors(self.cum)
                o.accumulateScaleFactors([n - self.T for n in self.internal], len(self.internal), self.cum)

    def accumulate_by_partition(self):
        if self.scaling:
            for k in range(self.K):
                self.eng.resetScaleFactorsByPartition(self.cum, k)
                self.eng.accumulateScaleFactorsByPartition([n - self.T for n in self.internal], len(self.internal), self.cum, k)

    def cum_or_none(self):
        return self.cum if self.scaling else NONE

    def expected(self):
        """per oracle partition: (lnL, site values)"""
        out = []
        for o in self.ora:
            v = [0.0]
            o.calculateRootLogLikelihoods([self.tree.root], [0], [0], [self.cum_or_none()], 1, v)
            out.append((v[0], o.getSiteLogLikelihoods()))
        return out

    def check_whole(self, total, site, what):
        exp = self.expected()
        want = sum(v for v, _ in exp)
        assert helpers.rel_err(total, want) <= 1e-10, (what, total, want)
        want_site = np.concatenate([s for _, s in exp])
        assert site_rel(site, want_site) <= 1e-10, what

    def root_by_partition(self, parts=None, sets=None, cum=None):
        parts = list(range(self.K)) if parts is None else parts
        sets = sets or [0] * len(parts)
        c = self.cum_or_none() if cum is None else cum
        by, tot = np.zeros(len(parts)), [0.0]
        self.eng.calculateRootLogLikelihoodsByPartition([self.root(j) for j in sets], parts, parts, [c] * len(parts), parts, len(parts), 1, by, tot)
        return by, tot[0]

    def check_by_partition(self, by, total, parts, site, what):
        exp = self.expected()
        for i, k in enumerate(parts):
            want = exp[self.ids.index(k)][0] if k in self.ids else 0.0
            assert (by[i] == 0.0) if k not in self.ids else helpers.rel_err(by[i], want) <= 1e-10, (what, k, by[i], want)
            if k in self.ids:
                a, b = self.ranges[k]
                assert site_rel(site[a:b], exp[self.ids.index(k)][1]) <= 1e-10, (what, k)
        assert helpers.rel_err(total, float(np.sum(by))) <= 1e-13, what

    def further_evaluations(self, what):
        """two ordinary by-partition evaluations (BEAST's), branch lengths changed each time"""
        for i, f in enumerate((1.07, 0.93)):
            self.matrices(f)
            self.update_by_partition()
            self.accumulate_by_partition()
            by, tot = self.root_by_partition()
            self.check_by_partition(by, tot, list(range(self.K)), self.eng.getSiteLogLikelihoods(), "%s, then evaluation %d" % (what, i))
        self.matrices(1.0)


class device_doubles:
    """n zeroed doubles in device memory (the HIP runtime the engine links), for the device-side root call"""

    def __init__(self, n):
        import ctypes as C
        rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
        self.C, self.n = C, n
        self.hip = C.CDLL(os.path.join(rocm, "lib", "libamdhip64.so"))
        p = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(p), C.c_size_t(8 * n)) == 0
        self.ptr = p.value
        assert self.hip.hipMemset(C.c_void_p(self.ptr), 0, C.c_size_t(8 * n)) == 0
        assert self.hip.hipDeviceSynchronize() == 0

    def read(self):
        out = np.zeros(self.n)
        assert self.hip.hipMemcpy(out.ctypes.data_as(self.C.c_void_p), self.C.c_void_p(self.ptr), self.C.c_size_t(8 * self.n), 2) == 0   # device to host
        return out

    def free(self):
        self.hip.hipFree(self.C.c_void_p(self.ptr))


def roots_in_walk(case):
    return case.eng.walkLaunchInfo()["partition_roots_in_walk"]


def fused_by_partition_expected(case):
    """by-partition roots that must be finished inside the walk's launch: 4 states, no write-mode rescaling (whose accumulation
    launches the walk first), all partitions non-empty and at most eight of them"""
    return case.S == 4 and not case.scaling and case.K == 2


@pytest.mark.parametrize("scaling", [False, True])
@pytest.mark.parametrize("K", [2, 3, 9])
@pytest.mark.parametrize("S", [4, 20, 61])
def test_whole_range_root_right_behind_a_by_partition_walk(S, K, scaling, oracle_lib):
    """Sequence 1: updatePartialsByPartition (held back on a 4-state instance) -> calculateRootLogLikelihoods over all patterns on the
    shared root buffer: the sum of the partitions' values, their site values in a row — then through the device-side root call."""
    c = Case(S, K, oracle_lib, scaling=scaling)
    try:
        for via_device in (False, True):
            c.update_by_partition()
            c.accumulate_by_partition()
            fused0 = c.eng.rootFusedCount()
            if via_device:
                out = device_doubles(2)
                try:
                    c.eng.calculateRootLogLikelihoodsDevice(c.root(), 0, 0, c.cum_or_none(), out.ptr)
                    c.eng.synchronize()
                    got = out.read()
                finally:
                    out.free()
                total = float(got[0])
                assert got[1] == 0.0                              # (one value written, nothing behind it)
            else:
                v = [0.0]
                c.eng.calculateRootLogLikelihoods([c.root()], [0], [0], [c.cum_or_none()], 1, v)
                total = v[0]
            assert c.eng.rootFusedCount() == fused0          # (no partition's slice covers [0, P): the walk goes out as it is)
            c.check_whole(total, c.eng.getSiteLogLikelihoods(), "whole-range root, device %s" % via_device)
            before = roots_in_walk(c)
            c.further_evaluations("whole-range root, device %s" % via_device)
            if fused_by_partition_expected(c):
                assert roots_in_walk(c) == before + 2
    finally:
        c.close()


@pytest.mark.parametrize("shards", ["2"])
def test_whole_range_root_on_a_partitioned_sharded_handle(shards, oracle_lib, monkeypatch):
    """Sequence 1 on the pattern-sharded handle (resource G+1, two shards on one device: tests/test_gpu_sharded_instance.py): every
    shard holds some partitions' patterns; the whole-range sum is the shards' sums added."""
    monkeypatch.setenv("BEAGLE_MI355_SHARDS", shards)
    g = len(bm.beagle.engine().resource_list()) - 2
    c = Case(4, 3, oracle_lib, sizes=[300, 77, 140], ids=[0, 1, 2], resource=(g + 1,))
    try:
        c.update_by_partition()
        v = [0.0]
        c.eng.calculateRootLogLikelihoods([c.root()], [0], [0], [NONE], 1, v)
        c.check_whole(v[0], c.eng.getSiteLogLikelihoods(), "sharded whole-range root")
        c.further_evaluations("sharded whole-range root")
    finally:
        c.close()


@pytest.mark.parametrize("K", [2, 3, 9])
@pytest.mark.parametrize("S", [4, 20])
def test_per_partition_root_buffers_then_a_whole_range_root(S, K, oracle_lib):
    """Sequence 2: every partition evaluated into its OWN buffer set, the by-partition root names each partition's root buffer
    (finished inside the walk on 4 states); then all partitions into set 0 and a whole-range root on that set's root buffer."""
    c = Case(S, K, oracle_lib)
    try:
        before = roots_in_walk(c)
        c.update_by_partition(sets=list(range(K)))
        by, tot = c.root_by_partition(sets=list(range(K)))
        c.check_by_partition(by, tot, list(range(K)), c.eng.getSiteLogLikelihoods(), "own buffer sets")
        if fused_by_partition_expected(c):
            assert roots_in_walk(c) == before + 1
        c.update_by_partition()
        v = [0.0]
        c.eng.calculateRootLogLikelihoods([c.root(0)], [0], [0], [NONE], 1, v)
        c.check_whole(v[0], c.eng.getSiteLogLikelihoods(), "whole-range root on buffer set 0")
        c.further_evaluations("per-partition buffer sets")
    finally:
        c.close()


@pytest.mark.parametrize("K", [2, 3, 9])
@pytest.mark.parametrize("S", [4, 61])
def test_root_by_partition_naming_a_subset_permuted_and_twice(S, K, oracle_lib):
    """Sequence 3: right behind a held walk, a by-partition root that names some of the partitions, in another order, one of them
    twice: each named value is that partition's, the total their sum (the twice-named one counted twice)."""
    c = Case(S, K, oracle_lib)
    try:
        for parts in ([K - 1, 0], [K - 1, 0, K - 1], [1] if K > 2 else [1, 1]):
            c.update_by_partition()
            by, tot = c.root_by_partition(parts=parts)
            c.check_by_partition(by, tot, parts, c.eng.getSiteLogLikelihoods(), "subset %s" % parts)
        c.further_evaluations("subsets")
    finally:
        c.close()


def whole_checks(c, what):
    """whole-range roots on the shared root buffer (every cumulative buffer in use) and the root's partials: the unpartitioned
    oracle instance's"""
    for ci in ((c.cum, c.cum + 1) if c.scaling else (NONE,)):
        v, w = [0.0], [0.0]
        c.eng.calculateRootLogLikelihoods([c.root()], [0], [0], [ci], 1, v)
        site = c.eng.getSiteLogLikelihoods()
        c.whole.calculateRootLogLikelihoods([c.tree.root], [0], [0], [ci], 1, w)
        assert helpers.rel_err(v[0], w[0]) <= 1e-10, (what, ci, v[0], w[0])
        assert site_rel(site, c.whole.getSiteLogLikelihoods()) <= 1e-10, (what, ci)
    pe, po = c.eng.getPartials(c.root(), NONE), c.whole.getPartials(c.tree.root, NONE)
    scale = np.maximum(np.abs(po).max(axis=(0, 2), keepdims=True), 1e-300)
    assert np.max(np.abs(pe - po) / scale) <= 1e-10, what
    return v[0], site


def whole_scale_calls(c, b):
    """whole-range reset / accumulate / remove / accumulate again into the second cumulative buffer"""
    if c.scaling:
        idx = [n - c.T for n in c.internal]
        b.resetScaleFactors(c.cum + 1)
        b.accumulateScaleFactors(idx, len(idx), c.cum + 1)
        b.removeScaleFactors(idx[:3], 3, c.cum + 1)
        b.accumulateScaleFactors(idx[:3], 3, c.cum + 1)


@pytest.mark.parametrize("scaling", [False, True])
@pytest.mark.parametrize("S,K", SHAPES_WITH_LEVELS)
def test_whole_range_list_on_a_partitioned_instance_is_the_unpartitioned_evaluation(S, K, scaling, oracle_lib):
    """Sequence 4, one model for every partition: a 7-int updatePartials (the cumulative index on the call when scaling), the
    whole-range scale calls and whole-range roots — one unpartitioned oracle instance given the same calls.  The 7-int list and the
    same list written as 9-int tuples (each operation once per non-empty partition) give the same bits.  80 states: the level path."""
    c = Case(S, K, oracle_lib, scaling=scaling, shared_model=True)
    cum = c.cum if scaling else NONE
    o7 = c.ops(0, 0, scaling)[1]
    try:
        for b in (c.eng, c.whole):
            if scaling:
                b.resetScaleFactors(c.cum)
            b.updatePartials(o7, len(o7) // 7, cum)
            whole_scale_calls(c, b)
        v7, s7 = whole_checks(c, "7-int list")
        d = Case(S, K, oracle_lib, scaling=scaling, shared_model=True)
        try:
            if scaling:
                d.eng.resetScaleFactors(c.cum)
            e9 = []
            for i in range(len(c.internal)):
                for k in range(K):
                    if k in c.ids:
                        e9 += o7[7 * i:7 * i + 7] + [k, cum]
            d.eng.updatePartialsByPartition(e9, len(e9) // 9)
            whole_scale_calls(d, d.eng)
            v9 = [0.0]
            d.eng.calculateRootLogLikelihoods([d.root()], [0], [0], [c.cum + 1 if scaling else NONE], 1, v9)
            assert v9[0] == v7 and np.array_equal(d.eng.getSiteLogLikelihoods(), s7)
        finally:
            d.close()
        c.further_evaluations("7-int list")
    finally:
        c.close()


@pytest.mark.parametrize("S,K", SHAPES_WITH_LEVELS)
def test_whole_range_scale_calls_on_a_partitioned_instance(S, K, oracle_lib):
    """Sequence 4, the scale calls alone: a by-partition list rescaling in write mode (every partition, one model), then
    whole-range reset / accumulate / remove into the cumulative buffers and whole-range roots — the unpartitioned oracle instance."""
    c = Case(S, K, oracle_lib, scaling=True, shared_model=True)
    idx = [n - c.T for n in c.internal]
    o7 = c.ops(0, 0, True)[1]
    try:
        e9 = []
        for i in range(len(c.internal)):
            for k in range(K):
                e9 += c.ops(k, 0, True, model=0)[0][9 * i:9 * i + 9]
        c.eng.updatePartialsByPartition(e9, len(e9) // 9)
        c.whole.updatePartials(o7, len(o7) // 7, NONE)
        for b in (c.eng, c.whole):
            b.resetScaleFactors(c.cum)
            b.accumulateScaleFactors(idx, len(idx), c.cum)
            whole_scale_calls(c, b)
        whole_checks(c, "by-partition list, whole-range scale calls")
        c.further_evaluations("whole-range scale calls")
    finally:
        c.close()


@pytest.mark.parametrize("scaling", [False, True])
@pytest.mark.parametrize("K", [2, 9])
def test_reads_and_scale_calls_between_a_held_walk_and_its_root(K, scaling, oracle_lib):
    """Sequence 5 (4 states): between a held by-partition walk and its root call, getPartials, getPartialsBatch,
    getSiteLogLikelihoods, resetScaleFactorsByPartition and copyScaleFactors — each against the oracle, then the root."""
    c = Case(4, K, oracle_lib, scaling=scaling)
    try:
        c.update_by_partition()
        c.accumulate_by_partition()
        by, tot = c.root_by_partition()
        c.check_by_partition(by, tot, list(range(K)), c.eng.getSiteLogLikelihoods(), "first")
        site_before = c.eng.getSiteLogLikelihoods()
        c.matrices(1.05)
        c.update_by_partition()                                  # (held back)
        assert np.array_equal(c.eng.getSiteLogLikelihoods(), site_before)       # the last root sum's values, not the held walk's
        n = c.internal[len(c.internal) // 2]
        pe = c.eng.getPartials(c.buf(0, n), NONE)
        batch = c.eng.getPartialsBatch([c.root(), c.buf(0, n)])
        for i, k in enumerate(c.ids):
            a, b = c.ranges[k]
            for x, (eng_p, node) in enumerate(((pe, n), (batch[1], n), (batch[0], c.tree.root))):
                po = c.ora[i].getPartials(node, NONE)
                scale = np.maximum(np.abs(po).max(axis=(0, 2), keepdims=True), 1e-300)
                assert np.max(np.abs(eng_p[:, a:b, :] - po) / scale) <= 1e-10, (k, x)
        if scaling:
            c.eng.resetScaleFactorsByPartition(c.cum + 1, 0)
            c.eng.copyScaleFactors(c.cum + 1, c.cum)             # (stale factors of the last evaluation: the walk wrote new ones)
            c.accumulate_by_partition()
            c.eng.copyScaleFactors(c.cum + 1, c.cum)
            by, tot = c.root_by_partition(cum=c.cum + 1)
        else:
            by, tot = c.root_by_partition()
        c.check_by_partition(by, tot, list(range(K)), c.eng.getSiteLogLikelihoods(), "after the reads")
        c.further_evaluations("reads in between")
    finally:
        c.close()
