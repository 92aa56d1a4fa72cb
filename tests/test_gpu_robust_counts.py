"""Codon robust counts on the GPU (include/beagle_mi355.h beagleMi355RobustCounts / beagleMi355SimulateUnconditionedCounts,
beast-mcmc_amd/robustcounting.py) against the host restatement (tests/robust_counting_reference.py): the three draws must be the
ancestral sampler's byte for byte; values and totals equal by the criterion of tests/test_gpu_markov_jumps.py,
|a - b| <= 1e-12 |b| + floor with floor = 1e-15 x (magJ / P + |J| magP / P^2) gathered the same way (the kernels and the
restatement form every product and sum alike; the device's exp() and the host's differ in the last bit, which the difference
quotient of populateAuxInt amplifies by 1 / |la - lb| — the case builder keeps eigenvalue gaps out of (1e-7, 1e-4); chains with
gaps inside that band and under the tie threshold, and a branch of 1e-6, are in tests/test_gpu_markov_jumps_exact.py, which measures
the whole tables against an exact yardstick instead of a floor).  The unconditioned histories must equal the restatement exactly.
"""
import ctypes as C

import numpy as np
import pytest

import beast_mcmc_amd as bm
import helpers
import robust_counting_cases as cases
import robust_counting_reference as rr
from beast_mcmc_amd.inputs import substmodel, synth, trees
from beast_mcmc_amd.robustcounting import CodonPartitionedRobustCounting
from beast_mcmc_amd.treelikelihood import RESCALE_ALWAYS, RESCALE_DYNAMIC, BeagleTreeLikelihood

pytestmark = pytest.mark.gpu

G = helpers.golden("robust_counting.json")


class Case:
    """Three evaluated tree likelihoods over one tree (codon positions 1..3) and the robust-counting object over them."""

    def __init__(self, T, P, C=1, seed=0, rescale_first=False, unknown_fraction=0.05, tree=None, models=None, tips=None, **kw):
        eigs, pis, rates = models if models is not None else cases.position_models(seed)
        cat_rates, cat_weights = np.ones(1), np.ones(1)
        if tree is None:
            base = helpers.random_workload(T, P, 4, C, seed=500 + seed + T, unknown_fraction=unknown_fraction)
            tree, cat_rates, cat_weights = base.tree, base.cat_rates / base.cat_rates[0], base.cat_weights
        self.tree = tree
        self.tls = []
        for q in range(3):
            states = tips[q] if tips is not None else \
                helpers.random_workload(T, P, 4, C, seed=900 + 10 * seed + q, unknown_fraction=unknown_fraction).tip_states
            wl = synth.Workload("codon-%d" % q, self.tree, eigs[q], pis[q], rates[q] * cat_rates, cat_weights, states,
                                np.ones(states.shape[1]), 4)
            always = rescale_first and q == 0
            self.tls.append(BeagleTreeLikelihood(wl, rescaling=RESCALE_ALWAYS if always else RESCALE_DYNAMIC, delay_rescaling=not always,
                                                 **kw))
        self.rc = CodonPartitionedRobustCounting(*self.tls)
        self.rc.registers = cases.three_registers()
        self.evaluate()

    def evaluate(self):
        return [tl.getLogLikelihood() for tl in self.tls]

    def call(self, seeds=(11, 22, 33), use_map=False, registers=None, **kw):
        rows, order = self.rc.node_lists()
        U, Ui, lam, Q, _ = self.rc.chain()
        regs = self.rc.registers if registers is None else registers
        return self.rc.beagle.robustCounts([s.beagle for s in self.rc.samplers[1:]], rows, self.rc.branch_lengths(order), U, Ui, lam, Q,
                                           regs, seeds, map=use_map, **kw)

    def restated(self, states, include=None, registers=None):
        """-> ((values, site totals, branch totals), (their floors), tables) of the restatement for the drawn states."""
        rows, order = self.rc.node_lists()
        U, Ui, lam, Q, _ = self.rc.chain()
        regs = self.rc.registers if registers is None else registers
        taus = self.rc.branch_lengths(order)
        cond, J, P = rr.tables(U, Ui, lam, Q, regs, taus)
        fl = rr.floors(U, Ui, lam, Q, regs, taus, J, P)
        cod = rr.codons(states)
        return rr.gather(cond, cod, rows[0][:, 2], include), rr.gather(fl, cod, rows[0][:, 2], include), cond

    def close(self):
        for tl in self.tls:
            tl.close()


def assert_close(a, b, floor):
    """|a - b| <= 1e-12 |b| + floor"""
    err = np.abs(a - b)
    bad = ~(err <= 1e-12 * np.abs(b) + floor)
    assert not bad.any(), (np.argwhere(bad)[:5], a[bad][:5], b[bad][:5], err.max())


def check_against_restatement(case, use_map):
    seeds = (11, 22, 33)
    res = case.call(seeds, use_map, states=True, counts=True)
    rows, _ = case.rc.node_lists()
    for q in range(3):
        st, _ = case.rc.samplers[q].beagle.sampleAncestralStates(rows[q], 0, 0, seeds[q], map=use_map)
        assert np.array_equal(res["states"][q], st), q                              # the sampler's draw, byte for byte
    (vals, site, branch), (fv, fs, fb), _ = case.restated(res["states"])
    print("max |device - restatement|: values %.3e, site totals %.3e, branch totals %.3e" % (
        np.abs(res["counts"] - vals).max(), np.abs(res["site_totals"] - site).max(), np.abs(res["branch_totals"] - branch).max()))
    assert_close(res["counts"], vals, fv)
    assert_close(res["site_totals"], site, fs)
    assert_close(res["branch_totals"], branch, fb)
    assert not res["counts"][:, 0].any() and not res["branch_totals"][:, 0].any()     # row 0
    again = case.call(seeds, use_map, states=True, counts=True)
    for key in res:
        assert np.array_equal(res[key], again[key]), key                            # deterministic
    fewer = case.call(seeds, use_map)
    assert set(fewer) == {"site_totals", "branch_totals"}
    for key in fewer:
        assert np.array_equal(res[key], fewer[key]), key                            # fewer outputs, the same bits
    return res


@pytest.mark.parametrize("T,P,C,rescale", [
    (9, 300, 1, False),
    (25, 257, 1, True),          # position 1 under rescaling ALWAYS: its stored partials carry scale factors
    (6, 1, 1, False),
    (12, 500, 3, False),         # three rate categories on the instances: drawn and otherwise unused
])
def test_counts_equal_the_restatement(T, P, C, rescale):
    case = Case(T, P, C, seed=T % 8, rescale_first=rescale)
    for use_map in (False, True):
        check_against_restatement(case, use_map)
    case.close()


def test_known_answers_and_exact_ties_on_the_device():
    """CodonPartitionedRobustCountingTest.testCounts: three identical HKY kappa 2 models — every eigenvalue of the product chain is
    tied with others — on a two-tip tree with branch length 1.0."""
    g = G["conditional_means"]
    eigs = [substmodel.hky(k, f) for k, f in zip(g["kappa"], g["frequencies_acgt"])]
    pis = [np.asarray(f) for f in g["frequencies_acgt"]]
    tree = trees.Tree([-1, -1, 0], [-1, -1, 1], [0.0, 0.0, g["time"]], 2)
    tips = [np.zeros((2, 40), dtype=np.int32) for _ in range(3)]
    case = Case(2, 40, models=(eigs, pis, [1.0, 1.0, 1.0]), tree=tree, tips=tips)
    case.rc.registers = case.rc.registers[:2]
    res = case.call(tables=True, states=True)
    rows, order = case.rc.node_lists()
    assert list(case.rc.branch_lengths(order)) == [0.0, g["time"], g["time"]]

    def codon(text):
        return sum("ACGT".index(ch) << sh for ch, sh in zip(text, (4, 2, 0)))

    got = [res["tables"][("syn", "nonsyn").index(lab), 1, codon(g["from"]), codon(to)] for lab, to in zip(g["labeling"], g["to"])]
    print("device conditional means:", got)
    np.testing.assert_allclose(got, g["values"], rtol=0, atol=g["tolerance"])
    U, Ui, lam, Q, _ = case.rc.chain()
    taus = case.rc.branch_lengths(order)
    cond, J, P = rr.tables(U, Ui, lam, Q, case.rc.registers, taus)
    assert_close(res["tables"], cond, rr.floors(U, Ui, lam, Q, case.rc.registers, taus, J, P))
    case.close()


def test_zero_length_branch():
    case = Case(6, 120, seed=3)
    tl = case.tls[0]
    tree = case.tree
    node = next(n for n in range(tree.tip_count, tree.node_count) if tree.parent[n] >= 0)
    for t in case.tls:
        t.set_node_height(node, t.node_height(int(tree.parent[node])))
    case.evaluate()
    res = case.call(states=True, counts=True, tables=True)
    rows, order = case.rc.node_lists()
    r = list(order).index(node)
    assert case.rc.branch_lengths(order)[r] == 0.0
    assert not res["counts"][:, r].any() and not res["branch_totals"][:, r].any()
    (vals, site, branch), (fv, fs, fb), cond = case.restated(res["states"])
    np.testing.assert_array_equal(res["tables"][:, r], cond[:, r])                   # (NaNs equal: exp(0) is exact on both sides)
    assert_close(res["counts"], vals, fv)
    assert_close(res["site_totals"], site, fs)
    case.close()


def test_include_rows():
    case = Case(10, 200, seed=4)
    rows, order = case.rc.node_lists()
    tips = np.asarray(order) < case.tree.tip_count
    full = case.call(states=True, counts=True)
    for include in (tips.astype(np.uint8), (~tips).astype(np.uint8), np.ones(len(order), dtype=np.uint8)):
        res = case.call(states=True, counts=True, include_rows=include)
        (vals, site, branch), (fv, fs, fb), _ = case.restated(res["states"], include)
        assert_close(res["site_totals"], site, fs)
        for key in ("states", "counts", "branch_totals"):
            assert np.array_equal(res[key], full[key]), key
    assert np.array_equal(res["site_totals"], full["site_totals"])
    case.rc.include_internal = False
    out = case.rc.sample(11)
    ext = case.call((11, 12, 13), include_rows=tips.astype(np.uint8))
    assert np.array_equal(out["site"], ext["site_totals"])
    assert np.array_equal(out["branch"][:, order], ext["branch_totals"])
    case.close()


def test_unknown_compact_tips_and_a_tip_with_partials():
    case = Case(14, 300, seed=5, unknown_fraction=0.2)
    tl = case.tls[1]
    rng = np.random.default_rng(4)
    part = rng.uniform(0.0, 1.0, size=(300, 4))
    part[rng.random(300) < 0.5] = 1.0
    part = np.ascontiguousarray(part)
    assert tl.h.btlSetTipPartials(tl.ptr, 3, part.ctypes.data_as(C.POINTER(C.c_double))) == 0
    case.evaluate()
    for use_map in (False, True):
        check_against_restatement(case, use_map)
    case.close()


def raw(case, **kw):
    """The C call itself with one argument replaced -> return code."""
    lib = case.rc.beagle.lib.lib
    f = lib.beagleMi355RobustCounts
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 6 + [C.c_int] + \
        [C.c_void_p] * 6
    rows, order = case.rc.node_lists()
    U, Ui, lam, Q, _ = case.rc.chain()
    n, P = rows.shape[1], case.tls[0].pattern_count
    a = {
        "instances": np.array([tl.instance for tl in case.tls], dtype=np.int32), "nodes": np.ascontiguousarray(rows, dtype=np.int32),
        "nodeCount": n, "w": np.zeros(3, dtype=np.int32), "f": np.zeros(3, dtype=np.int32),
        "seeds": np.array([1, 2, 3], dtype=np.uint64), "flags": 0, "tau": case.rc.branch_lengths(order), "U": U, "Ui": Ui, "lam": lam,
        "Q": Q, "regs": np.ascontiguousarray(case.rc.registers), "K": len(case.rc.registers), "include": None, "states": None,
        "counts": None, "site": np.empty((8, P)), "branch": np.empty((8, n)), "tables": None,
    }
    a.update(kw)
    keep = [v for v in a.values() if isinstance(v, np.ndarray)]
    args = [v.ctypes.data if isinstance(v, np.ndarray) else v for v in a.values()]
    rc = f(*args)
    del keep
    return rc


def test_error_codes():
    case = Case(8, 64, seed=6)
    assert raw(case) == 0
    rows, _ = case.rc.node_lists()
    # BEAGLE_ERROR_OUT_OF_RANGE
    for name in ("instances", "nodes", "w", "f", "seeds", "tau", "U", "Ui", "lam", "Q", "regs"):
        assert raw(case, **{name: None}) == -5, name
    assert raw(case, nodeCount=0) == -5
    assert raw(case, K=0) == -5 and raw(case, K=9) == -5
    assert raw(case, flags=2) == -5 and raw(case, flags=1) == 0
    assert raw(case, site=None, branch=None) == -5
    wrong = rows.copy()
    wrong[2, 3, 2] = 0 if rows[2, 3, 2] != 0 else 1
    assert raw(case, nodes=np.ascontiguousarray(wrong)) == -5                        # parent rows disagree
    twice = np.array([case.tls[0].instance, case.tls[0].instance, case.tls[2].instance], dtype=np.int32)
    assert raw(case, instances=twice) == -5
    assert raw(case, w=np.array([0, 7, 0], dtype=np.int32)) == -5                    # the ancestral call's errors
    bad_root = rows.copy()
    bad_root[1, 0, 0] = 0                                                            # a compact tip at the root
    assert raw(case, nodes=np.ascontiguousarray(bad_root)) == -5
    # BEAGLE_ERROR_FLOATING_POINT: a gathered value that is not finite
    tau = case.rc.branch_lengths(case.rc.node_lists()[1])
    tau[3] = np.nan
    assert raw(case, tau=tau) == -8
    # BEAGLE_ERROR_NO_IMPLEMENTATION
    other = Case(8, 65, seed=6)
    mixed = np.array([case.tls[0].instance, other.tls[1].instance, case.tls[2].instance], dtype=np.int32)
    assert raw(case, instances=mixed) == -7                                          # differing P
    wl20 = helpers.random_workload(8, 64, 20, 1, seed=3)
    tl20 = BeagleTreeLikelihood(wl20)
    tl20.getLogLikelihood()
    assert raw(case, instances=np.array([case.tls[0].instance, case.tls[1].instance, tl20.instance], dtype=np.int32)) == -7
    tl20.close()
    case.rc.samplers[2].beagle.setPatternPartitions(2, (np.arange(64) >= 32).astype(np.int32))
    assert raw(case) == -7
    case.close(); other.close()


def test_sharded_and_other_device_handles_are_refused():
    case = Case(8, 64, seed=6)
    g = len(bm.beagle.engine().resource_list()) - 2
    wl = helpers.random_workload(8, 64, 4, 1, seed=3)
    sharded = BeagleTreeLikelihood(wl, resource_list=(g + 1,))
    sharded.getLogLikelihood()
    assert raw(case, instances=np.array([case.tls[0].instance, sharded.instance, case.tls[2].instance], dtype=np.int32)) == -7
    b = bm.beagle.Beagle.attach(sharded)
    with pytest.raises(bm.beagle.BeagleException) as e:
        b.simulateUnconditionedCounts(np.array([[-1.0, 1.0], [1.0, -1.0]]), [0.5, 0.5], [1.0], 4, np.ones((1, 2, 2)), 1)
    assert e.value.code == -7
    sharded.close()
    if g > 1:
        far = BeagleTreeLikelihood(wl, resource_list=(2,))                            # the second GPU
        far.getLogLikelihood()
        assert raw(case, instances=np.array([case.tls[0].instance, far.instance, case.tls[2].instance], dtype=np.int32)) == -7
        far.close()
    case.close()


def test_the_call_leaves_the_likelihood_path_alone():
    a, b = Case(20, 600, seed=7), Case(20, 600, seed=7)
    before = [(tl.getLogLikelihood(), tl.getSiteLogLikelihoods()) for tl in a.tls]
    a.rc.sample(3, per_branch_site=True, states=True)
    a.rc.sample(4)
    a.rc.unconditioned(5)
    for tl, (lnl, sites) in zip(a.tls, before):
        tl.makeDirty()
        assert tl.getLogLikelihood() == lnl and np.array_equal(tl.getSiteLogLikelihoods(), sites)
    for tl in b.tls:
        tl.makeDirty()
        tl.getLogLikelihood()
    tree = a.tree
    rng = np.random.default_rng(1)
    for it in range(6):
        node = int(rng.integers(tree.tip_count, tree.node_count))
        h = helpers.proposed_height(tree, node, rng)
        for case in (a, b):
            for tl in case.tls:
                tl.set_node_height(node, h)
        tree.height[node] = h
        assert a.evaluate() == b.evaluate()                                          # bitwise
        for x, y in zip(a.tls, b.tls):
            assert np.array_equal(x.getSiteLogLikelihoods(), y.getSiteLogLikelihoods())
        if it % 2 == 0:
            a.rc.sample(it)
    a.close(); b.close()


@pytest.mark.parametrize("name", ["chain64", "hky4"])
@pytest.mark.parametrize("sites", cases.UNCONDITIONED_SITES)
def test_unconditioned_equals_the_restatement(name, sites):
    Q, pi, regs = cases.unconditioned_cases()[name]
    wl = helpers.random_workload(4, 8, 4, 1, seed=1)
    tl = BeagleTreeLikelihood(wl)
    b = bm.beagle.Beagle.attach(tl)
    res = b.simulateUnconditionedCounts(Q, pi, cases.UNCONDITIONED_LENGTHS, sites, regs, cases.UNCONDITIONED_SEED)
    vals, near, cut = rr.unconditioned(Q, pi, cases.UNCONDITIONED_LENGTHS, sites, regs, cases.UNCONDITIONED_SEED)
    assert int(near.sum()) == 0 and not cut.any()                                    # nothing is excluded from the comparison
    print("histories that differ:", int((res["counts"] != vals).any(axis=0).sum()), "of", near.size)
    assert np.array_equal(res["counts"], vals)
    assert not res["counts"][:, 0].any() and (sites == 1 or res["counts"][:, 2].any())      # length 0.0: all zeros
    np.testing.assert_allclose(res["totals"], rr.block_totals(vals), rtol=1e-13, atol=0)
    again = b.simulateUnconditionedCounts(Q, pi, cases.UNCONDITIONED_LENGTHS, sites, regs, cases.UNCONDITIONED_SEED)
    only = b.simulateUnconditionedCounts(Q, pi, cases.UNCONDITIONED_LENGTHS, sites, regs, cases.UNCONDITIONED_SEED, counts=False)
    assert np.array_equal(again["counts"], res["counts"]) and np.array_equal(again["totals"], res["totals"])
    assert set(only) == {"totals"} and np.array_equal(only["totals"], res["totals"])
    tl.close()


def test_unconditioned_stage_smaller_than_the_lengths():
    """Two length rows of 2^24 + 256 sites are more than the 256 MiB stage holds: the counts leave in two launches of one row each.
    A 0/1 register's values are whole numbers, so every sum of them is exact: the totals of the call without counts (one launch over
    both rows) are the counts' sums, and row 0 is the one-row call's (its streams are keyed on l * sites + s: the same keys)."""
    Q, pi, _ = cases.unconditioned_cases()["hky4"]
    regs = np.ones((1, 4, 4))
    sites, lengths = (1 << 24) + 256, [0.05, 0.02]
    tl = BeagleTreeLikelihood(helpers.random_workload(4, 8, 4, 1, seed=1))
    b = bm.beagle.Beagle.attach(tl)
    res = b.simulateUnconditionedCounts(Q, pi, lengths, sites, regs, 77)
    only = b.simulateUnconditionedCounts(Q, pi, lengths, sites, regs, 77, counts=False)
    first = b.simulateUnconditionedCounts(Q, pi, lengths[:1], sites, regs, 77)
    assert np.array_equal(res["totals"], only["totals"]) and np.array_equal(res["counts"].sum(axis=2), only["totals"])
    assert res["totals"][0, 0] > res["totals"][0, 1] > 0.0
    assert np.array_equal(res["counts"][:, 0], first["counts"][:, 0])
    tl.close()


def test_unconditioned_through_the_veneer_and_error_codes():
    case = Case(8, 300, seed=2)
    case.rc.registers = case.rc.registers[:2]
    u = case.rc.unconditioned(17)
    _, _, _, Q, pi = case.rc.chain()
    vals, near, _ = rr.unconditioned(Q, pi, [case.rc.expected_tree_length()], 300, case.rc.registers, 17)
    assert int(near.sum()) == 0 and np.array_equal(u, vals[:, 0])
    per = case.rc.unconditioned(18, per_branch=True)
    assert per.shape == (2, case.tree.node_count, 300) and not per[:, case.tree.root].any() and per.sum() > 0.0
    assert case.rc.marginal_rate(0) > 0.0 and case.rc.marginal_rate(1) > case.rc.marginal_rate(0)
    b = case.rc.beagle
    regs = case.rc.registers

    def code(Qx=Q, pix=pi, lengths=(1.0,), sites=10, R=regs, **kw):
        with pytest.raises(bm.beagle.BeagleException) as e:
            b.simulateUnconditionedCounts(Qx, pix, lengths, sites, R, 1, **kw)
        return e.value.code

    assert code(Qx=np.zeros((1, 1)), pix=np.ones(1), R=np.zeros((1, 1, 1))) == -5     # stateCount outside 2..64
    assert code(Qx=np.zeros((65, 65)), pix=np.ones(65), R=np.zeros((1, 65, 65))) == -5
    assert code(R=np.zeros((0, 64, 64))) == -5 and code(R=np.zeros((9, 64, 64))) == -5
    bad = Q.copy(); bad[3, 4] = np.inf
    assert code(Qx=bad) == -5
    assert code(lengths=(-0.1,)) == -5 and code(lengths=(np.nan,)) == -5 and code(lengths=()) == -5
    assert code(sites=0) == -5 and code(counts=False, totals=False) == -5
    f = b.lib.lib.beagleMi355SimulateUnconditionedCounts
    f.restype = C.c_int
    f.argtypes = [C.c_int, C.c_int] + [C.c_void_p] * 3 + [C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_ulonglong, C.c_void_p, C.c_void_p]
    out = np.empty((2, 1, 10))
    one = np.ones(1)
    ptrs = [Q.ctypes.data, pi.ctypes.data, one.ctypes.data, regs.ctypes.data]
    assert f(b.instance, 64, ptrs[0], ptrs[1], ptrs[2], 1, 10, ptrs[3], 2, 1, out.ctypes.data, None) == 0
    for i in range(4):
        p = list(ptrs); p[i] = None
        assert f(b.instance, 64, p[0], p[1], p[2], 1, 10, p[3], 2, 1, out.ctypes.data, None) == -5, i
    # a Q x length that would never finish: cut at 100 000 jumps, BEAGLE_ERROR_FLOATING_POINT
    fast = np.array([[-1e9, 1e9], [1e9, -1e9]])
    assert code(Qx=fast, pix=np.array([0.5, 0.5]), R=np.ones((1, 2, 2)), sites=3) == -8
    case.close()
