"""The Markov-jump and robust-count tables of the device against an exact yardstick (tests/markov_jumps_exact.py: a long double
block exponential, no eigenvalue in it), where tests/test_gpu_markov_jumps.py and tests/test_gpu_robust_counts.py compare with a
restatement of the kernels' own formula under a floor sized to that formula's cancellation.

Markov jumps: every case of markov_jumps_exact.jump_cases() on a two-tip tree; each gathered value against the yardstick entry of
its drawn (category, parent state, state) in the metric |v - exact| / max(|exact|, unit).  Robust counts: the whole 64 x 64 table
of every row.  Bounds (markov_jumps_exact.bound_for): 1e-10 where the eigen formula is well conditioned or exactly tied; elsewhere
(near ties, short branches, thin transition probabilities) 4 x what the float64 restatement loses against the yardstick on the
same entries, plus 1e-13 — device and restatement do the same operations in the same order and differ in the last bit of exp(),
which enters every entry through the same cancellation.  The restatement is measured against; the device never is.
Run with -s for the figures DESIGN.md section 6 tabulates.
"""
import numpy as np
import pytest

import beast_mcmc_amd as bm
import helpers
import markov_jumps_exact as mx
import robust_counting_reference as rr
import test_gpu_markov_jumps as jumps_base
import test_gpu_robust_counts as robust_base
from beast_mcmc_amd.inputs import substmodel
from beast_mcmc_amd.markovjumps import MarkovJumpsSampler
from beast_mcmc_amd.treelikelihood import BeagleTreeLikelihood

pytestmark = pytest.mark.gpu


def device_eigen(case):
    """The case's model decomposed by the device and read back."""
    b = bm.beagle.Beagle(2, 3, 2, case.S, 16, 1, 4, 1, 0)
    b.setReversibleModels([0], [case.rel_rates], [case.pi])
    U, Ui, lam = b.getEigenDecomposition(0)
    b.finalize()
    return U, Ui, lam


@pytest.mark.parametrize("case", mx.jump_cases(), ids=repr)
def test_gathered_values_against_the_yardstick(case):
    if case.device_eigen:
        host = next(c for c in mx.host_jump_cases() if c.name == case.name.replace("-device", ""))
        U, Ui, lam = device_eigen(case)
        cond, unit = case.exact(U, Ui, lam)
        assert np.sort(lam)[-2] - np.sort(lam)[0] < 1e-7                              # S - 1 tied eigenvalues, by its own solver
    else:
        host = case
        U, Ui, lam, cond, unit = mx.host_tables(case)
    R = mx.host_repeats(host)
    S, C = case.S, len(case.cat_rates)
    tl = BeagleTreeLikelihood(mx.two_tip_workload(case, substmodel.EigenDecomposition(U, Ui, lam), R))
    tl.set_branch_rates(np.full(3, case.branch_rate))
    tl.getLogLikelihood()
    s = MarkovJumpsSampler(tl)
    for tag, values, kind, scaled in zip(case.tags, case.registers, case.kinds, case.scale_by_time):
        s.add_register(tag, np.diag(values) if kind == "rewards" else values, kind=kind, scale_by_time=scaled)
    rows, order = s.ancestral.node_list()
    times, rates = s.branch_times(order)
    assert np.array_equal(times, case.times()) and np.array_equal(rates, case.rates()) and list(rows[:, 2]) == [-1, 0, 0]
    res = jumps_base.raw_call(s, 4242, states=True, jumps=True)                    # returns: the call's code was 0
    st, ca = res["states"], res["categories"]
    missing = mx.drawn_missing_share(st, ca, S, C)
    mats = s.beagle.getTransitionMatrix(int(rows[1, 1])).reshape(C, S, S)
    rest = case.restatement(U, Ui, lam, matrices=mats)
    got, lost, bound = mx.judge(case.regime, res["jumps"][:, 1:3], mx.gathered(rest, st, ca), mx.gathered(cond, st, ca),
                                unit[:, ca][:, None, :])
    print("%s (%s), %d patterns, %.3f %% of a row's entries never gathered: %s" % (case.name, case.regime, st.shape[1], 100.0 * missing,
          "; ".join("%s device %.2e restatement %.2e bound %.2e" % z for z in zip(case.tags, got, lost, bound))))
    tl.close()
    assert st.shape[1] > 256 and missing <= mx.COVERAGE_DRAWN
    assert np.all(res["jumps"][:, 0] == 0.0)
    assert np.all(got <= bound), (got, lost, bound)


@pytest.mark.parametrize("case", mx.robust_cases(), ids=repr)
def test_robust_count_tables_against_the_yardstick(case):
    rng = np.random.default_rng(8)
    tips = [rng.integers(0, 4, size=(case.tree.tip_count, 64)).astype(np.int32) for _ in range(3)]       # (the tables do not depend on them)
    g = robust_base.Case(case.tree.tip_count, 64, models=case.models, tree=case.tree, tips=tips)
    g.rc.registers = case.registers()
    res = g.call(tables=True)
    rows, order = g.rc.node_lists()
    taus = g.rc.branch_lengths(order)
    assert np.array_equal(np.sort(taus[1:]), np.sort(case.branch_lengths()[case.branch_lengths() > 0.0]))
    U, Ui, lam, Q, _ = g.rc.chain()                                                # what the call was handed
    for a, b in zip((U, Ui, lam, Q), case.chain()):
        np.testing.assert_allclose(a, b, rtol=0, atol=1e-14)
    exact, mask = case.exact(taus, (U, Ui, lam, Q)), case.resolvable(taus, (U, Ui, lam, Q))
    rest = rr.tables(U, Ui, lam, Q, g.rc.registers, taus)[0]
    g.close()
    assert not res["tables"][:, 0].any()
    failures = []
    for r in range(1, len(taus)):
        regime = case.row_regime(taus[r])
        got, lost, bound = mx.judge(regime, res["tables"][:, r], rest[:, r], exact[:, r], case.units()[:, None, None], mask[r])
        print("%s row %d tau %g (%s), %.1f %% of the entries below float64's resolution of P: device %s restatement %s bound %s" % (
            case.name, r, taus[r], regime, 100.0 * (1.0 - mask[r].mean()), got, lost, bound))
        if not np.all(got <= bound) or not (mask[r].all() or regime == "short"):
            failures.append((r, taus[r], got, bound))
    assert not failures, failures


def test_zero_length_branch_in_the_markov_jump_call():
    """An inner node moved onto its parent: the call succeeds; that row's values are finite, its counts 0 and its time-scaled
    rewards 0 (tau = 0: A = 0, so J = 0 over P = I on the diagonal, which is all a draw gathers there); the totals equal the
    restatement's by the criterion of tests/test_gpu_markov_jumps.py."""
    wl = helpers.random_workload(6, 300, 4, 2, seed=77)
    tl = jumps_base.make(wl, branch_rate_seed=5)
    tree = wl.tree
    node = next(n for n in range(tree.tip_count, tree.node_count) if tree.parent[n] >= 0)
    tl.set_node_height(node, tl.node_height(int(tree.parent[node])))
    tl.getLogLikelihood()
    s = jumps_base.three_registers(MarkovJumpsSampler(tl), 4, seed=6)
    rows, order = s.ancestral.node_list()
    r = list(order).index(node)
    assert s.branch_times(order)[0][r] == 0.0
    for use_map in (False, True):
        res = jumps_base.raw_call(s, 19, use_map, states=True, jumps=True)         # a floating-point error flag would raise (-8)
        assert np.all(np.isfinite(res["jumps"][:, r]))
        assert np.array_equal(res["states"][r], res["states"][rows[r, 2]])           # P = I: the child is its parent
        assert not res["jumps"][:, r].any() and not res["row_totals"][:, r].any()
        vals, tot, row_tot, floors = jumps_base.restated(tl, s, res["states"], res["categories"])
        jumps_base.assert_close(res["jumps"], vals, floors[0])
        jumps_base.assert_close(res["pattern_totals"], tot, floors[1])
        jumps_base.assert_close(res["row_totals"], row_tot, floors[2])
    tl.close()
