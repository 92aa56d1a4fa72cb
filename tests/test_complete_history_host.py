"""Complete-history simulation, CPU tier: the C ABI symbol, the host restatement (tests/complete_history_reference.py) against a
literal transliteration of the reference's Java objects fed the same uniforms, against the exact tip-pattern distribution and the
marginal rates, the rules of the header on hand-made cases, and the condition the GPU tier rests on: no history of any case it uses
has an event time within 1e-12 relative of its branch's end, and none is cut.

Reward bound against the transliterated getTotalReward: the restatement adds R_cc * (t - t_prev) per sojourn in time order, the
reference first adds the sojourns per state (getWaitingTimes) and then forms the index-order dot product with the S-vector — the same
exact quantity, reached by n + 1 products and additions on one side and n + 1 additions, S products and S additions on the other.
Every partial sum is at most tau * max |R_kk|, so the two differ by at most (n + 2 + S) roundings of that size on each side; with
the factor BOUND_C of the GPU tier (which covers both sides and the subtraction): BOUND_C * (n + 2 + S) * 2^-53 * tau * max |R_kk|.
"""
import os
import re

import numpy as np
import pytest

import beast_mcmc_amd as bm
import complete_history_cases as cc
import complete_history_reference as hr
import helpers
import simulate_cases as sc
import uniformized_reference as ur

SYMBOL = "beagleMi355SimulateCompleteHistories"


def test_library_exports_and_header_declares_the_simulator(engine_lib):
    assert hasattr(engine_lib.lib, SYMBOL)
    hdr = open(os.path.join(helpers.ROOT, "include", "beagle_mi355.h")).read()
    assert re.search(r"\bint\s+%s\s*\(" % SYMBOL, hdr)
    assert "cumulative form" in hdr.lower() and "0x3C6EF372FE94F82B" in hdr      # the draw's form and the stream are part of the contract
    exports = open(os.path.join(helpers.ROOT, "beast-mcmc_amd", "csrc", "exports.map")).read()
    assert re.search(r"global:[^}]*\bbeagle\*;", exports)                       # (the map exports the C API by its prefix)
    assert SYMBOL in bm.beagle.ABI_SYMBOLS
    assert hasattr(bm.beagle.Beagle, "simulateCompleteHistories")
    from beast_mcmc_amd.completehistory import CompleteHistorySimulator
    assert hasattr(CompleteHistorySimulator, "simulate") and hasattr(CompleteHistorySimulator, "node_list")


# ---- a literal transliteration of StateHistory (src/dr/inference/markovjumps/StateHistory.java) and of MathUtils' two draws
class JavaStateHistory:
    def __init__(self, time, state, state_count):
        self.stateList = [(time, state)]
        self.stateCount = state_count
        self.finalized = False

    def addChange(self, time, state):
        assert not self.finalized
        self.stateList.append((time, state))

    def addEndingState(self, time, state):
        assert not self.finalized
        self.stateList.append((time, state))
        self.finalized = True

    def getNumberOfJumps(self):
        return len(self.stateList) - 2

    def getEndingState(self):
        return self.stateList[-1][1]

    def accumulateSufficientStatistics(self, counts, times):
        nJumps = self.getNumberOfJumps()
        currentTime, currentState = self.stateList[0]
        for i in range(1, nJumps + 1):
            nextTime, nextState = self.stateList[i]
            if counts is not None:
                counts[currentState * self.stateCount + nextState] += 1
            if times is not None:
                times[currentState] += (nextTime - currentTime)
            currentState, currentTime = nextState, nextTime
        if times is not None:
            times[currentState] += (self.stateList[nJumps + 1][0] - currentTime)

    def getTotalRegisteredCounts(self, register):
        counts = [0] * (self.stateCount * self.stateCount)
        self.accumulateSufficientStatistics(counts, None)
        total = 0.0
        for i in range(len(counts)):
            total += counts[i] * register[i]
        return total

    def getTotalReward(self, register):
        times = [0.0] * self.stateCount
        self.accumulateSufficientStatistics(None, times)
        total = 0.0
        for i in range(len(times)):
            total += times[i] * register[i]
        return total


def java_random_choice_pdf(pdf, next_double):
    total = 0.0
    for x in pdf:
        total += x
    U = next_double() * total
    for i in range(len(pdf)):
        U -= pdf[i]
        if U < 0.0:
            return i
    raise AssertionError("randomChoicePDF falls through")


def java_simulate_unconditional(starting_time, starting_state, ending_time, lam, state_count, next_double):
    history = JavaStateHistory(starting_time, starting_state, state_count)
    currentTime, currentState = starting_time, starting_state
    while currentTime < ending_time:
        currentRate = -lam[currentState * state_count + currentState]
        waitingTime = -1.0 * float(np.log(1 - next_double())) / currentRate
        currentTime += waitingTime
        if currentTime < ending_time:
            multinomial = list(lam[currentState * state_count:(currentState + 1) * state_count])
            multinomial[currentState] = 0
            currentState = java_random_choice_pdf(multinomial, next_double)
            history.addChange(currentTime, currentState)
    history.addEndingState(ending_time, currentState)
    return history


def java_traverse(c, seed, site_count):
    """CompleteHistorySimulator.traverse over the rows of a case: per (row, site) the StateHistory, fed the stream of (row, site)."""
    n = len(c.rows)
    histories = [[None] * site_count for _ in range(n)]
    seq = np.zeros((n, site_count), dtype=np.int64)
    cats = np.zeros(site_count, dtype=np.int64)
    for s in range(site_count):
        z = hr.stream(seed, np.uint64(s))
        us = iter([float(ur.uniform(z, 0)), float(ur.uniform(z, 1))])
        seq[0, s] = java_random_choice_pdf(list(c.freqs), lambda: next(us))
        cats[s] = java_random_choice_pdf(list(c.cat_weights), lambda: next(us)) if c.C > 1 else 0
    for r in range(1, n):
        lam = list(c.Q[c.rows[r, 1]].reshape(-1))
        for s in range(site_count):
            z = hr.stream(seed, np.uint64(r * site_count + s))
            q = [0]

            def next_double():
                q[0] += 1
                return float(ur.uniform(z, q[0] - 1))

            length = c.cat_rates[cats[s]] * c.lengths[r]
            histories[r][s] = java_simulate_unconditional(0.0, int(seq[c.rows[r, 2], s]), length, lam, c.S, next_double)
            seq[r, s] = histories[r][s].getEndingState()
    return histories, seq, cats


@pytest.mark.parametrize("name,sites", [("s2", 40), ("s4", 25), ("s4zero", 6), ("s20", 12)])
def test_restatement_equals_the_transliterated_java(name, sites):
    c = cc.build(name)
    res = cc.restate(c, site_count=sites)
    assert not res["bad"] and res["near"].sum() == 0
    histories, seq, cats = java_traverse(c, c.seed, sites)
    assert np.array_equal(res["states"], seq) and np.array_equal(res["categories"], cats)
    e, worst = 0, 0.0
    for s in range(sites):
        for r in range(1, len(c.rows)):
            h = histories[r][s]
            jumps = h.getNumberOfJumps()
            assert res["counts"][r, s] == jumps
            for m in range(jumps):                          # the jump list: site, row, time order
                assert res["event_site"][e] == s and res["event_row"][e] == r
                assert res["event_time"][e] == h.stateList[m + 1][0]
                assert tuple(res["event_states"][e]) == (h.stateList[m][1], h.stateList[m + 1][1])
                e += 1
            tau = c.cat_rates[cats[s]] * c.lengths[r]
            for k in range(c.K):
                if c.flags[k] & hr.REWARDS:
                    want = h.getTotalReward(list(np.diag(c.registers[k])))
                    bound = cc.BOUND_C * (jumps + 2 + c.S) * cc.EPS * tau * np.abs(np.diag(c.registers[k])).max()
                    diff = abs(res["values"][k, r, s] - want)
                    assert diff <= bound
                    worst = max(worst, diff / bound if bound > 0 else 0.0)
                else:
                    assert res["values"][k, r, s] == h.getTotalRegisteredCounts(list(c.registers[k].reshape(-1)))
    assert e == len(res["event_site"])
    print("%s: %d events, largest reward difference %.3f of its bound" % (name, e, worst))


# ---- the distribution of the tips, the case of tests/simulate_cases.py
def _distribution_inputs():
    tl = sc.tree_likelihood(library=helpers.oracle_library())
    assert np.isfinite(tl.getLogLikelihood())
    prob = np.exp(tl.getSiteLogLikelihoods())
    tl.close()
    tree = sc.tree()
    rows, order = cc.tree_rows(tree, ancestral=False)
    lengths = np.array([0.0 if r == 0 else tree.branch_length(int(n)) for r, n in enumerate(order)])
    return prob, rows, lengths, cc.q_of(sc.model())


def _tips(states, rows):
    out = np.zeros((4, states.shape[1]), dtype=np.uint8)
    for r in range(len(rows)):
        if rows[r, 0] >= 0:
            out[rows[r, 0]] = states[r]
    return out


@pytest.fixture(scope="module")
def exact_case():
    return _distribution_inputs()


def test_restatement_draws_the_exact_pattern_distribution(exact_case):
    prob, rows, lengths, Q = exact_case
    res = hr.simulate(rows, lengths, Q[None], np.ones((1, 4, 4)), None, sc.CAT_RATES, sc.CAT_WEIGHTS, sc.FREQS, sc.SEED, sc.N_SITES,
                      events=False)
    assert not res["bad"]
    sc.check_distribution(_tips(res["states"], rows), res["categories"], prob)


def test_a_transposed_restatement_exceeds_the_bound(exact_case):
    prob, rows, lengths, Q = exact_case
    assert not np.allclose(Q, Q.T, atol=1e-3)
    res = hr.simulate(rows, lengths, np.ascontiguousarray(Q.T)[None], np.ones((1, 4, 4)), None, sc.CAT_RATES, sc.CAT_WEIGHTS, sc.FREQS,
                      sc.SEED, sc.N_SITES, events=False)
    stat = sc.chi_square(_tips(res["states"], rows), prob)
    print("transposed: chi2 = %.1f (bound %.2f)" % (stat, sc.CHI2_BOUND))
    assert stat > sc.CHI2_BOUND


def test_means_are_marginal_rate_and_reward_times_length():
    """Stationary start: every branch's start state has the frequencies' distribution, so the mean all-jumps count on a branch is
    sum_i pi_i (-Q_ii) x E[rate] x length and the mean reward sum_i pi_i R_ii x E[tau]; 5 standard errors at a fixed seed."""
    tree = sc.tree()
    rows, order = cc.tree_rows(tree)
    lengths = np.array([0.0 if r == 0 else tree.branch_length(int(n)) for r, n in enumerate(order)])
    Q = cc.q_of(sc.model())
    reward = np.array([0.3, 1.1, 0.7, 2.0])
    regs = np.stack([np.ones((4, 4)) - np.eye(4), np.diag(reward)])
    n = 200000
    res = hr.simulate(rows, lengths, Q[None], regs, [0, hr.REWARDS], sc.CAT_RATES, sc.CAT_WEIGHTS, sc.FREQS, 777, n, events=False)
    assert not res["bad"]
    mean_rate = float(np.dot(sc.CAT_WEIGHTS, sc.CAT_RATES))
    marginal = float(np.dot(sc.FREQS, -np.diag(Q)))
    for r in range(1, len(rows)):
        for k, want in ((0, marginal * mean_rate * lengths[r]), (1, float(np.dot(sc.FREQS, reward)) * mean_rate * lengths[r])):
            v = res["values"][k, r]
            se = v.std(ddof=1) / np.sqrt(n)
            print("row %d register %d: mean %.5f, expected %.5f, standard error %.5f" % (r, k, v.mean(), want, se))
            assert abs(v.mean() - want) <= 5.0 * se


# ---- the rules
def _tiny(Q, lengths, regs, flags, rates=(1.0,), weights=(1.0,), freqs=None, rows=None, n=500, seed=5, **kw):
    S = len(Q)
    rows = [[0, 0, -1], [1, 0, 0], [2, 0, 1]] if rows is None else rows
    freqs = np.full(S, 1.0 / S) if freqs is None else freqs
    return hr.simulate(rows, lengths, np.asarray(Q, dtype=np.float64)[None], regs, flags, rates, weights, freqs, seed, n, **kw)


Q3 = np.array([[-1.0, 0.6, 0.4], [0.5, -1.5, 1.0], [0.2, 0.3, -0.5]])
COUNT_AND_REWARD = (np.stack([np.ones((3, 3)) - np.eye(3), np.diag([1.0, 2.0, 3.0])]), [0, hr.REWARDS])


def test_a_zero_length_branch_copies_the_parent():
    res = _tiny(Q3, [0.0, 0.0, 1.5], *COUNT_AND_REWARD)
    assert np.array_equal(res["states"][1], res["states"][0]) and not res["counts"][1].any()
    assert not res["values"][:, 1].any() and res["counts"][2].any()


def test_an_absorbing_state_ends_the_history():
    Q = np.array([[-1.0, 1.0, 0.0], [0.0, 0.0, 0.0], [0.5, 0.5, -1.0]])
    res = _tiny(Q, [0.0, 3.0, 3.0], *COUNT_AND_REWARD, root_states=np.zeros(500, dtype=np.uint8))
    assert not res["bad"]
    assert res["counts"][1].max() == 1 and set(np.unique(res["states"][1])) == {0, 1}
    absorbed = res["states"][1] == 1
    assert np.all(res["states"][2][absorbed] == 1) and not res["counts"][2][absorbed].any()
    assert np.all(res["values"][1, 2][absorbed] == 2.0 * 3.0)             # the reward of the whole branch in state 1


def test_a_zero_rate_category_stops_the_clock():
    res = _tiny(Q3, [0.0, 2.0, 2.0], *COUNT_AND_REWARD, rates=(0.0, 2.0), weights=(0.5, 0.5))
    still = res["categories"] == 0
    assert still.any() and not still.all()
    assert np.all(res["states"][1:, still] == res["states"][0, still]) and not res["counts"][:, still].any()
    assert not res["values"][:, :, still].any() and res["counts"][:, ~still].any()


def test_given_root_states_and_categories_are_taken_as_they_are():
    n = 500
    root, cats = (np.arange(n) % 3).astype(np.uint8), (np.arange(n) % 2).astype(np.int32)
    res = _tiny(Q3, [0.0, 1.0, 1.0], *COUNT_AND_REWARD, rates=(0.5, 1.5), weights=(0.3, 0.7), root_states=root, rate_categories=cats)
    assert np.array_equal(res["states"][0], root) and np.array_equal(res["categories"], cats)
    free = _tiny(Q3, [0.0, 1.0, 1.0], *COUNT_AND_REWARD, rates=(0.5, 1.5), weights=(0.3, 0.7))
    same = (free["states"][0] == root) & (free["categories"] == cats)
    assert same.any()                                                      # the branch streams do not depend on how the root was set
    assert np.array_equal(free["states"][:, same], res["states"][:, same]) and np.array_equal(free["values"][:, :, same], res["values"][:, :, same])


def test_rows_nobody_wants_change_nothing():
    rows = [[0, 0, -1], [-1, 0, 0], [1, 0, 1]]
    a = _tiny(Q3, [0.0, 1.0, 1.0], *COUNT_AND_REWARD, rows=rows)
    b = _tiny(Q3, [0.0, 1.0, 1.0], *COUNT_AND_REWARD)
    assert np.array_equal(a["states"], b["states"]) and np.array_equal(a["values"], b["values"])


def test_event_order_and_the_height_formula():
    heights = np.array([3.0, 2.0, 0.5])
    res = _tiny(Q3, [0.0, 1.0, 1.5], *COUNT_AND_REWARD, heights=heights, n=300)
    si, ro, tt = res["event_site"], res["event_row"], res["event_time"]
    key = si * 3 + ro
    assert np.all(np.diff(key) >= 0) and np.all(np.diff(tt)[np.diff(key) == 0] > 0)
    assert np.array_equal(np.bincount(key, minlength=900).reshape(300, 3).T, res["counts"])
    hp, hc = heights[np.array([0, 0, 1])[ro]], heights[ro]
    assert np.array_equal(res["event_heights"], hp + (tt / res["event_tau"]) * (hc - hp))
    assert np.all(res["event_heights"] < hp) and np.all(res["event_heights"] > hc)
    # a history's events chain: from = the previous to, the first from = the parent's state, the last to = the row's state
    fr, to = res["event_states"][:, 0], res["event_states"][:, 1]
    same = np.diff(key) == 0
    assert np.array_equal(fr[1:][same], to[:-1][same]) and np.all(fr != to)
    first = np.r_[True, ~same]
    last = np.r_[~same, True]
    assert np.array_equal(fr[first], res["states"][np.array([0, 0, 1])[ro[first]], si[first]])
    assert np.array_equal(to[last], res["states"][ro[last], si[last]])


def test_the_jump_cap_cuts_a_history_and_keeps_its_values():
    Q = np.array([[-1.0, 1.0], [1.0, -1.0]])
    res = hr.simulate([[0, 0, -1], [1, 0, 0]], [0.0, 1e9], Q[None], np.stack([np.ones((2, 2)), np.diag([1.0, 1.0])]), [0, hr.REWARDS],
                      [1.0], [1.0], [0.5, 0.5], 3, 1, events=False, max_jumps=2000)
    assert res["bad"] and res["cut"][1, 0] and res["counts"][1, 0] == 2000 and res["values"][0, 1, 0] == 2000.0
    assert 0.0 < res["values"][1, 1, 0] < 1e9                              # the reward so far, without a final term


def test_a_row_without_off_diagonal_weight_is_flagged():
    Q = np.array([[-1.0, 0.0], [1.0, -1.0]])                               # state 0 has a rate and nowhere to go
    res = hr.simulate([[0, 0, -1], [1, 0, 0]], [0.0, 50.0], Q[None], np.ones((1, 2, 2)), None, [1.0], [1.0], [0.5, 0.5], 3, 200)
    assert res["bad"] and res["cut"][1].any()
    assert np.all(res["states"][1][res["cut"][1]] == 0)


# ---- what the GPU tier rests on
@pytest.mark.parametrize("name", sorted(cc.CASES) + ["generators"])
def test_no_history_of_a_gpu_case_is_near_its_end_or_cut(name):
    res = cc.restated_generators() if name == "generators" else cc.restated(name)
    assert res["near"].sum() == 0 and not res["cut"].any() and not res["bad"]
    assert res["counts"].sum() == len(res["event_site"]) > 0


def test_no_history_of_the_other_gpu_seeds_is_near_its_end():
    """test_gpu_complete_history.py's other calls: the determinism seeds, the capacity case, the sharded shape."""
    c = cc.build("s4")
    for seed in cc.OTHER_SEEDS:
        res = cc.restate(c, seed=seed)
        assert res["near"].sum() == 0 and not res["bad"]
    res = cc.restate(c, seed=cc.SHARDED_SEED, site_count=cc.SHARDED_SITES)
    assert res["near"].sum() == 0 and not res["bad"]
