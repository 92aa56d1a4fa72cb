"""Host restatement of beagleMi355SimulateCompleteHistories (include/beagle_mi355.h), vectorised over sites.

Written from the call's documented behaviour: a rate category per site (given, or drawn from the category weights when there is
more than one, else 0), a root state per site (given, or drawn from the state frequencies) and, for every other row of the pre-order
list, StateHistory.simulateUnconditionalOnEndingState (src/dr/inference/markovjumps/StateHistory.java:324-354) from the parent's
realised state over tau = category rate x branch length, as CompleteHistorySimulator.traverse runs it
(src/dr/app/beagle/tools/CompleteHistorySimulator.java:420-496); the history's ending state is the row's state.

A draw is the header's cumulative form: cum_i = cum_{i-1} + w_i from 0.0 in index order (one IEEE addition each; numpy does not
contract to FMA), U = u * cum_{n-1}, the first i with U < cum_i, else the largest i with w_i > 0.  The streams are the engine's
stateless SplitMix64 outputs: z = the output for key row * site_count + site from seed ^ 0x3C6EF372FE94F82B, u_q its (q + 1)-th
output as (x >> 11) * 2^-53; row 0: u_0 the root state, u_1 the category; row r >= 1: u_(2m) waiting time m, u_(2m+1) the state after
it.  Every sum is formed in the order the header states, so states, counts and count-register values must agree with the device's
bit for bit, and rewards and event heights differ only where log() does.
"""
import numpy as np

import ancestral_reference as ar
import uniformized_reference as ur
from robust_counting_reference import block_totals  # noqa: F401  (the row totals' fixed order)

STREAM_SALT = 0x3C6EF372FE94F82B
MAX_JUMPS = 100000
NEAR = 1e-12
REWARDS = 1


def stream(seed, key):
    """z of a history: SplitMix64's output for `key` from seed ^ 0x3C6EF372FE94F82B (uint64, elementwise over key)."""
    return ar.splitmix64(seed ^ STREAM_SALT, key)


def line(w, own=-1):
    """One jump-table line: (cum [n], total, last_positive, bad) of the weights w with entry `own` taken as 0."""
    w = np.array(w, dtype=np.float64)
    if own >= 0:
        w[own] = 0.0
    cum = np.empty_like(w)
    run, last = 0.0, 0
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(len(w)):
            run = run + w[i]
            cum[i] = run
            if w[i] > 0.0:
                last = i
    bad = not (run > 0.0 and run <= ar.DBL_MAX)
    return cum, run, last, bad


def pick(cum, total, last, u):
    """cum [m, n], total [m], last [m], u [m] -> the first i with u * total < cum_i, else last."""
    with np.errstate(invalid="ignore"):
        above = (u * total)[:, None] < cum
    return np.where(above.any(axis=1), np.argmax(above, axis=1), last)


def generator_tables(Q):
    """Q [S][S] -> (cum [S][S], total [S], last [S], bad [S], rate [S])."""
    Q = np.asarray(Q, dtype=np.float64)
    S = Q.shape[0]
    lines = [line(Q[i], i) for i in range(S)]
    return (np.array([x[0] for x in lines]), np.array([x[1] for x in lines]), np.array([x[2] for x in lines], dtype=np.int64),
            np.array([x[3] for x in lines], dtype=bool), -np.diag(Q).copy())


def simulate(rows, lengths, generators, registers, flags, cat_rates, cat_weights, freqs, seed, site_count, heights=None,
             root_states=None, rate_categories=None, sites=None, events=True, max_jumps=MAX_JUMPS):
    """The call for `rows` ([n][3] {outRow, qIndex, parentRow}, root first; outRow is not looked at) -> dict:
    states uint8 [n, m] BY ROW, categories int32 [m], values [K, n, m], site_totals [K, m], counts int32 [n, m], near [n, m] (some
    event time of the history lies within 1e-12 relative of tau: the one place a last-bit difference in log() could change a
    state or a count), cut [n, m] (given up at max_jumps or on a failed draw), bad (a draw failed or a history was cut), rate_c [m] (the
    sites' category rates); with `events`: event_site, event_row, event_time, event_tau, event_states [E, 2] in (site, row, time) order and, with
    `heights`, event_heights.  `sites`: restate only these site indices (default all; m = their number)."""
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, 3)
    n = len(rows)
    lengths = np.asarray(lengths, dtype=np.float64)
    w, f, rates = (np.asarray(x, dtype=np.float64) for x in (cat_weights, freqs, cat_rates))
    C, S = len(w), len(f)
    gens = np.asarray(generators, dtype=np.float64).reshape(-1, S, S)
    regs = np.asarray(registers, dtype=np.float64).reshape(-1, S, S)
    K = regs.shape[0]
    reward = np.zeros(K, dtype=bool) if flags is None else (np.asarray(flags).reshape(-1) & REWARDS) != 0
    sites = np.arange(site_count, dtype=np.int64) if sites is None else np.asarray(sites, dtype=np.int64)
    m = len(sites)
    gsite = sites.astype(np.uint64)
    any_bad = False

    z0 = stream(seed, gsite)
    if rate_categories is not None:
        cats = np.asarray(rate_categories, dtype=np.int64)[sites]
    elif C > 1:
        cum, total, last, bad = line(w)
        any_bad |= bad
        cats = np.zeros(m, dtype=np.int64) if bad else pick(np.broadcast_to(cum, (m, C)), np.full(m, total), np.full(m, last),
                                                            ur.uniform(z0, 1))
    else:
        cats = np.zeros(m, dtype=np.int64)
    states = np.zeros((n, m), dtype=np.uint8)
    if root_states is not None:
        states[0] = np.asarray(root_states, dtype=np.uint8)[sites]
    else:
        cum, total, last, bad = line(f)
        any_bad |= bad
        if not bad:
            states[0] = pick(np.broadcast_to(cum, (m, S)), np.full(m, total), np.full(m, last), ur.uniform(z0, 0))
    rate_c = rates[cats]

    values = np.zeros((K, n, m))
    counts = np.zeros((n, m), dtype=np.int32)
    near = np.zeros((n, m), dtype=bool)
    cut = np.zeros((n, m), dtype=bool)
    ev = []                                                   # (site index, row, jump number, t, from, to)
    tables = {}
    for r in range(1, n):
        q, parent = int(rows[r, 1]), int(rows[r, 2])
        if q not in tables:
            tables[q] = generator_tables(gens[q])
        cumQ, totalQ, lastQ, badQ, rateQ = tables[q]
        tau = rate_c * lengths[r]
        with np.errstate(over="ignore"):
            z = stream(seed, np.uint64(r) * np.uint64(site_count) + gsite)
        cur = states[parent].astype(np.int64)
        t, t_prev = np.zeros(m), np.zeros(m)
        v = np.zeros((K, m))
        active = t < tau
        step = 0
        while active.any():
            idx = np.nonzero(active)[0]
            c = cur[idx]
            rate = rateQ[c]
            alive = rate > 0.0
            active[idx[~alive]] = False
            idx, c, rate = idx[alive], c[alive], rate[alive]
            if idx.size == 0:
                break
            tn = t[idx] + (-1.0 * np.log(1.0 - ur.uniform(z[idx], 2 * step))) / rate
            t[idx] = tn
            near[r, idx] |= np.abs(tn - tau[idx]) <= NEAR * tau[idx]
            jump = tn < tau[idx]
            active[idx[~jump]] = False
            j, cj, tj = idx[jump], c[jump], tn[jump]
            if j.size:
                if step == max_jumps:
                    cut[r, j] = True
                    active[j] = False
                    break
                none = badQ[cj]
                cut[r, j[none]] = True
                active[j[none]] = False
                j, cj, tj = j[~none], cj[~none], tj[~none]
                nxt = pick(cumQ[cj], totalQ[cj], lastQ[cj], ur.uniform(z[j], 2 * step + 1))
                for k in range(K):
                    if reward[k]:
                        v[k, j] = v[k, j] + regs[k, cj, cj] * (tj - t_prev[j])
                    else:
                        v[k, j] = v[k, j] + regs[k, cj, nxt]
                if events:
                    ev.append((j, np.full(j.size, r), np.full(j.size, step), tj, cj, nxt))
                t_prev[j] = tj
                cur[j] = nxt
                counts[r, j] += 1
            step += 1
        ok = ~cut[r]
        for k in range(K):
            if reward[k]:
                v[k, ok] = v[k, ok] + regs[k, cur[ok], cur[ok]] * (tau[ok] - t_prev[ok])
        values[:, r] = v
        states[r] = cur
    site_totals = np.zeros((K, m))
    for r in range(1, n):
        site_totals = site_totals + values[:, r]
    any_bad = bool(any_bad or cut.any())
    out = {"states": states, "categories": cats.astype(np.int32), "values": values, "site_totals": site_totals, "counts": counts,
           "near": near, "cut": cut, "bad": any_bad, "rate_c": rate_c}
    if events:
        if ev:
            si, ro, st, tt, fr, to = (np.concatenate([e[i] for e in ev]) for i in range(6))
        else:
            si = ro = st = fr = to = np.zeros(0, dtype=np.int64)
            tt = np.zeros(0)
        order = np.lexsort((st, ro, si))
        si, ro, tt, fr, to = si[order], ro[order], tt[order], fr[order], to[order]
        tau_e = rate_c[si] * lengths[ro]
        out.update(event_site=si, event_row=ro, event_time=tt, event_tau=tau_e,
                   event_states=np.stack([fr, to], axis=1).astype(np.uint8).reshape(-1, 2))
        if heights is not None:
            h = np.asarray(heights, dtype=np.float64)
            hp, hc = h[rows[ro, 2]], h[ro]
            out["event_heights"] = hp + (tt / tau_e) * (hc - hp)
    return out


def row_totals(values):
    """[K][n][m] -> [K][n]: the device's fixed order (robust_counting_reference.block_totals), row 0 zero."""
    out = block_totals(values)
    out[:, 0] = 0.0
    return out
