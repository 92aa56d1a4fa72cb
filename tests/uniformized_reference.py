"""Host restatement of beagleMi355SampleMarkovJumpsUniformized (include/beagle_mi355.h), from what an engine reads back.

It restates SubordinatedProcess (src/dr/inference/markovjumps/SubordinatedProcess.java: getMaxRate, constructDtmcMatrix,
getDtmcProbabilities, drawNumberOfChanges, computePdfNextChainState), UniformizedStateHistory.simulateConditionalOnEndingState,
UniformizedSubstitutionModel.computeCondStatMarkovJumps with RETURN_UNIFORMLY_DISTRIBUTED_EVENT, StateHistory's registered counts
and rewards, and MarkovJumpsBeagleTreeLikelihood.computeSampledMarkovJumpsForBranch (:473-509), with the engine's keyed SplitMix64
numbers.  Every product, quotient and sum is one IEEE double operation in the order the kernels form it (kernels_uniformized.hip),
so the histories agree exactly except where the device's exp() or log() rounds differently from the host's: a Poisson draw whose
cutoff lies within 1e-12 relative of a cumulative sum is flagged ``near``; times and values agree to rounding.

Vectorised over histories: one history per (simulant, row, pattern), driven step by step with masks.
"""
import numpy as np

import ancestral_reference as ar
import markov_jumps_reference as mr
from beast_mcmc_amd.markovjumps import java_double

STREAM_SALT = 0x6A09E667F3BCC909
MAX_TRIES = 1000
NEAR = 1e-12


def chain(Q):
    """(mu, R): mu = max_i -Q_ii in getMaxRate's order, R = Q / mu, then +1 on the diagonal (constructDtmcMatrix)."""
    Q = np.asarray(Q, dtype=np.float64)
    S = Q.shape[0]
    mu = -Q[0, 0]
    for i in range(1, S):
        if -Q[i, i] > mu:
            mu = -Q[i, i]
    R = Q / mu
    R[np.diag_indices(S)] += 1.0
    return float(mu), R


def table_length(mu, times, branch_rates, cat_rates):
    """N = min(1000, ceil(lambda + 20 sqrt(lambda)) + 40), lambda = mu * the largest tau of rows >= 1 and live categories."""
    times = np.asarray(times, dtype=np.float64)
    rates = np.ones(len(times)) if branch_rates is None else np.asarray(branch_rates, dtype=np.float64)
    cr = np.asarray(cat_rates, dtype=np.float64)
    cr = cr[cr > 0.0]
    tmax = float(np.max((times[1:] * rates[1:])[:, None] * cr[None, :])) if len(times) > 1 and len(cr) else 0.0
    lam = mu * max(tmax, 0.0)
    if not lam < 1000.0:
        return MAX_TRIES
    return min(MAX_TRIES, int(np.ceil(lam + 20.0 * np.sqrt(lam))) + 40)


def powers(R, N):
    """[N][S][S]: R^0 = I, R^1 = R, R^n = R^(n-1) R (MarkovJumpsCore.matrixMultiply: inner index ascending from 0)."""
    S = R.shape[0]
    out = np.zeros((max(N, 2), S, S))
    out[0] = np.eye(S)
    out[1] = R
    for n in range(2, N):
        out[n] = mr.mm(out[n - 1], R)
    return out


def _mix(z):
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(ar.MIX1)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(ar.MIX2)
        return z ^ (z >> np.uint64(31))


def stream(seed, key):
    """z of a history: SplitMix64's output for `key` from seed ^ 0x6A09E667F3BCC909 (uint64, elementwise over key)."""
    key = np.asarray(key, dtype=np.uint64)
    with np.errstate(over="ignore"):
        return _mix(np.uint64((seed ^ STREAM_SALT) & 0xFFFFFFFFFFFFFFFF) + (key + np.uint64(1)) * np.uint64(ar.GOLDEN))


def uniform(z, q):
    """u_q of streams z (elementwise; q scalar or array)."""
    z = np.asarray(z, dtype=np.uint64)
    q = np.asarray(q, dtype=np.uint64)
    with np.errstate(over="ignore"):
        v = _mix(z + (q + np.uint64(1)) * np.uint64(ar.GOLDEN))
    return (v >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def spacing(z, q):
    return -np.log(1.0 - uniform(z, q))


def draw_n(u0, i, j, tau, pij, mu, table, N):
    """SubordinatedProcess.drawNumberOfChanges with cutoff u0, elementwise -> (n, near): n = N is the fallback; near: some
    cumulative sum lies within 1e-12 relative of u0."""
    u0, tau, pij = (np.asarray(x, dtype=np.float64) for x in (u0, tau, pij))
    i, j = np.asarray(i, dtype=np.int64), np.asarray(j, dtype=np.int64)
    eff = mu * tau
    pre = np.exp(-eff)
    cdf = np.zeros(u0.shape)
    scale = np.ones(u0.shape)
    n = np.full(u0.shape, -1, dtype=np.int64)
    near = np.zeros(u0.shape, dtype=bool)
    active = np.ones(u0.shape, dtype=bool)
    step = 0
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        while active.any():
            if step == N:
                n = np.where(active, N, n)
                break
            if step > 0:
                scale = np.where(active, scale * eff, scale)
            if step > 1:
                scale = np.where(active, scale / float(step), scale)
            cdf = np.where(active, cdf + ((pre * scale) * table[step][i, j]) / pij, cdf)
            n = np.where(active, step, n)
            near |= active & (np.abs(u0 - cdf) <= NEAR * np.maximum(np.abs(u0), np.abs(cdf)))
            active = active & (u0 >= cdf)
            step += 1
    return n, near


def next_state_pdf(R_table, cur, end, n, m):
    """computePdfNextChainState: pdf[k] = R[cur][k] R^(n-m)[k][end] (unnormalised)."""
    return R_table[1][cur, :] * R_table[n - m][:, end]


def simulate(z, i, j, tau, pij, mu, table, N):
    """Histories of streams z from i to j over tau -> dict: "n", "near", "bad" per history; events "hist", "f", "from", "to" in
    (history, time) order."""
    H = len(z)
    S = table.shape[1]
    i, j = np.asarray(i, dtype=np.int64), np.asarray(j, dtype=np.int64)
    n, near = draw_n(uniform(z, 0), i, j, tau, pij, mu, table, N)
    bad = ~((pij > 0.0) & (pij <= ar.DBL_MAX))
    ev = []                                                     # (hist, order, f, from, to)
    one = ((n == 1) | (n == N)) & (i != j)
    h1 = np.nonzero(one)[0]
    ev.append((h1, np.zeros(len(h1), dtype=np.int64), uniform(z[h1], 1), i[h1], j[h1]))
    M = np.nonzero((n >= 2) & (n < N))[0]
    if len(M):
        nn, zm, jm = n[M], z[M], j[M]
        total = np.zeros(len(M))
        for q in range(1, int(nn.max()) + 2):
            total = np.where(q <= nn + 1, total + spacing(zm, q), total)
        run = np.zeros(len(M))
        cur = i[M].copy()
        for m in range(1, int(nn.max())):
            act = m < nn
            run = np.where(act, run + spacing(zm, m), run)
            pw = np.where(act, nn - m, 0)
            weights = [table[1][cur, k] * table[pw, k, jm] for k in range(S)]
            nxt, b = ar.draw_choice(weights, uniform(zm, nn + 1 + m), False)
            bad[M] |= act & b
            ch = act & (nxt != cur)
            ev.append((M[ch], np.full(ch.sum(), m), (run / total)[ch], cur[ch], nxt[ch]))
            cur = np.where(ch, nxt, cur)
        last = cur != jm
        run = np.where(last, run + spacing(zm, nn), run)
        ev.append((M[last], nn[last], (run / total)[last], cur[last], jm[last]))
    hist = np.concatenate([e[0] for e in ev]).astype(np.int64)
    order = np.concatenate([e[1] for e in ev]).astype(np.int64)
    srt = np.lexsort((order, hist))
    return {"n": n, "near": near, "bad": bad, "hist": hist[srt], "f": np.concatenate([e[2] for e in ev])[srt],
            "from": np.concatenate([e[3] for e in ev]).astype(np.int64)[srt],
            "to": np.concatenate([e[4] for e in ev]).astype(np.int64)[srt], "H": H}


def register_values(sim, i, tau, registers, flags):
    """[K][H]: every register over each history's events in time order (StateHistory.getTotalRegisteredCounts /
    getTotalReward, as the kernel sums them)."""
    H = sim["H"]
    K = len(registers)
    regs = np.asarray(registers, dtype=np.float64)
    acc = np.zeros((K, H))
    prev = np.zeros(H)
    last = np.asarray(i, dtype=np.int64).copy()
    hist = sim["hist"]
    rank = np.zeros(len(hist), dtype=np.int64)
    if len(hist):
        starts = np.r_[0, np.nonzero(np.diff(hist))[0] + 1]
        idx = np.arange(len(hist))
        rank = idx - np.repeat(starts, np.diff(np.r_[starts, len(hist)]))
    tau = np.asarray(tau, dtype=np.float64)
    for q in range(int(rank.max()) + 1 if len(rank) else 0):
        sel = rank == q
        h, f, fr, to = hist[sel], sim["f"][sel], sim["from"][sel], sim["to"][sel]
        t = f * tau[h]
        for k in range(K):
            if flags[k] & 1:
                acc[k, h] = acc[k, h] + regs[k][fr, fr] * (t - prev[h])
            else:
                acc[k, h] = acc[k, h] + regs[k][fr, to]
        prev[h] = t
        last[h] = to
    for k in range(K):
        if flags[k] & 1:
            acc[k] = acc[k] + regs[k][last, last] * (tau - prev)
    return acc


def restate(parents, times, branch_rates, heights, states, cats, cat_rates, matrices, Q, registers, flags, simulants, seed,
            pattern_count=None, patterns=None):
    """The whole call over the draw's `states` [n][P'] and `cats` [P'] (P' = the restated patterns; `patterns`: their indices in
    the alignment, default all; `pattern_count`: the alignment's P).  ``matrices`` [n][C][S][S] (row 0 ignored).  -> dict:
    "values" [K][n][P'], "pattern_totals" [K][P'], "row_totals" [K][n] (over the restated patterns, in pattern order),
    "event_counts" [n][P'], "event_heights", "event_states" [E][2] in (pattern, row, time) order, "fallbacks", "near" [n][P'],
    "bad", "N", "n" [simulants][n][P'] (-1 where no history is simulated), "event_f" (the events' fractions of tau)."""
    parents = np.asarray(parents, dtype=np.int64)
    nrows, P = states.shape
    pats = np.arange(P) if patterns is None else np.asarray(patterns, dtype=np.int64)
    GP = P if pattern_count is None else pattern_count
    times = np.asarray(times, dtype=np.float64)
    rates = np.ones(nrows) if branch_rates is None else np.asarray(branch_rates, dtype=np.float64)
    heights = np.zeros(nrows) if heights is None else np.asarray(heights, dtype=np.float64)
    cat_rates = np.asarray(cat_rates, dtype=np.float64)
    flags = [int(f) for f in flags]
    K = len(registers)
    mu, R = chain(Q)
    N = table_length(mu, times, rates, cat_rates)
    table = powers(R, N)
    cats = np.asarray(cats, dtype=np.int64)
    st = states.astype(np.int64)
    rc = cat_rates[cats]                                          # [P']
    rr, pp = np.meshgrid(np.arange(1, nrows), np.arange(len(pats)), indexing="ij")
    rr, pp = rr.ravel(), pp.ravel()
    live = rc[pp] > 0.0
    rr, pp = rr[live], pp[live]
    i, j = st[parents[rr], pp], st[rr, pp]
    tau = (times[rr] * rates[rr]) * rc[pp]
    pij = np.asarray(matrices, dtype=np.float64)[rr, cats[pp], i, j]
    values = np.zeros((K, nrows, len(pats)))
    sums = np.zeros((K, len(rr)))
    near = np.zeros((nrows, len(pats)), dtype=bool)
    counts = np.zeros((nrows, len(pats)), dtype=np.int32)
    nout = np.full((simulants, nrows, len(pats)), -1, dtype=np.int64)
    fallbacks, bad = 0, False
    ev = None
    for s in range(simulants):
        key = (np.uint64(s) * np.uint64(nrows) + rr.astype(np.uint64)) * np.uint64(GP) + pats[pp].astype(np.uint64)
        z = stream(seed, key)
        sim = simulate(z, i, j, tau, pij, mu, table, N)
        acc = register_values(sim, i, tau, registers, flags)
        sums = sums + acc
        near[rr, pp] |= sim["near"]
        nout[s, rr, pp] = sim["n"]
        fallbacks += int((sim["n"] == N).sum())
        bad |= bool(sim["bad"].any())
        if s == 0:
            ev = sim
            counts[rr, pp] = np.bincount(sim["hist"], minlength=len(rr))
    for k in range(K):
        v = sums[k] / float(simulants)
        if flags[k] & 2:
            v = v / (rates[rr] * rc[pp])
        values[k, rr, pp] = v
        if flags[k] & 3 == 3:                                     # rate_c <= 0: MarkovJumpsBeagleTreeLikelihood.java:553-559
            dr, dp = np.meshgrid(np.arange(1, nrows), np.nonzero(~(rc > 0.0))[0], indexing="ij")
            dr, dp = dr.ravel(), dp.ravel()
            values[k, dr, dp] = np.where(st[parents[dr], dp] == st[dr, dp], times[dr], 0.0)
    bad |= not np.isfinite(values).all()
    tot = np.zeros((K, len(pats)))
    for r in range(1, nrows):
        tot = tot + values[:, r]
    h = ev["hist"]
    er, ep = rr[h], pp[h]
    srt = np.lexsort((np.arange(len(h)), er, ep))                 # pattern, then row, then time (already in time order)
    hp, hc = heights[parents[er]], heights[er]
    f = ev["f"]
    ev_heights = (hp + f * (hc - hp))[srt]
    ev_states = np.stack([ev["from"], ev["to"]], axis=1).astype(np.uint8)[srt]
    return {"values": values, "pattern_totals": tot, "row_totals": values.sum(axis=2), "event_counts": counts,
            "event_heights": ev_heights, "event_states": ev_states, "event_f": f[srt], "event_rows": er[srt],
            "event_patterns": ep[srt], "fallbacks": fallbacks, "near": near, "bad": bad, "N": N, "n": nout, "mu": mu, "table": table}


def history_strings(event_rows, event_patterns, event_heights, event_states, node_of_row, node_count, pattern_count, codes,
                    compact=False):
    """[node][pattern] -> the reference's history string (StateHistory.toStringChanges, addEventToStringBuilder): "{}" when the
    branch has no change at the site; with `compact`, the site (1-based) leads every event."""
    out = [["{}"] * pattern_count for _ in range(node_count)]
    parts = {}
    for r, p, h, (a, b) in zip(event_rows, event_patterns, event_heights, event_states):
        body = "{" + ("%d," % (p + 1) if compact else "") + java_double(h) + "," + codes[a] + "," + codes[b] + "}"
        parts.setdefault((int(node_of_row[r]), int(p)), []).append(body)
    for (n, p), v in parts.items():
        out[n][p] = "{" + ",".join(v) + "}"
    return out
