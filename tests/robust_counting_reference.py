"""Host restatement of beagleMi355RobustCounts and beagleMi355SimulateUnconditionedCounts (include/beagle_mi355.h).

It restates ProductChainSubstitutionModel.computeKroneckerSumsAndProducts (src/dr/evomodel/substmodel/ProductChainSubstitutionModel
.java:301-362), MarkovJumpsSubstitutionModel's registration (MarkovJumpsSubstitutionModel.java:84-131), MarkovJumpsCore's
conditional mean (src/dr/inference/markovjumps/MarkovJumpsCore.java:84-103, 198-221) over the product chain's own transition
probabilities (BaseSubstitutionModel.java:206-240), the gather of CodonPartitionedRobustCounting (:216-307) and
StateHistory.simulateUnconditionalOnEndingState (StateHistory.java:324-354) with the engine's stateless random numbers.

Every product is one IEEE double operation and every matrix product sums over its inner index in ascending order from 0.0
(markov_jumps_reference.mm), as kernels_robustcounts.hip forms them: the tables differ only where exp() does, and a simulated
history only where log() moves an event time across the end of its interval.
"""
import numpy as np

import ancestral_reference as ar
import markov_jumps_reference as mr
import uniformized_reference as ur

STREAM_SALT = 0xBB67AE8584CAA73B
MAX_JUMPS = 100000
NEAR = 1e-12


def product_chain(eigs, site_rates):
    """(U, U^-1, lambda, Q) of the product chain: Q and eigenvalues of every base model times its site rate, Q the Kronecker sum,
    eigenvalues added, eigenvectors Kronecker-multiplied (first model most significant), the inverse through the transpose."""
    U = UiT = lam = Q = None
    for eig, rate in zip(eigs, site_rates):
        evec, ievc, evals = (np.asarray(x, dtype=np.float64) for x in (eig.evec, eig.ievc, eig.evals))
        q = mr.q_from_eigen(evec, ievc, evals)
        if rate != 1.0:
            q, evals = rate * q, rate * evals
        if U is None:
            U, UiT, lam, Q = evec, ievc.T, evals, q
            continue
        m, n = Q.shape[0], q.shape[0]
        Q = np.kron(Q, np.eye(n)) + np.kron(np.eye(m), q)
        lam = np.kron(lam, np.ones(n)) + np.kron(np.ones(m), evals)
        U, UiT = np.kron(U, evec), np.kron(UiT, ievc.T)
    return np.ascontiguousarray(U), np.ascontiguousarray(UiT.T), np.ascontiguousarray(lam), np.ascontiguousarray(Q)


def codon_registers(table):
    """(syn, nonsyn) [64][64] from a genetic-code table string (codon i * 16 + j * 4 + k): one position differs, both sense."""
    syn, non = np.zeros((64, 64)), np.zeros((64, 64))
    for u in range(64):
        for v in range(64):
            pos = [(u >> sh) & 3 != (v >> sh) & 3 for sh in (4, 2, 0)]
            if sum(pos) == 1 and table[u] != "*" and table[v] != "*":
                (syn if table[u] == table[v] else non)[u, v] = 1.0
    return syn, non


def register_m(U, Ui, Q, R):
    """M = U^-1 ((Q o R, R's diagonal as 0) U)."""
    Rz = np.array(R, dtype=np.float64)
    np.fill_diagonal(Rz, 0.0)
    return mr.mm(Ui, mr.mm(Q * Rz, U))


def transition(U, Ui, lam, tau):
    """P = |U (diag(e^(lambda tau)) U^-1)|, [..., S, S] for tau of batch shape."""
    e = np.exp(lam * np.asarray(tau, dtype=np.float64)[..., None])
    return np.abs(mr.mm(U, e[..., :, None] * Ui))


def tables(U, Ui, lam, Q, registers, taus):
    """(Cond [K][n][S][S], J, P): rows 1..n-1 from taus[1:], row 0 all 0."""
    taus = np.asarray(taus, dtype=np.float64)
    n, S, K = len(taus), U.shape[0], len(registers)
    cond, J = np.zeros((K, n, S, S)), np.zeros((K, n, S, S))
    P = np.zeros((n, S, S))
    P[1:] = transition(U, Ui, lam, taus[1:])
    for k in range(K):
        M = register_m(U, Ui, Q, registers[k])
        J[k, 1:] = mr.joint_precompute(U, Ui, lam, M, taus[1:])
        with np.errstate(divide="ignore", invalid="ignore"):
            cond[k, 1:] = J[k, 1:] / P[1:]
    return cond, J, P


def floors(U, Ui, lam, Q, registers, taus, J, P):
    """[K][n][S][S]: 1e-15 x (magJ / P + |J| magP / P^2) with magJ = |U| ((A^ o |M|) |U^-1|), magP = |U| diag(e) |U^-1| and
    A^ = |A| on a tie, else (e_a + e_b) / |la - lb| — what an entry moves by when exp() is off in its last bit (non-finite: 0)."""
    taus = np.asarray(taus, dtype=np.float64)[1:]
    e = np.exp(lam[None, :] * taus[:, None])
    ea, eb = e[:, :, None], e[:, None, :]
    d = np.abs(lam[:, None] - lam[None, :])
    with np.errstate(divide="ignore", invalid="ignore"):
        A = np.where(d < 1e-7, np.abs(ea * taus[:, None, None]), (ea + eb) / d)
    magP = np.abs(U) @ (e[:, :, None] * np.abs(Ui))
    out = np.zeros_like(J)
    for k, R in enumerate(registers):
        M = np.abs(register_m(U, Ui, Q, R))
        magJ = np.abs(U) @ ((A * M) @ np.abs(Ui))
        with np.errstate(divide="ignore", invalid="ignore"):
            v = 1e-15 * (magJ / P[1:] + np.abs(J[k, 1:]) * magP / (P[1:] * P[1:]))
        out[k, 1:] = np.where(np.isfinite(v), v, 0.0)
    return out


def codons(states):
    """[3][n][P] position states -> [n][P] codon states s0 * 16 + s1 * 4 + s2."""
    st = np.asarray(states).astype(np.int64)
    return st[0] * 16 + st[1] * 4 + st[2]


def gather(table, codon, parents, include=None):
    """-> (values [K][n][P], site totals [K][P] over the included rows 1.. in row order, branch totals [K][n] over the sites)."""
    K, n = table.shape[:2]
    P = codon.shape[1]
    vals = np.zeros((K, n, P))
    for r in range(1, n):
        vals[:, r] = table[:, r, codon[parents[r]], codon[r]]
    tot = np.zeros((K, P))
    for r in range(1, n):
        if include is None or include[r]:
            tot = tot + vals[:, r]
    return vals, tot, vals.sum(axis=2)


def stream(seed, key):
    """z of a history: SplitMix64's output for `key` from seed ^ 0xBB67AE8584CAA73B (uint64, elementwise over key)."""
    return ar.splitmix64(seed ^ STREAM_SALT, key)


def unconditioned(Q, pi, lengths, site_count, registers, seed):
    """-> (values [K][L][site_count], near [L][site_count] bool, cut [L][site_count] bool).  One history per (length row, site),
    all of them advanced together, each by the rules of the header: u_0 the start state, u_(2m+1) waiting time m, u_(2m+2) the
    state after it.  near: some event time of the history was within 1e-12 relative of its end (the one place a last-bit
    difference in log() could change the value); cut: given up at MAX_JUMPS jumps or on a failed draw."""
    Q = np.asarray(Q, dtype=np.float64)
    S = Q.shape[0]
    regs = np.asarray(registers, dtype=np.float64).reshape(-1, S, S)
    lengths = np.asarray(lengths, dtype=np.float64)
    L, N = len(lengths), len(lengths) * site_count
    key = np.arange(N, dtype=np.uint64)
    length = np.repeat(lengths, site_count)
    z = stream(seed, key)
    cur, bad = ar.draw_choice([np.full(N, float(pi[i])) for i in range(S)], ur.uniform(z, 0), False)
    cut = bad.copy()
    t = np.zeros(N)
    vals = np.zeros((regs.shape[0], N))
    near = np.zeros(N, dtype=bool)
    active = ~bad & (t < length)
    q, jumps = 1, 0
    while active.any():
        idx = np.nonzero(active)[0]
        c = cur[idx]
        rate = -Q[c, c]
        alive = rate > 0.0
        active[idx[~alive]] = False
        idx, c, rate = idx[alive], c[alive], rate[alive]
        if idx.size == 0:
            break
        tn = t[idx] + (-1.0 * np.log(1.0 - ur.uniform(z[idx], q))) / rate
        t[idx] = tn
        near[idx] |= np.abs(tn - length[idx]) <= NEAR * length[idx]
        jump = tn < length[idx]
        active[idx[~jump]] = False
        j, cj = idx[jump], c[jump]
        if j.size:
            if jumps == MAX_JUMPS:
                cut[j] = True
                active[j] = False
                break
            W = Q[cj].copy()
            W[np.arange(j.size), cj] = 0.0
            nxt, none = ar.draw_choice([W[:, i] for i in range(S)], ur.uniform(z[j], q + 1), False)
            ok = ~none
            vals[:, j[ok]] = vals[:, j[ok]] + regs[:, cj[ok], nxt[ok]]
            cur[j[ok]] = nxt[ok]
            cut[j[none]] = True
            active[j[none]] = False
        q += 2
        jumps += 1
    shape = (L, site_count)
    return vals.reshape((-1,) + shape), near.reshape(shape), cut.reshape(shape)


def block_totals(values):
    """[K][L][N] -> [K][L]: the device's fixed order — per 256 consecutive sites a wave's 64 by an xor tree (distances 32 .. 1),
    the four waves in wave order, then the blocks in ascending order."""
    K, L, N = values.shape
    blocks = (N + 255) // 256
    v = np.zeros((K, L, blocks * 256))
    v[:, :, :N] = values
    w = v.reshape(K, L, blocks, 4, 64)
    for d in (32, 16, 8, 4, 2, 1):
        w = w + w[..., np.arange(64) ^ d]
    w = w[..., 0]
    b = ((w[..., 0] + w[..., 1]) + w[..., 2]) + w[..., 3]
    out = np.zeros((K, L))
    for i in range(blocks):
        out = out + b[:, :, i]
    return out
