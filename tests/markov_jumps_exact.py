"""An exact yardstick for the Markov-jump and robust-count tables, independent of the eigen formula the kernels and their host
restatements (tests/markov_jumps_reference.py, tests/robust_counting_reference.py) share.

Cond[i][j] = J(tau)[i][j] / P(tau)[i][j] with [[P, J], [0, P]] = expm(tau [[Q, B], [0, Q]]) (Van Loan 1978; Minin & Suchard 2008,
eq. 9), B the rate-registration matrix: Q o R with a zero diagonal for counts, diag(w) for rewards.  ``exact_tables`` takes that
exponential by scaling and squaring of a Taylor series in long double (64-bit significand), block by block: no eigenvalue enters,
so neither the difference quotient (e^(la t) - e^(lb t)) / (la - lb) nor its tie threshold does.  Q is U diag(lambda) U^-1 in
long double from the float64 arrays the engine was handed or read back: both sides are functions of the same inputs.

One error metric everywhere: |v - exact| / max(|exact|, unit), unit the largest value the register can take in one event on that
branch — max |R_k| for counts, max |w| tau for rewards, either divided by branch rate x category rate where the register is scaled by
time — so that an O(tau^2) entry cannot dominate a maximum through its relative error alone.

The Markov-jump call returns gathered values only, so a case is a two-tip tree whose tips run over all S^2 ordered state pairs,
repeated R times: with both tips known and different the drawn root is either tip's state with equal odds however short the branch
(pi_i P_ij = pi_j P_ji), so every pattern forces an off-diagonal gather.  ``expected_missing_share`` gives, from the model alone, the
expected share of table entries no pattern gathers; ``repeats`` picks the smallest R that crosses a 256-pattern workgroup and
keeps that share at most 0.1 %.
"""
import functools

import numpy as np

import helpers
import markov_jumps_reference as mr
import robust_counting_cases as rcases
import robust_counting_reference as rr
from beast_mcmc_amd.inputs import substmodel, synth, trees

LD = np.longdouble
BOUND = 1e-10                     # the project's bound on the engine
MARGIN, SLACK = 4.0, 1e-13        # where the formula itself loses digits: device <= MARGIN x restatement + SLACK
COVERAGE_EXPECTED, COVERAGE_DRAWN = 1e-3, 1e-2


# ---- the yardstick ------------------------------------------------------------------------------------------------------------

def exact_q(U, Ui, lam):
    """Q = U diag(lambda) U^-1 in long double from float64 arrays."""
    return (np.asarray(U, dtype=LD) * np.asarray(lam, dtype=LD)[None, :]) @ np.asarray(Ui, dtype=LD)


def exact_rate_registration(Q, R, kind):
    """B in long double: counts Q o R with a zero diagonal; rewards diag(R[i][i])."""
    R = np.asarray(R, dtype=LD).reshape(Q.shape)
    if kind == "rewards":
        return np.diag(np.diag(R))
    B = Q * R
    np.fill_diagonal(B, 0.0)
    return B


def exact_tables(U, Ui, lam, rate_reg, tau):
    """-> (J, P) as np.longdouble: the top-right and top-left blocks of expm(tau [[Q, B], [0, Q]]).  ``rate_reg``: B [S][S], or
    [K][S][S] for K registers over one P (then J is [K][S][S]).  The block matrix is scaled by 2^-s to a row-sum norm of at most
    1/4, its exponential summed term by term (term_n = term_(n-1) M / n, in blocks: Tj <- (Tp B + Tj Q) / n, Tp <- Tp Q / n) until
    a term is below 1e-40, then squared s times ([[P, J], [0, P]]^2 = [[P P, P J + J P], [0, P P]])."""
    A = exact_q(U, Ui, lam) * LD(tau)
    B = np.asarray(rate_reg, dtype=LD) * LD(tau)
    S = A.shape[0]
    norm = float(np.abs(A).sum(axis=1).max() + np.abs(B).sum(axis=-1).max())
    s = 0
    while norm > 0.25:
        norm, s = norm / 2.0, s + 1
    A, B = A / LD(2.0) ** s, B / LD(2.0) ** s
    P, J = np.eye(S, dtype=LD), np.zeros(B.shape, dtype=LD)
    Tp, Tj = P.copy(), J.copy()
    for n in range(1, 60):
        Tj = (Tp @ B + Tj @ A) / LD(n)
        Tp = (Tp @ A) / LD(n)
        P, J = P + Tp, J + Tj
        if max(float(np.abs(Tp).max()), float(np.abs(Tj).max())) < 1e-40:
            break
    for _ in range(s):
        J = P @ J + J @ P
        P = P @ P
    return J, P


def exact_cond(U, Ui, lam, registers, kinds, scale_by_time, time, rate, cat_rates):
    """-> (Cond [K][C][S][S] long double, unit [K][C] float64) of one branch, with markov_jumps_reference.tables' rules: tau =
    (time x rate) x category rate; a register that scales by time is divided by rate x category rate; a category of rate <= 0 has
    an all-zero table, or ``time`` on the diagonal for a reward register that scales by time."""
    S, K, C = np.asarray(U).shape[0], len(registers), len(cat_rates)
    Q = exact_q(U, Ui, lam)
    B = np.stack([exact_rate_registration(Q, registers[k], kinds[k]) for k in range(K)])
    cond, unit = np.zeros((K, C, S, S), dtype=LD), np.zeros((K, C))
    for c, rc in enumerate(cat_rates):
        tau = (float(time) * float(rate)) * float(rc)
        live = rc > 0.0
        if live:
            J, P = exact_tables(U, Ui, lam, B, tau)
        for k in range(K):
            off = np.asarray(registers[k], dtype=np.float64).reshape(S, S).copy()
            if kinds[k] == "rewards":
                unit[k, c] = np.abs(np.diag(off)).max() * tau
            else:
                np.fill_diagonal(off, 0.0)
                unit[k, c] = np.abs(off).max()
            if not live:
                if kinds[k] == "rewards" and scale_by_time[k]:
                    cond[k, c] = np.eye(S, dtype=LD) * LD(time)
                    unit[k, c] = np.abs(np.diag(off)).max() * float(time)
                continue
            with np.errstate(divide="ignore", invalid="ignore"):
                cond[k, c] = J[k] / P
            if scale_by_time[k]:
                cond[k, c] = cond[k, c] / (LD(rate) * LD(rc))
                unit[k, c] = unit[k, c] / (float(rate) * float(rc))
    return cond, unit


def metric(v, exact, unit):
    """|v - exact| / max(|exact|, unit) elementwise, as float64 (``unit`` broadcasts)."""
    exact = np.asarray(exact, dtype=LD)
    with np.errstate(divide="ignore", invalid="ignore"):
        return (np.abs(np.asarray(v, dtype=LD) - exact) / np.maximum(np.abs(exact), np.asarray(unit, dtype=LD))).astype(np.float64)


def bound_for(regime, restatement_worst):
    """What a candidate's worst metric value may be: the project's bound where the eigen formula is well conditioned or exactly
    tied; elsewhere MARGIN x what the restatement itself loses on the same entries, plus SLACK."""
    return BOUND if regime in ("well", "tied", "tied-device") else MARGIN * restatement_worst + SLACK


def judge(regime, candidate, restatement, exact, unit, mask=None):
    """Per register (the leading axis): -> (worst metric value of ``candidate``, of ``restatement``, the bound on the former), over
    the entries of ``mask`` (default: all) at which the exact value and the restatement are both finite; a candidate that is not
    finite there has an infinite metric value.  The candidate is never what a bound or the set of entries is derived from."""
    K = len(candidate)
    worst_c, worst_r, bounds = np.zeros(K), np.zeros(K), np.zeros(K)
    u = np.broadcast_to(unit, np.shape(exact))
    for k in range(K):
        ok = np.isfinite(np.asarray(exact[k], dtype=np.float64)) & np.isfinite(restatement[k]) & (u[k] > 0.0)
        if mask is not None:
            ok = ok & mask
        if ok.any():
            mc = metric(np.asarray(candidate[k])[ok], np.asarray(exact[k])[ok], u[k][ok])
            worst_c[k] = np.inf if np.isnan(mc).any() else mc.max()
            worst_r[k] = metric(restatement[k][ok], np.asarray(exact[k])[ok], u[k][ok]).max()
        bounds[k] = bound_for(regime, worst_r[k])
    return worst_c, worst_r, bounds


def mpmath_cond(U, Ui, lam, registers, kinds, scale_by_time, time, rate, cat_rates, digits=50):
    """exact_cond's tables once more, by mpmath's matrix exponential of the whole 2S x 2S block matrix at ``digits`` digits ->
    [K][C] lists of mpmath matrices (live categories only)."""
    import mpmath
    S = np.asarray(U).shape[0]
    with mpmath.workdps(digits):
        Um, Uim = mpmath.matrix(np.asarray(U).tolist()), mpmath.matrix(np.asarray(Ui).tolist())
        Q = Um * mpmath.diag([mpmath.mpf(float(x)) for x in lam]) * Uim
        out = []
        for k, R in enumerate(registers):
            R = np.asarray(R, dtype=np.float64).reshape(S, S)
            B = mpmath.zeros(S)
            for i in range(S):
                for j in range(S):
                    if kinds[k] == "rewards":
                        B[i, j] = mpmath.mpf(float(R[i, i])) if i == j else 0
                    else:
                        B[i, j] = Q[i, j] * mpmath.mpf(float(R[i, j])) if i != j else 0
            per_cat = []
            for rc in cat_rates:
                tau = mpmath.mpf((float(time) * float(rate)) * float(rc))
                big = mpmath.zeros(2 * S)
                for i in range(S):
                    for j in range(S):
                        big[i, j] = big[S + i, S + j] = Q[i, j] * tau
                        big[i, S + j] = B[i, j] * tau
                E = mpmath.expm(big, method="taylor")
                scale = mpmath.mpf(float(rate)) * mpmath.mpf(float(rc)) if scale_by_time[k] else mpmath.mpf(1)
                per_cat.append(mpmath.matrix(S, S))
                for i in range(S):
                    for j in range(S):
                        per_cat[-1][i, j] = E[i, S + j] / E[i, j] / scale
            out.append(per_cat)
    return out


def metric_against_mpmath(cond, unit, mp_cond, digits=50):
    """The metric of a long double table [K][C][S][S] against mpmath_cond's, the differences taken in mpmath -> max per register."""
    import mpmath
    K, C, S = cond.shape[0], cond.shape[1], cond.shape[2]
    worst = np.zeros(K)
    with mpmath.workdps(digits):
        for k in range(K):
            for c in range(C):
                for i in range(S):
                    for j in range(S):
                        hi = float(cond[k, c, i, j])
                        v = mpmath.mpf(hi) + mpmath.mpf(float(cond[k, c, i, j] - LD(hi)))        # the long double, exactly
                        e = mp_cond[k][c][i, j]
                        worst[k] = max(worst[k], float(abs(v - e) / max(abs(e), mpmath.mpf(float(unit[k, c])))))
    return worst


# ---- Markov-jump cases -------------------------------------------------------------------------------------------------------

def equal_rates(pi):
    """Equal exchangeabilities with frequencies pi (JC, F81 and their 20- and 61-state kin): S - 1 tied eigenvalues."""
    S = len(pi)
    return np.ones(S * (S - 1) // 2), np.asarray(pi, dtype=np.float64)


class JumpCase:
    """One two-tip Markov-jump case: a reversible model (upper-triangle relative rates + frequencies), a site model, one branch
    time and rate for both branches, and the registers of the existing tests (all jumps; one ordered pair, scaled by time; a
    reward vector, scaled by time)."""

    def __init__(self, name, regime, rel_rates, pi, tau, cat_rates=(1.0,), cat_weights=(1.0,), branch_rate=1.25, registers=3,
                 device_eigen=False, mpmath=False):
        self.name, self.regime, self.device_eigen, self.mpmath = name, regime, device_eigen, mpmath
        self.rel_rates, self.pi = np.asarray(rel_rates, dtype=np.float64), np.asarray(pi, dtype=np.float64)
        self.S = len(self.pi)
        self.cat_rates, self.cat_weights = np.asarray(cat_rates, dtype=np.float64), np.asarray(cat_weights, dtype=np.float64)
        self.branch_rate = float(branch_rate)
        self.time = float(tau) / self.branch_rate                  # tau names the branch length in substitutions at category rate 1
        S = self.S
        one = np.zeros((S, S)); one[0, S - 1] = 1.0
        reward = np.diag(np.random.default_rng(S).uniform(0.0, 2.0, S))
        every = np.ones((S, S)); np.fill_diagonal(every, 0.0)
        regs = [("all-jumps", every, "counts", False), ("single-pair", one, "counts", True), ("reward", reward, "rewards", True)]
        if registers == 2:
            regs = [regs[0], regs[2]]
        self.tags = [r[0] for r in regs]
        self.registers = [r[1] for r in regs]
        self.kinds = [r[2] for r in regs]
        self.scale_by_time = [r[3] for r in regs]

    def __repr__(self):
        return self.name

    def host_eigen(self):
        """The eigen system the host decomposes (numpy's symmetric solver on the pi-symmetrised matrix)."""
        return substmodel.decompose_reversible(substmodel.reversible_q(self.rel_rates, self.pi), self.pi)

    def times(self):
        return np.array([0.0, self.time, self.time])

    def rates(self):
        return np.array([1.0, self.branch_rate, self.branch_rate])

    def exact(self, U, Ui, lam):
        """-> (Cond [K][C][S][S], unit [K][C]) for the eigen system in use (cached per case for the host's)."""
        return exact_cond(U, Ui, lam, self.registers, self.kinds, self.scale_by_time, self.time, self.branch_rate, self.cat_rates)

    def restatement(self, U, Ui, lam, matrices=None, scale_by_time=None):
        """markov_jumps_reference.tables for the case's one branch -> [K][C][S][S].  ``matrices`` [C][S][S]: the branch's transition
        matrices (default: U (diag(e^(lambda tau)) U^-1) summed as the restatement sums)."""
        if matrices is None:
            tau = (self.time * self.branch_rate) * self.cat_rates
            matrices = mr.mm(U, np.exp(lam[None, :] * tau[:, None])[:, :, None] * Ui)
        mats = np.stack([np.zeros_like(matrices), matrices, matrices])
        sc = self.scale_by_time if scale_by_time is None else scale_by_time
        return mr.tables(U, Ui, lam, self.registers, self.kinds, sc, self.times(), self.rates(), self.cat_rates, mats)[:, 1]


@functools.lru_cache(maxsize=None)
def host_tables(case):
    """-> (U, Ui, lam, exact Cond, unit) of a case over the host's eigen system, computed once per process."""
    eig = case.host_eigen()
    return (eig.evec, eig.ievc, eig.evals) + case.exact(eig.evec, eig.ievc, eig.evals)


def hky_rates(kappa):
    return [1.0, kappa, 1.0, 1.0, kappa, 1.0]


@functools.lru_cache(maxsize=None)
def jump_cases():
    """Every Markov-jump case, by regime:
      well         GTR at 4 states (two categories of uneven rates and weights), random reversible models at 7, 20, 61 and 100 states
                   (100: two registers), tau in {0.05, 1, 30}.  The eigen formula loses a few tens of ulps of 1 in an entry of J or P
                   whatever its size, so Cond[i][j] loses that over P_ij: the random models here keep every P_ij near tau / S
      thin         the 61- and 100-state models of uneven frequencies at tau 0.05, where P_ij goes down to 5e-6 and the formula's
                   own loss reaches 1e-10: judged as the regimes below are
      tied         JC and F81 at 4 states, equal exchangeabilities with uneven frequencies at 20 and 61 states
      tied-device  the same four, over the eigen system the device decomposed (its basis inside the tied eigenspace is its own)
      near         HKY kappa = 1 + delta, pi = (.1, .2, .3, .4): eigenvalue gaps on either side of populateAuxInt's 1e-7
      short        GTR at 4 and 20 states, tau in {1e-3, 1e-6, 1e-8}
    The state counts run k_jumpMatrices4 (4), k_jumpMatrices (7, 20, 61) and k_jumpMatricesBig (100)."""
    pi4 = np.array([0.1, 0.2, 0.3, 0.4])
    gtr4 = [1.3, 4.1, 0.7, 1.1, 3.9, 1.0]
    out = []

    def random_model(S, even):
        """``even``: exchangeabilities within a factor 3 and frequencies within a few tens of per cent of each other, so that no
        P_ij is far below tau / S; otherwise substmodel.random_reversible's spread (P_ij down to 5e-6 at tau 0.05, 100 states)."""
        rng = np.random.default_rng(4000 + S)
        n = S * (S - 1) // 2
        if even:
            return rng.uniform(0.5, 1.5, size=n), rng.dirichlet(np.full(S, 50.0))
        return rng.gamma(shape=1.0, scale=1.0, size=n) + 0.05, rng.dirichlet(np.full(S, 5.0))

    for tau in (0.05, 1.0, 30.0):
        out.append(JumpCase("gtr4-t%g" % tau, "well", gtr4, pi4, tau, cat_rates=(0.5, 1.5), cat_weights=(0.4, 0.6), mpmath=True))
        for S in (7, 20, 61, 100):
            r, pi = random_model(S, even=True)
            out.append(JumpCase("rand%d-t%g" % (S, tau), "well", r, pi, tau, registers=2 if S == 100 else 3,
                                mpmath=S == 7 or (S == 20 and tau == 1.0)))
    for S in (61, 100):
        r, pi = random_model(S, even=False)
        out.append(JumpCase("uneven%d-t0.05" % S, "thin", r, pi, 0.05, registers=2 if S == 100 else 3))
    tied = [("jc", np.full(4, 0.25), (0.05, 1.0)), ("f81", pi4, (0.05, 1.0)),
            ("equal20", np.random.default_rng(20).dirichlet(np.full(20, 5.0)), (1.0,)),
            ("equal61", np.random.default_rng(61).dirichlet(np.full(61, 5.0)), (1.0,))]
    for name, pi, taus in tied:
        for tau in taus:
            out.append(JumpCase("%s-t%g" % (name, tau), "tied", *equal_rates(pi), tau, mpmath=len(pi) == 4))
    for name, pi, taus in tied:
        out.append(JumpCase("%s-device-t1" % name, "tied-device", *equal_rates(pi), 1.0, device_eigen=True))
    for delta in (8e-8, 2e-7, 1e-6, 1e-5):
        for tau in (1.0, 10.0):
            out.append(JumpCase("hky-d%g-t%g" % (delta, tau), "near", hky_rates(1.0 + delta), pi4, tau, mpmath=True))
    r20, pi20 = random_model(20, even=False)
    for tau in (1e-3, 1e-6, 1e-8):
        out.append(JumpCase("gtr4-t%g" % tau, "short", gtr4, pi4, tau, mpmath=True))
        out.append(JumpCase("rand20-t%g" % tau, "short", r20, pi20, tau))
    return tuple(out)


def host_jump_cases():
    """The cases whose eigen system the host decomposes (all but tied-device)."""
    return tuple(c for c in jump_cases() if not c.device_eigen)


# ---- the gather: patterns, coverage -----------------------------------------------------------------------------------------

def pair_probabilities(case, P):
    """[S tip-1 state i][S tip-2 state j][C][S root state]: the posterior of (category, root state) for a pattern with tips
    (i, j), from the frequencies, the branch's transition matrices ``P`` [C][S][S] and the category weights."""
    P = np.asarray(P, dtype=np.float64)
    joint = case.cat_weights[None, None, :, None] * case.pi[None, None, None, :] * \
        np.transpose(P, (2, 0, 1))[:, None, :, :] * np.transpose(P, (2, 0, 1))[None, :, :, :]
    return joint / joint.sum(axis=(2, 3), keepdims=True)


def expected_missing_share(case, P, R):
    """The expected share of a row's (category, parent state, state) table entries that none of the R S^2 patterns gathers.  Row 1
    gathers entry (c, s, i) from a pattern (i, j) that draws category c and root s; row 2 is its mirror image."""
    p = pair_probabilities(case, P)                                  # [i][j][c][s]
    with np.errstate(divide="ignore"):
        log_miss = R * np.log1p(-np.minimum(p, 1.0)).sum(axis=1)     # [i][c][s]: over tip-2 states j
    return float(np.exp(log_miss).mean())


def repeats(case, P, cap=400):
    """The smallest R whose R S^2 patterns cross a 256-pattern workgroup and leave an expected share of at most 0.1 % ungathered."""
    R = 256 // (case.S * case.S) + 1
    while expected_missing_share(case, P, R) > COVERAGE_EXPECTED and R < cap:
        R += 1
    return R


def exact_p(case, U, Ui, lam):
    """[C][S][S] float64: the branch's exact transition matrices."""
    zero = np.zeros((case.S, case.S))
    return np.stack([exact_tables(U, Ui, lam, zero, (case.time * case.branch_rate) * rc)[1] for rc in case.cat_rates]).astype(np.float64)


@functools.lru_cache(maxsize=None)
def host_repeats(case):
    U, Ui, lam = host_tables(case)[:3]
    return repeats(case, exact_p(case, U, Ui, lam))


def two_tip_workload(case, eig, R):
    """The case as a workload: tips 0 and 1 at height 0 under a root at height ``time``, patterns (i, j) for all S^2 ordered pairs,
    R times over."""
    S = case.S
    i, j = np.divmod(np.arange(S * S), S)
    tips = np.tile(np.stack([i, j]), (1, R)).astype(np.int32)
    tree = trees.Tree([-1, -1, 0], [-1, -1, 1], [0.0, 0.0, case.time], 2)
    return synth.Workload(case.name, tree, eig, case.pi, case.cat_rates, case.cat_weights, np.ascontiguousarray(tips),
                          np.ones(tips.shape[1]), S)


def gathered(table, states, cats):
    """[K][C][S][S] table of the one branch -> [K][2][P]: rows 1 and 2 of a two-tip draw (``states`` [3][P], row 0 the root)."""
    st = states.astype(np.int64)
    return np.stack([table[:, cats, st[0], st[r]] for r in (1, 2)], axis=1)


def drawn_missing_share(states, cats, S, C):
    """The larger, over the two rows, of the share of (category, parent state, state) entries no pattern gathered."""
    st = states.astype(np.int64)
    worst = 0.0
    for r in (1, 2):
        hit = np.unique((np.asarray(cats, dtype=np.int64) * S + st[0]) * S + st[r]).size
        worst = max(worst, 1.0 - hit / float(C * S * S))
    return worst


# ---- robust-count cases -----------------------------------------------------------------------------------------------------

class RobustCase:
    """Three position models, their site rates, a tree, and a regime per branch length."""

    def __init__(self, name, regime, models, tree, registers=3, mpmath=False):
        self.name, self.regime, self.models, self.tree, self.mpmath = name, regime, models, tree, mpmath
        self.register_count = registers

    def __repr__(self):
        return self.name

    def registers(self):
        return rcases.three_registers()[:self.register_count]

    def chain(self):
        eigs, _, rates = self.models
        return rr.product_chain(eigs, rates)

    def branch_lengths(self):
        """tau per tree node (the root: 0)."""
        t = self.tree
        return np.array([0.0 if t.parent[n] < 0 else t.height[t.parent[n]] - t.height[n] for n in range(t.node_count)])

    def row_regime(self, tau):
        return "short" if tau <= 1e-3 else self.regime

    def exact(self, taus, chain=None):
        """-> Cond [K][n][64][64] long double for rows of branch lengths ``taus`` (row 0 and zero lengths: 0; unit is max |R_k|
        off the diagonal, per register).  ``chain``: the (U, U^-1, lambda, Q) a call was handed (default: chain())."""
        U, Ui, lam, Q = self.chain() if chain is None else chain
        regs = self.registers()
        B = np.stack([exact_rate_registration(np.asarray(Q, dtype=LD), R, "counts") for R in regs])
        out = np.zeros((len(regs), len(taus), 64, 64), dtype=LD)
        for r, tau in enumerate(taus):
            if r > 0 and tau > 0.0:
                out[:, r] = _robust_exact(self, float(tau), U, Ui, lam, B)[0]
        return out

    def resolvable(self, taus, chain=None):
        """bool [n][64][64]: the entries whose transition probability float64 can tell from 0 at all.  The eigen sum P_ij = sum_a U_ia
        e^(lambda_a tau) U^-1_aj has, by the standard bound on a rounded dot product of n = 64 terms whose exp() is good to an ulp, an
        absolute error of at most (n + 2) ulp magP_ij, magP = |U| diag(e^(lambda tau)) |U^-1|.  Where the exact P_ij is at least
        twice that, any correctly rounded evaluation has P_ij > exact / 2 > 0 and Cond is finite; below it (three-substitution
        entries on a branch of 1e-6: P of order 1e-20) restatement and kernel divide by rounding noise or by 0, each by its own,
        and a comparison says nothing.  Rows of a hard-bounded regime must have no such entry (asserted by the tests)."""
        U, Ui, lam, Q = self.chain() if chain is None else chain
        out = np.ones((len(taus), 64, 64), dtype=bool)
        for r, tau in enumerate(taus):
            if r > 0 and tau > 0.0:
                P = _robust_exact(self, float(tau), U, Ui, lam, None)[1]
                mag = np.abs(U) @ (np.exp(lam * tau)[:, None] * np.abs(Ui))
                out[r] = P.astype(np.float64) >= 2.0 * 66.0 * np.finfo(np.float64).eps * mag
        return out

    def units(self):
        off = np.array(self.registers())
        off[:, np.arange(64), np.arange(64)] = 0.0
        return np.abs(off).max(axis=(1, 2))

    def restatement(self, taus):
        U, Ui, lam, Q = self.chain()
        return rr.tables(U, Ui, lam, Q, self.registers(), taus)[0]


_robust_cache = {}


def _robust_exact(case, tau, U, Ui, lam, B):
    """-> (Cond [K][64][64], P [64][64]) in long double; ``B`` None: P alone is wanted (Cond: None unless already there)."""
    key = (case.name, tau) + tuple(hash(np.ascontiguousarray(a).tobytes()) for a in (U, Ui, lam))
    if key not in _robust_cache or (B is not None and _robust_cache[key][0] is None):
        J, P = exact_tables(U, Ui, lam, np.zeros((1, 64, 64), dtype=LD) if B is None else B, tau)
        with np.errstate(divide="ignore", invalid="ignore"):
            _robust_cache[key] = (None if B is None else J / P, P)
    return _robust_cache[key]


@functools.lru_cache(maxsize=None)
def robust_cases():
    """The tied HKY kappa 2 chain of the golden file on its two-tip tree; a position_models chain on a two-tip tree with branches
    of 1.0 and 0.3; the near-tie chain on the same tree; the position_models chain on a 6-taxon caterpillar with one branch of
    1e-6 (judged as a short branch; its other rows as well conditioned)."""
    g = helpers.golden("robust_counting.json")["conditional_means"]
    eigs = [substmodel.hky(k, f) for k, f in zip(g["kappa"], g["frequencies_acgt"])]
    pis = [np.asarray(f) for f in g["frequencies_acgt"]]
    two = trees.Tree([-1, -1, 0], [-1, -1, 1], [0.0, 0.0, g["time"]], 2)
    uneven = trees.Tree([-1, -1, 0], [-1, -1, 1], [0.0, 0.7, 1.0], 2)
    cat = trees.caterpillar_tree(6, root_height=2.0)
    cat.height[7] = cat.height[8] - 1e-6                            # the second cherry's branch to its parent
    return (RobustCase("hky2-tied", "tied", (eigs, pis, [1.0, 1.0, 1.0]), two, registers=2, mpmath=False),
            RobustCase("position-models", "well", rcases.position_models(1), uneven),
            RobustCase("near-tie-chain", "near", rcases.near_tie_position_models(), uneven),
            RobustCase("short-branch", "well", rcases.position_models(3), cat))
