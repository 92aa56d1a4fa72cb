"""Host restatement of beagleMi355SampleMarkovJumps (include/beagle_mi355.h), from what an engine reads back.

It restates MarkovJumpsCore (src/dr/inference/markovjumps/MarkovJumpsCore.java: populateAuxInt :84-103, the joint forms :169-221
with and without PRECOMPUTE, the conditional forms :105-127), MarkovJumpsSubstitutionModel.setRegistration /
makeRateRegistrationMatrix / getMarginalRate, and MarkovJumpsBeagleTreeLikelihood.computeIntegratedMarkovJumpsForBranch
(src/dr/evomodel/treelikelihood/MarkovJumpsBeagleTreeLikelihood.java:510-567) with the per-pattern (:640-654) and per-row sums.

Every product is one IEEE double operation and every matrix product sums over its inner index in ascending order from 0.0 (``mm``),
as the kernels form them (kernels_markovjumps.hip): the two differ only where exp() does.  Arrays may carry leading batch axes.
"""
import numpy as np


def mm(A, B):
    """A @ B summed over the inner index in ascending order, one rounding per product and per sum (batch axes broadcast)."""
    out = np.zeros(np.broadcast_shapes(A.shape[:-1] + (B.shape[-1],), A.shape[:-2] + B.shape[-2:-1] + (B.shape[-1],)))
    for k in range(A.shape[-1]):
        out = out + A[..., :, k, None] * B[..., None, k, :]
    return out


def q_from_eigen(U, Ui, lam):
    """Q = U diag(lambda) U^-1 — the engine keeps no Q of its own."""
    return mm(U * lam[None, :], Ui)


def rate_registration(U, Ui, lam, R, kind):
    """rateReg: counts Q o R with R's diagonal 0; rewards diag(R[i][i])."""
    S = U.shape[0]
    R = np.asarray(R, dtype=np.float64).reshape(S, S)
    if kind == "rewards":
        return np.diag(np.diag(R))
    Rz = R.copy()
    np.fill_diagonal(Rz, 0.0)
    return q_from_eigen(U, Ui, lam) * Rz


def precompute(U, Ui, rate_reg):
    """M = U^-1 (rateReg U) (MarkovJumpsSubstitutionModel.makeRateRegistrationMatrix, PRECOMPUTE)."""
    return mm(Ui, mm(rate_reg, U))


def aux_int(lam, tau):
    """A[..., a, b] (Minin & Suchard eq. 37, populateAuxInt); tau may be an array of batch shape."""
    tau = np.asarray(tau, dtype=np.float64)[..., None, None]
    e = np.exp(lam[None, :] * tau)                                         # [..., 1, S]
    ea, eb = np.swapaxes(e, -1, -2), e
    la, lb = lam[:, None], lam[None, :]
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(np.abs(la - lb) < 1e-7, ea * tau, (ea - eb) / (la - lb))


def joint_precompute(U, Ui, lam, M, tau):
    """J = U ((A o M) U^-1) (computeJointStatMarkovJumpsPrecompute)."""
    return mm(U, mm(aux_int(lam, tau) * M, Ui))


def joint(U, Ui, lam, rate_reg, tau):
    """J = U ((A o (U^-1 (rateReg U))) U^-1) (computeJointStatMarkovJumps, no precomputation)."""
    return mm(U, mm(aux_int(lam, tau) * mm(Ui, mm(rate_reg, U)), Ui))


def marginal_rate(rate_reg, pi):
    """getMarginalRate: sum_i pi_i sum_j rateReg[i][j]."""
    return float(np.sum(np.asarray(pi)[:, None] * rate_reg))


def tables(U, Ui, lam, registers, kinds, scale_by_time, times, branch_rates, cat_rates, matrices):
    """Cond[k][r][c][S][S] for rows 1..n-1 (row 0: 0).  ``matrices`` [n][C][S][S]: row r's transition matrices as
    getTransitionMatrix returns them (row 0 ignored)."""
    n, C, S = len(times), len(cat_rates), U.shape[0]
    K = len(registers)
    times = np.asarray(times, dtype=np.float64)
    rates = np.ones(n) if branch_rates is None else np.asarray(branch_rates, dtype=np.float64)
    cat_rates = np.asarray(cat_rates, dtype=np.float64)
    out = np.zeros((K, n, C, S, S))
    tau = (times[1:] * rates[1:])[:, None] * cat_rates[None, :]           # [n-1, C]
    live = np.broadcast_to(cat_rates[None, :] > 0.0, tau.shape)
    P = np.asarray(matrices, dtype=np.float64)[1:]
    for k in range(K):
        M = precompute(U, Ui, rate_registration(U, Ui, lam, registers[k], kinds[k]))
        with np.errstate(divide="ignore", invalid="ignore"):
            V = joint_precompute(U, Ui, lam, M, tau) / P
            if scale_by_time[k]:
                V = V / (rates[1:, None] * cat_rates[None, :])[..., None, None]
        dead = np.zeros((n - 1, C, S, S))
        if kinds[k] == "rewards" and scale_by_time[k]:
            dead = dead + np.eye(S)[None, None] * times[1:, None, None, None]
        out[k, 1:] = np.where(live[..., None, None], V, dead)
    return out


def magnitudes(U, Ui, lam, registers, kinds, scale_by_time, times, branch_rates, cat_rates, matrices):
    """[K][n][C][S][S]: |U| ((|A| o |M_k|) |U^-1|) / P, with (e^(la t) + e^(lb t)) / |la - lb| for a difference entry of A — what
    an entry of ``tables`` is sensitive to when exp() is off by a few ulps (non-finite: 0; row 0: 0)."""
    n = len(times)
    times = np.asarray(times, dtype=np.float64)
    rates = np.ones(n) if branch_rates is None else np.asarray(branch_rates, dtype=np.float64)
    cat_rates = np.asarray(cat_rates, dtype=np.float64)
    tau = (times[1:] * rates[1:])[:, None] * cat_rates[None, :]
    e = np.exp(lam[None, None, :] * tau[..., None])[..., None, :]
    ea, eb = np.swapaxes(e, -1, -2), e
    d = np.abs(lam[:, None] - lam[None, :])
    with np.errstate(divide="ignore", invalid="ignore"):
        A = np.where(d < 1e-7, ea * tau[..., None, None], (ea + eb) / d)
    P = np.asarray(matrices, dtype=np.float64)
    out = np.zeros((len(registers),) + P.shape)
    for k, R in enumerate(registers):
        M = np.abs(precompute(U, Ui, rate_registration(U, Ui, lam, R, kinds[k])))
        with np.errstate(divide="ignore", invalid="ignore"):
            v = np.abs(U) @ ((A * M) @ np.abs(Ui)) / P[1:]
            if scale_by_time[k]:
                v = v / (rates[1:, None] * cat_rates[None, :])[..., None, None]
        out[k, 1:] = np.where(np.isfinite(v), v, 0.0)
    return out


def site_values(cond, states, parents, cats):
    """-> (values [K][n][P], pattern totals [K][P] summed over rows 1.. in row order, row totals [K][n] over patterns).
    ``states`` [n][P] (the draw's rows), ``parents`` [n] (row 0: -1), ``cats`` [P]."""
    K, n = cond.shape[:2]
    P = states.shape[1]
    st = states.astype(np.int64)
    cats = np.asarray(cats, dtype=np.int64)
    vals = np.zeros((K, n, P))
    for r in range(1, n):
        vals[:, r] = cond[:, r, cats, st[parents[r]], st[r]]
    tot = np.zeros((K, P))
    for r in range(1, n):
        tot = tot + vals[:, r]
    return vals, tot, vals.sum(axis=2)
