"""The restatement of the device's reversible-model decomposition (include/beagle_mi355.h beagleMi355SetReversibleModels;
csrc/kernels_eigen.hip) that its tests compare with, the yardstick both are measured against, and the test inputs.

The restatement is the kernel's iteration in numpy, in a dtype of the caller's choice: A = Pi^1/2 Q Pi^-1/2 formed symmetric from the
relative rates, cyclic Jacobi in the round-robin tournament order (n - 1 rounds of n / 2 disjoint pairs per sweep, n = S rounded up
to even with an idle player), the angle in its stable form, every 2 x 2 block of a round rotated by its row pair first and its
column pair second and mirrored from the upper block triangle, the stopping test off(A) <= eps ||A||_F at the top of each sweep, the
cap of 30 sweeps, eigenvalues ascending (ties by index).  It is not bit for bit the kernel (the device contracts multiply-adds and
sums the norms in another order).

The yardstick is P(t) = exp(Q t / n) by scaling and squaring with a Taylor series in np.longdouble: no eigensolver takes part in it.
"""
import numpy as np

from beast_mcmc_amd.inputs import substmodel

CAP = 30


def tournament(n):
    """The n - 1 rounds of the round-robin order for n (even) players: per round (p[n / 2], q[n / 2]), p < q.  Player n - 1 stays;
    pair 0 of round r is (r, n - 1)."""
    rounds = []
    for r in range(n - 1):
        a = np.array([(r + k) % (n - 1) for k in range(n // 2)])
        b = np.array([n - 1] + [(r - k) % (n - 1) for k in range(1, n // 2)])
        rounds.append((np.minimum(a, b), np.maximum(a, b)))
    return rounds


def generator(rates, pi, dtype=np.float64):
    """-> (Q unnormalised [S][S], n): Q_ij = r_ij pi_j, rows summing to zero (the diagonal is minus the sum over j ascending)."""
    r, pi = np.asarray(rates, dtype=dtype), np.asarray(pi, dtype=dtype)
    S = pi.shape[0]
    R = np.zeros((S, S), dtype=dtype)
    iu = np.triu_indices(S, 1)
    R[iu] = r
    R = R + R.T
    Q = R * pi[None, :]
    diag = np.zeros(S, dtype=dtype)
    for j in range(S):
        diag = diag - Q[:, j]
    Q[np.arange(S), np.arange(S)] = diag
    n = dtype(0)
    for i in range(S):
        n = n - pi[i] * diag[i]
    return Q, n


def symmetrised(rates, pi, dtype=np.float64):
    """-> (A [S][S], sqrt(pi), n): A_ij = (sqrt(pi_i) r_ij) sqrt(pi_j) for i < j, mirrored; A_ii = Q_ii."""
    r, pi = np.asarray(rates, dtype=dtype), np.asarray(pi, dtype=dtype)
    S = pi.shape[0]
    Q, n = generator(rates, pi, dtype)
    sq = np.sqrt(pi)
    A = np.zeros((S, S), dtype=dtype)
    iu = np.triu_indices(S, 1)
    A[iu] = (sq[iu[0]] * r) * sq[iu[1]]
    A = A + A.T
    A[np.arange(S), np.arange(S)] = np.diag(Q)
    return A, sq, n


def jacobi(A, dtype=np.float64):
    """-> (mu [S], V [S][S], sweeps, capped): A = V diag(mu) V^T by the kernel's iteration."""
    A = np.asarray(A, dtype=dtype)
    S = A.shape[0]
    n = S + (S & 1)
    M = np.zeros((n, n), dtype=dtype)
    M[:S, :S] = A
    V = np.eye(n, dtype=dtype)
    eps = dtype(np.finfo(np.float64).eps) if dtype == np.float64 else np.finfo(dtype).eps
    norm2 = np.sum(M * M)
    rounds = tournament(n)
    pair_of = []
    for p, q in rounds:
        po = np.empty(n, dtype=int)
        po[p] = np.arange(n // 2); po[q] = np.arange(n // 2)
        pair_of.append(po[:, None] <= po[None, :])          # the upper block triangle of the round
    one, zero, two = dtype(1), dtype(0), dtype(2)
    sweeps, capped = 0, False
    while True:
        off2 = two * np.sum(np.triu(M, 1) ** 2)
        if off2 <= eps * eps * norm2:
            break
        if sweeps == CAP:
            capped = True
            break
        for (p, q), upper in zip(rounds, pair_of):
            app, aqq, apq = M[p, p], M[q, q], M[p, q]
            live = apq != 0
            safe = np.where(live, apq, one)
            theta = (aqq - app) / (two * safe)
            big = np.abs(theta) > dtype(1e150)
            th = np.where(big, one, theta)
            t = np.where(theta < 0, -one, one) / (np.abs(th) + np.sqrt(th * th + one))
            with np.errstate(divide="ignore"):
                t = np.where(big, one / (two * theta), t)
            t = np.where(live, t, zero)
            c = one / np.sqrt(t * t + one)
            s = t * c
            # rows by their pair, then columns by theirs
            G = M.copy()
            rp, rq = M[p, :], M[q, :]
            G[p, :] = c[:, None] * rp - s[:, None] * rq
            G[q, :] = s[:, None] * rp + c[:, None] * rq
            cp, cq = G[:, p].copy(), G[:, q].copy()
            G[:, p] = cp * c[None, :] - cq * s[None, :]
            G[:, q] = cp * s[None, :] + cq * c[None, :]
            M = np.where(upper, G, G.T)
            M[p, p] = app - t * apq
            M[q, q] = aqq + t * apq
            M[p, q] = zero
            M[q, p] = zero
            vp, vq = V[:, p].copy(), V[:, q].copy()
            V[:, p] = vp * c[None, :] - vq * s[None, :]
            V[:, q] = vp * s[None, :] + vq * c[None, :]
        sweeps += 1
    return np.diag(M)[:S].copy(), V[:S, :S].copy(), sweeps, capped


class Decomposition:
    def __init__(self, evec, ievc, evals, sweeps, capped):
        self.evec, self.ievc, self.evals, self.sweeps, self.capped = evec, ievc, evals, sweeps, capped


def decompose(rates, pi, dtype=np.float64):
    """What the device call leaves in a slot: U = Pi^-1/2 V, U^-1 = V^T Pi^1/2, lambda = mu / n, eigenvalues ascending."""
    A, sq, n = symmetrised(rates, pi, dtype)
    mu, V, sweeps, capped = jacobi(A, dtype)
    order = np.argsort(mu, kind="stable")
    mu, V = mu[order], V[:, order]
    lam = mu / n
    if capped:
        lam = np.full_like(lam, np.nan)
    return Decomposition(V / sq[:, None], V.T * sq[None, :], lam, sweeps, capped)


def transition_probabilities(d, dist, dtype=np.float64):
    U, Ui, lam = (np.asarray(x, dtype=dtype) for x in (d.evec, d.ievc, d.evals))
    return (U * np.exp(lam * dtype(dist))[None, :]) @ Ui


def yardstick_p(rates, pi, dist):
    """exp(Q dist / n) in np.longdouble: scaling and squaring with a Taylor series (the matmul works on that dtype)."""
    ld = np.longdouble
    Q, n = generator(rates, pi, ld)
    M = Q * (ld(dist) / n)
    S = M.shape[0]
    norm = float(np.max(np.sum(np.abs(M), axis=1)))
    squarings = 0 if norm <= 0.5 else int(np.ceil(np.log2(norm))) + 1
    M = M / ld(2) ** squarings
    P = np.eye(S, dtype=ld)
    term = np.eye(S, dtype=ld)
    for k in range(1, 40):
        term = (term @ M) / ld(k)
        P = P + term
        if float(np.max(np.abs(term))) < 1e-24:
            break
    for _ in range(squarings):
        P = P @ P
    return P


# ---- the test inputs -------------------------------------------------------------------------------------------------------
STATES = [2, 3, 4, 5, 7, 8, 9, 16, 20, 61, 64]
BOUNDARY_STATES = [22, 23, 44, 45]          # the last and first state counts of the workgroup kernel's three register sizes (22, 44, 64 players)
LENGTHS = np.array([0.0, 1e-3, 0.11, 0.9, 25.0])
CATEGORY_RATES = np.array([0.05, 0.4, 1.1, 2.45])


def random_model(S, rng):
    """As inputs.substmodel.random_reversible draws them: (rates [S (S - 1) / 2], pi [S])."""
    return rng.gamma(shape=1.0, scale=1.0, size=S * (S - 1) // 2) + 0.05, rng.dirichlet(np.full(S, 5.0))


def jc69(S):
    return np.ones(S * (S - 1) // 2), np.full(S, 1.0 / S)


def gy94_flat():
    return np.asarray(substmodel.gy94_rates(2.0, 0.2), dtype=np.float64), np.full(61, 1.0 / 61)


def reducible6():
    """Three disconnected pairs: 0-1, 2-3, 4-5."""
    r = np.zeros(15)
    iu = np.triu_indices(6, 1)
    for k, (i, j) in enumerate(zip(*iu)):
        if (i, j) in ((0, 1), (2, 3), (4, 5)):
            r[k] = 1.0 + 0.5 * i
    return r, np.array([0.1, 0.2, 0.15, 0.25, 0.05, 0.25])


def models_at(S):
    """-> [(name, rates, pi)]: three random reversible models and the special ones of this state count."""
    rng = np.random.default_rng(100 + S)
    out = [("random%d" % k,) + random_model(S, rng) for k in range(3)]
    out.append(("jc69",) + jc69(S))
    if S == 61:
        out.append(("gy94-flat",) + gy94_flat())
    if S == 20:
        r, pi = random_model(20, rng)
        out.append(("rates-1e-8..1e8", 10.0 ** rng.uniform(-8, 8, size=190), pi))
        tiny = pi.copy()
        tiny[3] = 1e-12
        out.append(("frequency-1e-12", r, tiny / tiny.sum()))
    return out


def accuracy_models():
    """Every (S, name, rates, pi) of the accuracy test, the reducible 6-state model included."""
    out = [(S,) + m for S in STATES + BOUNDARY_STATES for m in models_at(S)]
    out.append((6, "reducible") + reducible6())
    return out


def residuals(d, rates, pi):
    """-> (max |U U^-1 - I|, max |U diag(lambda) U^-1 - Q / n| / max |Q / n|) of a decomposition, measured in longdouble."""
    ld = np.longdouble
    U, Ui, lam = (np.asarray(x, dtype=ld) for x in (d.evec, d.ievc, d.evals))
    Q, n = generator(rates, pi, ld)
    Qn = Q / n
    ident = float(np.max(np.abs(U @ Ui - np.eye(U.shape[0], dtype=ld))))
    recon = float(np.max(np.abs((U * lam[None, :]) @ Ui - Qn)) / np.max(np.abs(Qn)))
    return ident, recon


# ---- a branch-specific evaluation: one model per branch ----------------------------------------------------------------------
def branch_model_plan(kind, library, route, seed=51, taxa=8, patterns=64):
    """A tree of `taxa` tips (8) with `patterns` patterns (64) and 4 categories whose every branch has its own model — HKY kappa at 4
    states ("hky"), a random reversible model at 20 ("reversible20"), GY94 omega at 61 ("gy94") — as (workload, model set, evaluation):
    BranchGradient's buffer plan and post-order list over an instance with the set's double-buffered eigen systems."""
    import helpers
    from beast_mcmc_amd import beagle as _b, eigensystems
    from beast_mcmc_amd.gradient import BranchGradient

    S = {"hky": 4, "reversible20": 20, "gy94": 61}[kind]
    wl = helpers.random_workload(taxa, patterns, S, 4, seed=seed)
    edges = wl.tree.node_count - 1
    rng = np.random.default_rng(seed)
    models = eigensystems.SubstitutionModelSet(S, edges, route=route, library=library)
    if kind == "hky":
        models.set_hky(rng.gamma(4.0, 0.6, size=edges) + 0.2, wl.freqs)
    elif kind == "gy94":
        models.set_gy94(2.0, rng.gamma(2.0, 0.2, size=edges) + 0.02, wl.freqs)
    else:
        for k in range(edges):
            models.set_model(k, rng.gamma(1.0, 1.0, size=190) + 0.05, wl.freqs)

    class Evaluation(BranchGradient):
        def log_likelihood(self):
            models.update(self.b)
            idx = self._nodes
            self.b.updateTransitionMatricesWithMultipleModels(models.eigen_indices(), np.zeros(len(idx), dtype=np.int32),
                                                              self._edge_matrix[self._set], None, None, self.branch_lengths[idx], len(idx))
            self.b.updatePartials(self._post_ops, len(self._post_ops) // 7, _b.NONE)
            out = [0.0]
            self.b.calculateRootLogLikelihoods([self.post_index(self.tree.root)], [0], [0], [_b.NONE], 1, out)
            return out[0]

    return wl, models, Evaluation(wl, library=library, eigen_count=models.eigen_buffer_count)
