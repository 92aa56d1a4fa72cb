"""Substitution-parameter gradients (d lnL / d kappa, d lnL / d omega, d lnL / d rate_k ...) through the differential mass matrices of
the branches: the host side of the reference's BranchSubstitutionParameterDelegate.cacheDifferentialMassMatrix
(treedatalikelihood/discrete/BranchSubstitutionParameterDelegate.java:62-81; one model: HomogeneousSubstitutionParameterGradient,
ArbitrarySubstitutionGeneratorGradient) over the ``beagle.Beagle`` method set.

Per branch and rate category the delegate forms D with dP / d theta = P D
(substmodel/DifferentiableSubstitutionModelUtil.java:57-171 ``getExactDifferentialMassMatrix``), uploads it with a
``setDifferentialMatrix`` per branch and sums ``calculateEdgeDifferentials`` over the branches.  ``route="host"`` is that sequence,
with the numpy restatement below forming the matrices — the only route a library without the extension offers (the CPU oracle).
``route="device"`` forms every matrix on the device in one call (``Beagle.updateDifferentialMatrices``, include/beagle_mi355.h
beagleMi355UpdateDifferentialMatrices): D S^2 doubles cross the host link per gradient instead of a matrix per branch.

Eigen systems are taken as the engine takes them: row-major U and U^-1, eigenvalues [S], or [2 S] (real parts, imaginary parts) in the
real block form of an EIGEN_COMPLEX instance (inputs.substmodel.decompose_complex).
"""
import copy

import numpy as np

from . import beagle as _b
from .gradient import BranchGradient
from .inputs import substmodel

THRESHOLD = 1e-10
EXACT, FIRST_ORDER = 0, 1             # include/beagle_mi355.h BEAGLE_MI355_DIFFERENTIAL_*


def split_eigenvalues(evals, S):
    """-> (real parts [S], imaginary parts [S], indices of real eigenvalues, first indices of conjugate pairs), as
    getRealEigenValueIndices / getComplexEigenValueFirstIndices walk them."""
    ev = np.asarray(evals)
    re = ev[:S]
    im = ev[S:2 * S] if ev.shape[0] == 2 * S else np.zeros(S, dtype=ev.dtype)
    real, firsts, i = [], [], 0
    while i < S:
        if im[i] == 0:
            real.append(i); i += 1
        else:
            assert i + 1 < S and im[i + 1] == -im[i]
            firsts.append(i); i += 2
    return re, im, real, firsts


def _exp_cosine_integral(t, a, b):
    den = a * a + b * b
    e = np.exp(a * t)
    return (b * e * np.sin(b * t) + a * e * np.cos(b * t) - a) / den


def _exp_sine_integral(t, a, b):
    den = a * a + b * b
    e = np.exp(a * t)
    return (a * e * np.sin(b * t) - b * e * np.cos(b * t) + b) / den


def rotate(evec, ievc, dq, dtype=np.float64):
    """-> (V with small entries zeroed, V as computed): V = U^-1 (dQ U)."""
    U, Ui, Q = (np.asarray(x, dtype=dtype) for x in (evec, ievc, dq))
    raw = Ui @ (Q @ U)
    return np.where(np.abs(raw) < THRESHOLD, np.zeros_like(raw), raw), raw


def exact(evec, ievc, evals, dq, dist, dtype=np.float64):
    """-> (D, un-thresholded V) for one distance."""
    U, Ui = np.asarray(evec, dtype=dtype), np.asarray(ievc, dtype=dtype)
    S = U.shape[0]
    re, im, real, firsts = split_eigenvalues(np.asarray(evals, dtype=dtype), S)
    V, raw = rotate(U, Ui, dq, dtype)
    t = dtype(dist)
    W = V.copy()
    r = np.asarray(real, dtype=int)
    if len(r):
        li, lj = re[r][:, None], re[r][None, :]
        same = (np.abs(li - lj) < THRESHOLD) | np.eye(len(r), dtype=bool)
        gap = np.where(same, np.ones_like(li - lj), li - lj)
        v = V[np.ix_(r, r)]
        with np.errstate(over="ignore", invalid="ignore"):
            other = v * (1 - np.exp((lj - li) * t)) / gap
        W[np.ix_(r, r)] = np.where(same, v * t, np.where(v == 0, np.zeros_like(v), other))
    for i in real:
        for J in firsts:
            a, b = re[J] - re[i], im[J]
            c, s = _exp_cosine_integral(t, a, b), _exp_sine_integral(t, a, b)
            W[i, J], W[i, J + 1] = V[i, J] * c - V[i, J + 1] * s, V[i, J] * s + V[i, J + 1] * c
    for I in firsts:
        for j in real:
            a, b = re[j] - re[I], im[I]
            c, s = _exp_cosine_integral(t, a, b), _exp_sine_integral(t, a, b)
            W[I, j], W[I + 1, j] = V[I, j] * c - V[I + 1, j] * s, V[I, j] * s + V[I + 1, j] * c
        for J in firsts:
            aI, bI, aJ, bJ = re[I], im[I], re[J], im[J]
            vij, vijp1, vip1j, vip1jp1 = V[I, J], V[I, J + 1], V[I + 1, J], V[I + 1, J + 1]
            if abs(aI - aJ) < THRESHOLD and abs(bI - bJ) < THRESHOLD:
                c_plus, c_minus = np.sin(2 * bI * t) / 2 / bI, t
                s_plus, s_minus = (1 - np.cos(2 * bI * t)) / 2 / bI, dtype(0)
            else:
                c_plus, c_minus = _exp_cosine_integral(t, aJ - aI, bI + bJ), _exp_cosine_integral(t, aJ - aI, bI - bJ)
                s_plus, s_minus = _exp_sine_integral(t, aJ - aI, bI + bJ), _exp_sine_integral(t, aJ - aI, bI - bJ)
            half = dtype(0.5)
            W[I, J] = half * ((vij - vip1jp1) * c_plus + (vij + vip1jp1) * c_minus - (vip1j + vijp1) * s_plus + (vijp1 - vip1j) * s_minus)
            W[I, J + 1] = half * ((vijp1 + vip1j) * c_plus + (vijp1 - vip1j) * c_minus + (vij - vip1jp1) * s_plus - (vij + vip1jp1) * s_minus)
            W[I + 1, J] = half * ((vijp1 + vip1j) * c_plus + (vip1j - vijp1) * c_minus + (vij - vip1jp1) * s_plus + (vij + vip1jp1) * s_minus)
            W[I + 1, J + 1] = half * ((vip1jp1 - vij) * c_plus + (vij + vip1jp1) * c_minus + (vip1j + vijp1) * s_plus + (vijp1 - vip1j) * s_minus)
    return U @ (W @ Ui), raw


def first_order(dq, dist, dtype=np.float64):
    return dtype(dist) * np.asarray(dq, dtype=dtype)


# ---- models with an analytic dQ / d theta ---------------------------------------------------------------------------------
class ParameterModel:
    """A substitution model as a gradient sees it: its eigen system, its frequencies, and dQ / d theta of the NORMALISED generator for
    every parameter, [parameters][S][S].  The unnormalised generator of the models below is affine in the parameter, so its
    derivative, the normalisation term included, is exact: Q = Q~ / n with n = -sum_i pi_i Q~_ii gives
    dQ = (dQ~ - Q n') / n,  n' = -sum_i (pi'_i Q~_ii + pi_i dQ~_ii)."""

    def __init__(self, eig, freqs, dq):
        self.eig, self.freqs = eig, np.asarray(freqs, dtype=np.float64)
        self.dq = np.ascontiguousarray(dq, dtype=np.float64).reshape(-1, self.eig.evec.shape[0], self.eig.evec.shape[0])


def _normalised_derivative(q, dq, pi, dpi=None):
    n = substmodel.normalization(q, pi)
    dn = -float((np.diag(dq) * pi).sum()) - (0.0 if dpi is None else float((np.diag(q) * dpi).sum()))
    return (dq - (q / n) * dn) / n


def hky_kappa(kappa, pi):
    """HKY with theta = kappa (HKY.java:157-230: kappa on AG and CT)."""
    pi = np.asarray(pi, dtype=np.float64)
    q = substmodel.reversible_q([1.0, kappa, 1.0, 1.0, kappa, 1.0], pi)
    dq = substmodel.reversible_q([0.0, 1.0, 0.0, 0.0, 1.0, 0.0], pi)
    return ParameterModel(substmodel.hky(kappa, pi), pi, _normalised_derivative(q, dq, pi))


def reversible_rate(rates_upper, pi, which):
    """A general reversible model (inputs.substmodel.reversible_q) with theta = rates_upper[which], one parameter per entry of ``which``."""
    rates, pi = np.asarray(rates_upper, dtype=np.float64), np.asarray(pi, dtype=np.float64)
    q = substmodel.reversible_q(rates, pi)
    out = []
    for k in np.atleast_1d(which):
        unit = np.zeros_like(rates)
        unit[k] = 1.0
        out.append(_normalised_derivative(q, substmodel.reversible_q(unit, pi), pi))
    return ParameterModel(substmodel.decompose_reversible(q, pi), pi, np.stack(out))


def gy94_omega(kappa, omega, codon_pi=None):
    """GY94 over the 61 sense codons with theta = omega (GY94CodonModel.java:165-188: omega on the non-synonymous rates)."""
    pi = np.full(61, 1.0 / 61) if codon_pi is None else np.asarray(codon_pi, dtype=np.float64)
    q = substmodel.reversible_q(substmodel.gy94_rates(kappa, omega), pi)
    dq = substmodel.reversible_q(np.asarray(substmodel.gy94_rates(kappa, 1.0)) - np.asarray(substmodel.gy94_rates(kappa, 0.0)), pi)
    return ParameterModel(substmodel.gy94(kappa, omega, pi)[0], pi, _normalised_derivative(q, dq, pi))


def complex_rate(rates, state_count, which):
    """ComplexSubstitutionModel (inputs.substmodel.complex_q) with theta = rates[which], one parameter per entry of ``which``.  The
    model is normalised at its own stationary distribution, which moves with the rate: pi' solves pi' Q~ = -pi dQ~, sum pi' = 0."""
    rates = np.asarray(rates, dtype=np.float64)
    q = substmodel.complex_q(rates, state_count)
    pi, eig = substmodel.decompose_complex(q)
    a = np.vstack([q.T, np.ones(state_count)])
    out = []
    for k in np.atleast_1d(which):
        unit = np.zeros_like(rates)
        unit[k] = 1.0
        dq = substmodel.complex_q(unit, state_count)
        dpi = np.linalg.lstsq(a, np.concatenate([-(pi @ dq), [0.0]]), rcond=None)[0]
        out.append(_normalised_derivative(q, dq, pi, dpi))
    return ParameterModel(eig, pi, np.stack(out))


# ---- the gradient ---------------------------------------------------------------------------------------------------------
class SubstitutionParameterGradient(BranchGradient):
    """d lnL / d theta for every parameter of every model: BranchGradient's post- and pre-order passes over a list of models and a
    per-branch model index (the reference's branch-specific case; one model is the homogeneous one), then per parameter the branches'
    differential matrices in the slots behind the branch matrices and ONE calculateEdgeDifferentials over all branches.

    models: ParameterModel list, all with as many parameters; branch_model: [node_count] model index of the branch above each node
    (None: model 0 everywhere); the root's frequencies are the workload's.  gradient() -> (lnL, gradient[model, parameter]): the
    sum over the branches that evolve under the model."""

    def __init__(self, workload, models, branch_model=None, route="device", mode=EXACT, library=None, resource_list=(1,),
                 rescale=False):
        if route not in ("device", "host"):
            raise ValueError("route is 'device' or 'host'")
        self.models, self.route, self.mode = list(models), route, mode
        complex_eigen = self.models[0].eig.evals.shape[0] == 2 * workload.state_count
        workload = copy.copy(workload)
        workload.eig = self.models[0].eig                    # (eigen system 0 as BranchGradient sets it; the data stay the workload's)
        super().__init__(workload, library=library, rescale=rescale, resource_list=resource_list,
                         extra_matrices=workload.tree.node_count, eigen_count=len(self.models),
                         requirement_flags=_b.FLAG_EIGEN_COMPLEX if complex_eigen else 0)
        if route == "device" and not hasattr(self.b.lib.lib, "beagleMi355UpdateDifferentialMatrices"):
            raise ValueError("this library forms no differential matrices: route='host'")
        for k, m in enumerate(self.models):
            self.b.setEigenDecomposition(k, m.eig.evec, m.eig.ievc, m.eig.evals)
        self.parameter_count = self.models[0].dq.shape[0]
        self.branch_model = np.zeros(self.N, dtype=np.int32) if branch_model is None else np.asarray(branch_model, dtype=np.int32)
        self._edge_model = self.branch_model[self._nodes]
        self._edge_rate_set = np.zeros(len(self._nodes), dtype=np.int32)
        self._d_idx = (self.extra_index + self._nodes).astype(np.int32)         # the differential slot of the branch above node n

    def set_model(self, k, model):
        """Model k with new parameter values (its eigen system goes to the instance)."""
        self.models[k] = model
        self.b.setEigenDecomposition(k, model.eig.evec, model.eig.ievc, model.eig.evals)

    def log_likelihood(self):
        idx = self._nodes
        self.b.updateTransitionMatricesWithMultipleModels(self._edge_model, self._edge_rate_set, self._edge_matrix[self._set], None,
                                                          None, self.branch_lengths[idx], len(idx))
        self.b.updatePartials(self._post_ops, len(self._post_ops) // 7, _b.NONE)
        if self.rescale:
            self.b.resetScaleFactors(self.cum_scale)
            scales = self._scale_indices_by_set[self._set]
            self.b.accumulateScaleFactors(scales, len(scales), self.cum_scale)
        out = [0.0]
        self.b.calculateRootLogLikelihoods([self.post_index(self.tree.root)], [0], [0], [self.cum_scale], 1, out)
        return out[0]

    def host_matrices(self, parameter):
        """The branches' differential matrices as the host route forms them: [edges][C][S][S]."""
        rates = np.asarray(self.wl.cat_rates, dtype=np.float64)
        out = np.empty((len(self._nodes), self.C, self.S, self.S))
        for e, n in enumerate(self._nodes):
            m = self.models[self._edge_model[e]]
            for c, r in enumerate(rates):
                dist = self.branch_lengths[n] * r
                out[e, c] = exact(m.eig.evec, m.eig.ievc, m.eig.evals, m.dq[parameter], dist)[0] if self.mode == EXACT \
                    else first_order(m.dq[parameter], dist)
        return out

    def set_differential_matrices(self, parameter):
        """Every branch's differential matrix for one parameter into its slot, by the instance's route."""
        if self.route == "host":
            for slot, m in zip(self._d_idx, self.host_matrices(parameter)):
                self.b.setDifferentialMatrix(int(slot), m)
            return
        dq = np.stack([m.dq[parameter] for m in self.models])
        self.b.updateDifferentialMatrices(self._edge_model, self._edge_rate_set, dq, self._edge_model, self._d_idx,
                                          self.branch_lengths[self._nodes], len(self._nodes), self.mode)

    def gradient(self):
        lnl = self.log_likelihood()
        self.b.setPartials(self.pre_offset + self.tree.root, self._root_pre)
        self.b.updatePrePartials(self._pre_ops, len(self._pre_ops) // 7, _b.NONE)
        post, pre, n = self._edge_post[self._set], self._pre_idx, len(self._nodes)
        grad = np.zeros((len(self.models), self.parameter_count))
        for p in range(self.parameter_count):
            self.set_differential_matrices(p)
            per_branch, _, _ = self.b.calculateEdgeDifferentials(post, pre, self._d_idx, self._w0, n, want_squared=False)
            np.add.at(grad[:, p], self._edge_model, per_branch)
        return lnl, grad
