"""The stochastic Dollo (ALS) tree likelihood: the caller-side mirror of ``dr.oldevomodel.MSSD.ALSTreeLikelihood`` with its
``anyTip`` / ``singleTip`` observation processes (src/dr/oldevomodel/MSSD/ALSTreeLikelihood.java:87-95,
AbstractObservationProcess.java:174-229, AnyTipObservationProcess.java:57-168, SingleTipObservationProcess.java:57-59) — the
likelihood whose BEAGLE form, ``ALSBeagleTreeLikelihood.calculateLogLikelihood``, throws "Not implemented for BEAGLE".

The reference reads a ``getPartials`` per node and a ``getLogScaleFactors`` per internal node after the pruning pass and loops over
nodes x patterns x states on the host.  Here that loop is ONE engine call (include/beagle_mi355.h
``beagleMi355NodePatternLikelihoods``); ``route="readback"`` keeps the reference's shape — read everything back, loop in numpy — for
the benchmark and the tests.  Either way the likelihood is finished on the host exactly as the reference finishes it: ascertainment
correction, ``gammaNorm``, ``logN``, ``calculateLogTreeWeight`` and the two ``integrateGainRate`` branches.

This class borrows a ``treelikelihood.BeagleTreeLikelihood``'s instance, tree, tips and buffer numbering and runs its own pruning
pass on it: the branch matrices are those of ``MutationDeathModel.getTransitionProbabilities`` (a base model scaled by
2 * mutationRate * prod(freqs[:-1]), every state dying at rate delta into an absorbing last state) and come from their generator in
one call (``beagleMi355UpdateTransitionMatricesFromGenerators``); on a library without that call (the CPU oracle) they are formed
on the host and set one by one.
"""
import math

import numpy as np

from . import beagle as _b
from .generators import SYMBOL as _GENERATOR_SYMBOL

ANY_TIP, SINGLE_TIP = "anyTip", "singleTip"
NODE_PATTERN_SYMBOL = "beagleMi355NodePatternLikelihoods"


def mutation_death_generator(base_generator, freqs, mutation_rate, death_rate):
    """[S][S]: the generator whose exp(Q d) is MutationDeathModel.getTransitionProbabilities(d) (MutationDeathModel.java:140-168):
    the base model's [S-1][S-1] generator (None: one live state) times 2 * mutationRate * prod(freqs[:-1]), -delta on the diagonal,
    delta into the death column, a zero last row."""
    freqs = np.asarray(freqs, dtype=np.float64)
    S = freqs.size
    scale = 2.0 * mutation_rate
    for f in freqs[:-1]:
        scale *= f
    Q = np.zeros((S, S))
    if base_generator is not None:
        Q[:S - 1, :S - 1] = scale * np.asarray(base_generator, dtype=np.float64).reshape(S - 1, S - 1)
    for i in range(S - 1):
        Q[i, i] -= death_rate
        Q[i, S - 1] = death_rate
    return Q


def host_transition_matrix(Q, d):
    """exp(Q d) on the host by scaling and squaring over a 20-term series (libraries without the generator call)."""
    A = np.asarray(Q, dtype=np.float64) * d
    norm = np.abs(A).sum(axis=1).max()
    s = 0 if norm <= 0.5 else max(0, int(math.ceil(math.log2(norm / 0.5))))
    A = A / (2.0 ** s)
    T, term = np.eye(A.shape[0]), np.eye(A.shape[0])
    for k in range(1, 21):
        term = term @ A / k
        T = T + term
    for _ in range(s):
        T = T @ T
    return T


class ALSTreeLikelihood:
    """``alsTreeLikelihood`` over a ``treelikelihood.BeagleTreeLikelihood`` (which supplies the instance, the tree and the tips; its
    own substitution model is never used).

    ``freqs`` [S] with the death state last; ``base_generator`` [S-1][S-1] or None; ``death_rate`` is the model's delta and ``mu`` the
    observation process's death rate (the reference's XML names the same parameter for both; default: ``death_rate``); ``lam`` the
    birth rate.  ``observation``: "anyTip" or "singleTip".  ``rescale``: every internal node is rescaled (ALWAYS) and its log
    factors kept per node.  ``include`` / ``exclude``: AscertainedSitePatterns' pattern lists."""

    def __init__(self, tree_likelihood, tip_states, pattern_weights, freqs, death_rate, lam, base_generator=None, mutation_rate=1.0, mu=None,
                 observation=ANY_TIP, integrate_gain_rate=False, include=(), exclude=(), branch_rates=None, rescale=False,
                 death_state=None, route="device"):
        self.tl = tree_likelihood
        self.tree = tree_likelihood.tree
        self.beagle = _b.Beagle.attach(tree_likelihood)
        self.S, self.P, self.C = tree_likelihood.state_count, tree_likelihood.pattern_count, tree_likelihood.category_count
        self.freqs = np.asarray(freqs, dtype=np.float64)
        self.base_generator, self.mutation_rate = base_generator, float(mutation_rate)
        self.death_rate, self.lam = float(death_rate), float(lam)
        self.mu = self.death_rate if mu is None else float(mu)
        if observation not in (ANY_TIP, SINGLE_TIP):
            raise ValueError("observation: anyTip or singleTip")
        self.observation, self.integrate_gain_rate = observation, bool(integrate_gain_rate)
        self.include, self.exclude = [int(i) for i in include], [int(i) for i in exclude]
        self.branch_rates = np.ones(self.tree.node_count) if branch_rates is None else np.asarray(branch_rates, dtype=np.float64)
        self.rescale = bool(rescale)
        self.death_state = self.S - 1 if death_state is None else int(death_state)
        self.route = route
        self.tip_states = np.asarray(tip_states)             # [T][P] codes as the instance was given them
        self.pattern_weights = np.asarray(pattern_weights, dtype=np.float64)
        self.tip_partials = {}                               # tip -> [P][S]: tips held as partials (useAmbiguities)
        self.last = {}

    @classmethod
    def create(cls, tree, tip_states, pattern_weights, freqs, cat_rates, cat_weights, library=None, resource_list=(1,), **model):
        """A BeagleTreeLikelihood made for this likelihood (its eigen system is a placeholder: the matrices come from the generator)
        and the ALSTreeLikelihood over it; ``model``: the constructor's keywords."""
        from types import SimpleNamespace
        from .treelikelihood import RESCALE_NONE, BeagleTreeLikelihood
        S = len(freqs)
        eig = SimpleNamespace(evec=np.eye(S), ievc=np.eye(S), evals=np.zeros(S))
        tl = BeagleTreeLikelihood(tree=tree, tip_states=tip_states, weights=pattern_weights, eig=eig, freqs=freqs, cat_rates=cat_rates,
                                  cat_weights=cat_weights, state_count=S, rescaling=RESCALE_NONE, library=library,
                                  resource_list=resource_list)
        return cls(tl, tip_states, pattern_weights, freqs, **model)

    def close(self):
        self.tl.close()

    # ---- inputs -------------------------------------------------------------------------------------------------------------
    def set_tip_partials(self, tip, partials):
        """Tip ``tip`` as partials [P][S] instead of compact states (the route ALSTreeLikelihood takes: useAmbiguities)."""
        part = np.ascontiguousarray(partials, dtype=np.float64).reshape(self.P, self.S)
        self.beagle.setTipPartials(tip, part)
        self.tip_partials[int(tip)] = part

    def average_rate(self):
        """AbstractObservationProcess.getAverageRate: sum of proportion x rate over the categories, upwards."""
        avg = 0.0
        for w, r in zip(self.tl.cat_weights, self.tl.cat_rates):
            avg += w * r
        return avg

    def branch_time(self, node):
        """Operational time of the branch above ``node``: branch rate x length."""
        return self.branch_rates[node] * (self.tree.height[self.tree.parent[node]] - self.tree.height[node])

    def node_survival_probability(self, node):
        """AbstractObservationProcess.getNodeSurvivalProbability: 1 - exp(-mu avgRate rate_i t_i), 1 at the root."""
        if self.tree.parent[node] < 0:
            return 1.0
        return 1.0 - math.exp(-(self.mu * self.average_rate()) * self.branch_time(node))

    # ---- the pruning pass ---------------------------------------------------------------------------------------------------
    def generator(self):
        return mutation_death_generator(self.base_generator, self.freqs, self.mutation_rate, self.death_rate)

    def scale_index(self, node):
        return node - self.tree.tip_count if self.rescale and node >= self.tree.tip_count else _b.NONE

    def update_matrices(self):
        tree, tl = self.tree, self.tl
        nodes = [n for n in range(tree.node_count) if tree.parent[n] >= 0]
        slots = [tl.node_matrix_index(n) for n in nodes]
        lengths = [self.branch_time(n) for n in nodes]
        Q = self.generator()
        if hasattr(self.beagle.lib.lib, _GENERATOR_SYMBOL):
            self.beagle.updateTransitionMatricesFromGenerators(Q[None], None, None, slots, lengths)
        else:
            for slot, d in zip(slots, lengths):
                self.beagle.setTransitionMatrix(slot, np.stack([host_transition_matrix(Q, d * r) for r in self.tl.cat_rates]))

    def update_partials(self):
        tree, tl = self.tree, self.tl
        ops = []
        for n in tree.postorder():
            if n < tree.tip_count:
                continue
            a, b = int(tree.left[n]), int(tree.right[n])
            ops += [tl.node_buffer_index(n), self.scale_index(n), _b.NONE, tl.node_buffer_index(a), tl.node_matrix_index(a),
                    tl.node_buffer_index(b), tl.node_matrix_index(b)]
        self.beagle.updatePartials(ops, len(ops) // 7, _b.NONE)

    def prune(self):
        """Model arrays, mutation-death matrices and one post-order pass: what BeagleTreeLikelihood.calculateLogLikelihood leaves."""
        self.beagle.setStateFrequencies(0, self.freqs)
        self.beagle.setCategoryWeights(0, self.tl.cat_weights)
        self.beagle.setCategoryRates(self.tl.cat_rates)
        self.update_matrices()
        self.update_partials()

    def node_rows(self):
        """-> (rows int32 [node_count][4] = {buffer, scale buffer or -1, child1 row, child2 row} in post-order, log weights
        [node_count], the tree node of each row)."""
        tree, tl = self.tree, self.tl
        order = tree.postorder()
        row_of = {n: r for r, n in enumerate(order)}
        rows = np.zeros((len(order), 4), dtype=np.int32)
        logw = np.zeros(len(order))
        for r, n in enumerate(order):
            tip = n < tree.tip_count
            rows[r] = [tl.node_buffer_index(n), self.scale_index(n), -1 if tip else row_of[int(tree.left[n])],
                       -1 if tip else row_of[int(tree.right[n])]]
            logw[r] = math.log(self.node_survival_probability(n))
        return rows, logw, np.asarray(order, dtype=np.int64)

    # ---- the node-pattern loop ----------------------------------------------------------------------------------------------
    def log_pattern_device(self, node_terms=False):
        rows, logw, _ = self.node_rows()
        log_cum, terms, total, rc = self.beagle.nodePatternLikelihoods(rows, logw, self.death_state, 0, 0, node_terms=node_terms)
        self.last = {"sum": total, "rc": rc, "terms": terms}
        return log_cum

    def read_back(self):
        """What the reference reads: every node's partials [node][C][P][S] (tips included) and every node's own log scale factors
        [node][P] (0 where none), by tree node number — a getPartials per node held as partials, a getLogScaleFactors per rescaled node."""
        tree, tl = self.tree, self.tl
        partials = np.empty((tree.node_count, self.C, self.P, self.S))
        scales = np.zeros((tree.node_count, self.P))
        for n in range(tree.node_count):
            if n < tree.tip_count and n not in self.tip_partials:
                codes = np.asarray(self.tip_states[n])
                one = np.ones((self.P, self.S))
                known = codes < self.S
                one[known] = 0.0
                one[known, codes[known]] = 1.0
                partials[n] = one[None]
            elif n < tree.tip_count:
                partials[n] = self.tip_partials[n][None]
            else:
                partials[n] = self.beagle.getPartials(tl.node_buffer_index(n), _b.NONE)
                if self.rescale:
                    scales[n] = self.beagle.getLogScaleFactors(self.scale_index(n))
        return partials, scales

    def tip_extant(self):
        """[tip][P] 0 / 1 (AnyTipObservationProcess.setTipNodePatternInclusion)."""
        tree = self.tree
        out = np.zeros((tree.tip_count, self.P), dtype=np.int64)
        for t in range(tree.tip_count):
            if t in self.tip_partials:
                out[t] = self.tip_partials[t][:, self.death_state] == 0.0
            else:
                codes = np.asarray(self.tip_states[t])
                out[t] = (codes < self.S) & (codes != self.death_state)
        return out

    def log_pattern_readback(self):
        tree = self.tree
        partials, scales = self.read_back()
        extant = self.tip_extant()
        total = extant.sum(axis=0)
        below = np.zeros((tree.node_count, self.P), dtype=np.int64)
        lam = np.zeros((tree.node_count, self.P))
        terms = np.full((tree.node_count, self.P), -np.inf)
        w = np.asarray(self.tl.cat_weights, dtype=np.float64)
        with np.errstate(divide="ignore"):
            for n in tree.postorder():
                if n < tree.tip_count:
                    below[n] = extant[n]
                else:
                    a, b = int(tree.left[n]), int(tree.right[n])
                    below[n] = below[a] + below[b]
                    lam[n] = (lam[a] + lam[b]) + scales[n]
                site = np.tensordot(w, partials[n] @ self.freqs, axes=1)
                term = (np.log(site) + lam[n]) + math.log(self.node_survival_probability(n))
                terms[n] = np.where(below[n] >= total, term, -np.inf)
            top = terms.max(axis=0)
            safe = np.where(np.isfinite(top), top, 0.0)
            log_cum = np.where(np.isfinite(top), safe + np.log(np.exp(terms - safe).sum(axis=0)), top)
        self.last = {"terms": terms[tree.postorder()]}
        return log_cum

    # ---- the host finish ----------------------------------------------------------------------------------------------------
    def ascertainment_correction(self, pattern_probs):
        """AbstractObservationProcess.getAscertainmentCorrection over the include / exclude pattern lists (1 without them)."""
        if not self.include and not self.exclude:
            return 1.0
        include_prob = exclude_prob = 0.0
        for i in self.include:
            include_prob += pattern_probs[i]
        for i in self.exclude:
            exclude_prob += pattern_probs[i]
        if include_prob == 0.0:
            return 1.0 - exclude_prob
        if exclude_prob == 0.0:
            return include_prob
        return include_prob - exclude_prob

    def log_tree_weight(self):
        """calculateLogTreeWeight of the observation process (AnyTipObservationProcess.java:57-94, SingleTipObservationProcess.java:57-59)."""
        rate = self.average_rate() * self.mu
        if self.observation == SINGLE_TIP:
            return -self.lam / rate
        tree = self.tree
        p = np.array([1.0 - self.node_survival_probability(n) for n in range(tree.node_count)])
        u0 = np.zeros(tree.node_count)
        weight = 0.0
        for n in tree.postorder():
            if n < tree.tip_count:
                u0[n] = 0.0
                weight += 1.0 - p[n]
            else:
                u0[n] = 1.0
                for c in (int(tree.left[n]), int(tree.right[n])):
                    u0[n] *= 1.0 - p[c] * (1.0 - u0[c])
                weight += (1.0 - u0[n]) * (1.0 - p[n])
        return -weight * self.lam / rate

    def finish(self, log_cum):
        """nodePatternLikelihood from the per-pattern values on (AbstractObservationProcess.java:212-228), with log cumLike in place
        of cumLike: log(cumLike / correction) = log cumLike - log correction."""
        weights = self.pattern_weights
        total_patterns = 0.0
        for x in weights:
            total_patterns += x
        gamma_norm = -math.lgamma(total_patterns + 1.0)
        log_n = math.log(total_patterns)
        with np.errstate(over="ignore"):
            correction = self.ascertainment_correction(np.exp(log_cum))
        log_correction = math.log(correction) if correction > 0.0 else float("nan")
        logl = gamma_norm
        for j in range(self.P):
            logl += (log_cum[j] - log_correction) * weights[j]
        tree_weight = self.log_tree_weight()
        if self.integrate_gain_rate:
            logl -= gamma_norm + log_n + math.log(-tree_weight * self.mu / self.lam) * total_patterns
        else:
            logl += tree_weight + math.log(self.lam / self.mu) * total_patterns
        return logl

    def getLogLikelihood(self, route=None):
        route = route or self.route
        self.prune()
        if route == "device":
            if not hasattr(self.beagle.lib.lib, NODE_PATTERN_SYMBOL):
                raise _b.BeagleException("nodePatternLikelihoods", -7)      # no quiet fall-back: a missing kernel is an error
            log_cum = self.log_pattern_device()
        elif route == "readback":
            log_cum = self.log_pattern_readback()
        else:
            raise ValueError("route: device or readback")
        self.last["log_pattern"] = log_cum
        return self.finish(log_cum)
