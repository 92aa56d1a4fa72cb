"""Host restatement of the stochastic Dollo (ALS) likelihood, loop for loop after the reference
(src/dr/oldevomodel/MSSD/AbstractObservationProcess.java:134-229, AnyTipObservationProcess.java:57-168,
SingleTipObservationProcess.java:57-59, src/dr/oldevomodel/treelikelihood/ScaleFactorsHelper.java:83-140), and of what
beagleMi355NodePatternLikelihoods (include/beagle_mi355.h) makes of the same inputs.

Everything takes the partials of every node [node][C][P][S] (tips included) and every node's OWN log scale factors [node][P] as a
library returns them, and a ``dtype``: np.float64 (the reference's arithmetic) or np.longdouble (the yardstick: the same loops in
the 64-bit-mantissa format, inputs converted exactly).  Two forms of the per-pattern value:

  linear_cum      the reference's: partials multiplied back by exp(Lambda), cumLike[j] += exp(log(site) + logProb) over the nodes in
                  node-number order — underflows on large trees;
  log_terms / log_cum   the device's: term = (log site + Lambda) + logw per included node, then a running-maximum log-sum-exp over
                  the rows in list order.

Where linear_cum does not underflow, exp(log_cum) is linear_cum (up to rounding).
"""
import math

import numpy as np


def tip_extant(tip_states, tip_partials, S, death_state):
    """[tip][P] 0 / 1: AnyTipObservationProcess.setTipNodePatternInclusion.  ``tip_states`` [T][P] codes; ``tip_partials``: {tip:
    [P][S]} for the tips held as partials (their code contains the death state where partial[death] != 0)."""
    tip_states = np.asarray(tip_states)
    T, P = tip_states.shape
    out = np.zeros((T, P), dtype=np.int64)
    for t in range(T):
        for j in range(P):
            if t in tip_partials:
                out[t, j] = 1 if tip_partials[t][j][death_state] == 0.0 else 0
            else:
                s = int(tip_states[t, j])
                out[t, j] = 1 if (s < S and s != death_state) else 0
    return out


def inclusion(tree, extant):
    """-> (extantInTipsBelow [node][P], nodePatternInclusion [node][P]): setNodePatternInclusion."""
    P = extant.shape[1]
    total = extant.sum(axis=0)
    below = np.zeros((tree.node_count, P), dtype=np.int64)
    below[:tree.tip_count] = extant
    for n in tree.postorder():
        if n >= tree.tip_count:
            below[n] = below[int(tree.left[n])] + below[int(tree.right[n])]
    return below, below >= total[None, :]


def subtree_scale_factors(tree, own, dtype):
    """[node][P]: ScaleFactorsHelper.traverseComputeScaleFactors — child0 + child1 + the node's own, 0 at the tips."""
    lam = np.zeros(own.shape, dtype=dtype)
    for n in tree.postorder():
        if n >= tree.tip_count:
            lam[n] = (lam[int(tree.left[n])] + lam[int(tree.right[n])]) + own[n].astype(dtype)
    return lam


def site_values(partials_n, freqs, cat_weights, dtype, scale=None):
    """[P]: sum_c w_c sum_s pi_s x[c][j][s] (x multiplied by scale[j] first: ScaleFactorsHelper.rescalePartials), s and c upwards."""
    C, P, S = partials_n.shape
    x = partials_n.astype(dtype)
    pi, w = np.asarray(freqs).astype(dtype), np.asarray(cat_weights).astype(dtype)
    site = np.zeros(P, dtype=dtype)
    for c in range(C):
        inner = np.zeros(P, dtype=dtype)
        for s in range(S):
            xs = x[c, :, s] if scale is None else x[c, :, s] * scale
            inner = inner + pi[s] * xs
        site = site + w[c] * inner
    return site


def linear_cum(tree, partials, own_scales, incl, freqs, cat_weights, log_weights_by_node, dtype):
    """cumLike [P] as nodePatternLikelihood forms it (AbstractObservationProcess.java:189-210): nodes in node-number order."""
    lam = subtree_scale_factors(tree, own_scales, dtype)
    P = partials.shape[2]
    cum = np.zeros(P, dtype=dtype)
    with np.errstate(divide="ignore", under="ignore"):
        for n in range(tree.node_count):
            scale = np.exp(lam[n]) if n >= tree.tip_count else None
            site = site_values(partials[n], freqs, cat_weights, dtype, scale)
            value = np.exp(np.log(site) + dtype(log_weights_by_node[n]))
            cum = cum + np.where(incl[n], value, dtype(0.0))
    return cum


def log_terms(tree, order, partials, own_scales, incl, freqs, cat_weights, log_weights_by_node, dtype):
    """-> (terms [row][P], the largest |operand| entering each term [row][P]) for the rows ``order`` (tree nodes in list order)."""
    lam = subtree_scale_factors(tree, own_scales, dtype)
    P = partials.shape[2]
    terms = np.full((len(order), P), -np.inf, dtype=dtype)
    operand = np.zeros((len(order), P), dtype=dtype)
    with np.errstate(divide="ignore"):
        for r, n in enumerate(order):
            log_site = np.log(site_values(partials[n], freqs, cat_weights, dtype))
            lw = dtype(log_weights_by_node[n])
            terms[r] = np.where(incl[n], (log_site + lam[n]) + lw, dtype(-np.inf))
            operand[r] = np.maximum(np.maximum(np.abs(log_site), np.abs(lam[n])), abs(lw))
    return terms, operand


def log_cum(terms, dtype):
    """[P]: the running-maximum log-sum-exp of include/beagle_mi355.h over the rows in order."""
    R, P = terms.shape
    out = np.empty(P, dtype=dtype)
    for j in range(P):
        m, s = dtype(-np.inf), dtype(0.0)
        for r in range(R):
            t = terms[r, j]
            if t > m:
                s = s * np.exp(m - t) + dtype(1.0)
                m = t
            elif t > -np.inf:
                s = s + np.exp(t - m)
        out[j] = m + np.log(s) if s > 0 else dtype(-np.inf)
    return out


def bound(value64, value_ld, largest_operand, factor=8.0):
    """The tolerance tests/generator_matrices_reference.py's way: ``factor`` x max(what the float64 restatement loses against the
    long-double one, eps x (|value| + the largest |operand| entering it)) — elementwise; where the value is -inf it is 0 (exact)."""
    eps = np.finfo(np.float64).eps
    v = np.asarray(value_ld, dtype=np.longdouble)
    finite = np.isfinite(v)
    with np.errstate(invalid="ignore"):
        lost = np.where(finite, np.abs(np.asarray(value64, dtype=np.longdouble) - v), 0)
    floor = eps * (np.where(finite, np.abs(v), 0) + np.asarray(largest_operand, dtype=np.longdouble))
    return np.where(finite, factor * np.maximum(lost, floor), 0).astype(np.float64)


def node_survival_probability(tree, node, mu, average_rate, branch_rates=None):
    """getNodeSurvivalProbability: 1 - exp(-(mu avgRate) (rate_i t_i)), 1 at the root."""
    parent = int(tree.parent[node])
    if parent < 0:
        return 1.0
    rate = 1.0 if branch_rates is None else float(branch_rates[node])
    return 1.0 - math.exp(-(mu * average_rate) * (rate * (float(tree.height[parent]) - float(tree.height[node]))))


def log_tree_weight(tree, mu, lam, average_rate, observation="anyTip", branch_rates=None):
    """calculateLogTreeWeight (AnyTipObservationProcess.java:57-94; SingleTipObservationProcess.java:57-59)."""
    if observation == "singleTip":
        return -lam / (average_rate * mu)
    p = [1.0 - node_survival_probability(tree, n, mu, average_rate, branch_rates) for n in range(tree.node_count)]
    u0 = [0.0] * tree.node_count
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
    return -weight * lam / (average_rate * mu)


def tree_weight_sum(tree, mu, average_rate, branch_rates=None):
    """sum_i (1 - u0_i)(1 - p_i): calculateLogTreeWeight's logWeight before it is scaled by -lam / (avgRate mu)."""
    return -log_tree_weight(tree, mu, 1.0, average_rate, "anyTip", branch_rates) * (average_rate * mu)


def ascertainment_correction(pattern_probs, include, exclude):
    """getAscertainmentCorrection (AbstractObservationProcess.java:231-255); no lists: 1."""
    if not include and not exclude:
        return 1.0
    include_prob = exclude_prob = 0.0
    for i in include:
        include_prob += float(pattern_probs[i])
    for i in exclude:
        exclude_prob += float(pattern_probs[i])
    if include_prob == 0.0:
        return 1.0 - exclude_prob
    if exclude_prob == 0.0:
        return include_prob
    return include_prob - exclude_prob


def finish(log_cum_values, pattern_weights, tree, mu, lam, average_rate, observation="anyTip", integrate_gain_rate=False, include=(),
           exclude=(), branch_rates=None):
    """nodePatternLikelihood from cumLike on (AbstractObservationProcess.java:212-228), taking log cumLike."""
    total = 0.0
    for w in pattern_weights:
        total += float(w)
    gamma_norm = -math.lgamma(total + 1.0)
    correction = ascertainment_correction(np.exp(np.asarray(log_cum_values, dtype=np.float64)), list(include), list(exclude))
    logl = gamma_norm
    for j in range(len(pattern_weights)):
        logl += (float(log_cum_values[j]) - math.log(correction)) * float(pattern_weights[j])
    weight = log_tree_weight(tree, mu, lam, average_rate, observation, branch_rates)
    if integrate_gain_rate:
        logl -= gamma_norm + math.log(total) + math.log(-weight * mu / lam) * total
    else:
        logl += weight + math.log(lam / mu) * total
    return logl
