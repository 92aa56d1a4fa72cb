"""An independent restatement, pattern by pattern as the reference writes them, of the two tip error models whose partials the engine
takes as emission tables: SequenceErrorModel.getTipPartials and HypermutantErrorModel.getTipPartials
(src/dr/evomodel/tipstatesmodel/).  Plain loops over the alignment states (0..3 = A, C, G, T; 5 = an A in a hypermutation context;
anything else an ambiguity) — nothing here knows about tables."""
import math

import numpy as np

A, C, G, T, R = 0, 1, 2, 3, 5


def sequence_error_partials(states, error_type, base_rate, age_rate, tip_age, has_indicator, indicator_value, excluded):
    """``error_type``: "all" or "transitions"; ``base_rate`` / ``age_rate``: None when the model has no such parameter."""
    out = np.zeros((len(states), 4))
    if (not has_indicator) or indicator_value > 0.0:
        p_undamaged, p_ts, p_tv = 1.0, 0.0, 0.0
        if not excluded:
            if base_rate is not None:
                p_undamaged = p_undamaged - base_rate
            if age_rate is not None:
                p_undamaged *= math.exp(-age_rate * tip_age)
            if error_type == "all":
                p_ts = (1.0 - p_undamaged) / 3.0
                p_tv = p_ts
            elif error_type == "transitions":
                p_ts = 1.0 - p_undamaged
                p_tv = 0.0
            else:
                raise ValueError(error_type)
        for j, s in enumerate(states):
            if s == A:
                out[j] = (p_undamaged, p_tv, p_ts, p_tv)
            elif s == C:
                out[j] = (p_tv, p_undamaged, p_tv, p_ts)
            elif s == G:
                out[j] = (p_ts, p_tv, p_undamaged, p_tv)
            elif s == T:
                out[j] = (p_tv, p_ts, p_tv, p_undamaged)
            else:
                out[j] = (1.0, 1.0, 1.0, 1.0)
    else:
        for j, s in enumerate(states):
            if s == A:
                out[j] = (1.0, 0.0, 0.0, 0.0)
            elif s == C:
                out[j] = (0.0, 1.0, 0.0, 0.0)
            elif s == G:
                out[j] = (0.0, 0.0, 1.0, 0.0)
            elif s == T:
                out[j] = (0.0, 0.0, 0.0, 1.0)
            else:
                out[j] = (1.0, 1.0, 1.0, 1.0)
    return out


def hypermutant_partials(states, rate, is_hypermutated):
    out = np.zeros((len(states), 4))
    for j, s in enumerate(states):
        if s == A:
            out[j] = (1.0, 0.0, 0.0, 0.0)
        elif s == C:
            out[j] = (0.0, 1.0, 0.0, 0.0)
        elif s == G:
            out[j] = (0.0, 0.0, 1.0, 0.0)
        elif s == T:
            out[j] = (0.0, 0.0, 0.0, 1.0)
        elif s == R:
            out[j] = (1.0 - rate, 0.0, rate, 0.0) if is_hypermutated else (1.0, 0.0, 0.0, 0.0)
        else:
            out[j] = (1.0, 1.0, 1.0, 1.0)
    return out


def prune(tree, codes, matrices, freqs, cat_weights, pattern_weights):
    """Felsenstein pruning over COMPACT tips in numpy: ``codes`` [T][P] (a code >= S: missing), ``matrices`` {node: [C][S][S]} — a tip's
    matrix may be any [C][S][S] array (a folded one).  -> (lnL, site lnL)."""
    T, S = tree.tip_count, len(freqs)
    partial = {}
    for n in tree.postorder():
        if n < T:
            continue
        prod = None
        for ch in (int(tree.left[n]), int(tree.right[n])):
            m = np.asarray(matrices[ch])                                 # [C][S][S]
            if ch < T:
                c = np.asarray(codes[ch])
                known = c < S
                v = np.ones((m.shape[0], len(c), S))
                v[:, known, :] = np.transpose(m[:, :, c[known]], (0, 2, 1))      # column `code` of the matrix
            else:
                v = np.einsum("cij,cpj->cpi", m, partial[ch])
            prod = v if prod is None else prod * v
        partial[n] = prod
    site = np.einsum("c,cpi,i->p", np.asarray(cat_weights), partial[tree.root], np.asarray(freqs))
    site = np.log(site)
    return float(np.dot(site, pattern_weights)), site
