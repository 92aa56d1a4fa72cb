"""Host restatement of the regraft scores (include/beagle_mi355.h beagleMi355RegraftScores) in numpy: float64 and np.longdouble twins
of the formulas, over partials and matrices handed to them.  Every sum runs over its index in ascending order from 0.0.

``log_ratio``   R[p] = log(N_p / D_p) + logscale[p] of ONE candidate from (pre, sib, Msib, child, Mup, Mlow, Mpend) and the subtree's
                partials — partials [C, P, S], matrices [C, S, S] with M[c][a][b] = P(a -> b), None where the candidate names none.
``scores``      score[k] = sum_p w_p R_k[p], p ascending, a pattern of weight 0 left out.
``gamma`` / ``score_bound``   the first-order bounds: per entry (4 S + C + 12 + |R|) eps — the placement entry's with one more mat-vec
                (tests/placement_reference.py) — per score the entries' bounds weighted by the pattern weights plus
                P eps sum |w_p R_p| (safe for any summation order).
"""
import numpy as np

from placement_reference import EPS, _matvec, _vecmat, within        # noqa: F401  (within: the shared acceptance rule)


def log_ratio(pre, sib, m_sib, child, m_up, m_low, m_pend, subtree, weights, logscale=None, dtype=np.float64):
    """-> (R [P], bad [P]): bad where D is 0 or not finite (R is NaN there)."""
    cast = lambda x: None if x is None else np.asarray(x).astype(dtype)            # noqa: E731
    pre, sib, m_sib, child, m_up, m_low, m_pend, subtree = (cast(x) for x in (pre, sib, m_sib, child, m_up, m_low, m_pend, subtree))
    w = np.asarray(weights).astype(dtype)
    C, P, S = pre.shape
    u = pre if sib is None else pre * _matvec(m_sib, sib, dtype)
    t = u if m_up is None else _vecmat(u, m_up, dtype)
    e = t * _matvec(m_low, child, dtype)
    q = _matvec(m_pend, subtree, dtype)
    D = np.zeros(P, dtype=dtype)
    N = np.zeros(P, dtype=dtype)
    for c in range(C):
        d = np.zeros(P, dtype=dtype)
        n = np.zeros(P, dtype=dtype)
        for a in range(S):
            d = d + e[c, :, a]
            n = n + e[c, :, a] * q[c, :, a]
        D = D + w[c] * d
        N = N + w[c] * n
    bad = ~(np.isfinite(D) & (D != 0))
    with np.errstate(divide="ignore", invalid="ignore"):
        R = np.log(N / np.where(bad, np.nan, D))
    if logscale is not None:
        R = R + np.asarray(logscale).astype(dtype)
    return R, bad


def log_ratios(operands, subtree, weights, logscale=None, dtype=np.float64):
    """The ratios of a list of candidates (Placement.read_back's tuples): [K, P]."""
    return np.stack([log_ratio(*op, subtree, weights, logscale, dtype=dtype)[0] for op in operands])


def scores(ratios, pattern_weights, dtype=np.float64):
    """-> [K]; a pattern of weight 0 adds nothing at all."""
    R = np.asarray(ratios).astype(dtype)
    w = np.asarray(pattern_weights, dtype=np.float64)
    out = np.zeros(R.shape[0], dtype=dtype)
    for p in range(R.shape[1]):
        if w[p] != 0.0:
            out = out + w[p].astype(dtype) * R[:, p]
    return out


def gamma(R, S, C):
    return (4 * S + C + 12 + np.abs(np.asarray(R, dtype=np.float64))) * EPS


def score_bound(ratios, pattern_weights, S, C):
    """Gamma [K] = sum_p w_p gamma(R_p) + P eps sum_p |w_p R_p| over the patterns of weight != 0 (an infinite entry: an infinite bound)."""
    R = np.asarray(ratios, dtype=np.float64)
    w = np.abs(np.asarray(pattern_weights, dtype=np.float64))
    with np.errstate(invalid="ignore"):
        return scores(gamma(R, S, C), w) + R.shape[1] * EPS * scores(np.abs(R), w)
