"""Host restatement of the placement scores (include/beagle_mi355.h beagleMi355PlacementScores) in numpy: float64 and np.longdouble
twins of the formulas, over partials and matrices handed to them.  Every sum runs over its index in ascending order from 0.0.

``log_table``   T[p][x] = log(N_p,x / D_p) of ONE candidate from (pre, sib, Msib, child, Mup, Mlow, Mpend) — partials [C, P, S],
                matrices [C, S, S] with M[c][a][b] = P(a -> b), None where the candidate names none.
``scores``      score[q][k] = sum over the kept sites i, ascending, of T_k[sitePatterns[i]][queryCodes[q][i]].
``gamma`` / ``score_bound``   the first-order bounds of the issue: per entry (3 S + C + 12 + |T|) eps, per score the entries' bounds
                added up plus siteCount eps sum |T_i| (safe for any summation order).
"""
import numpy as np

EPS = 2.0 ** -53
MISSING = 255


def _matvec(m, v, dtype):
    """out[c][p][a] = sum_b m[c][a][b] v[c][p][b], b ascending from 0.0"""
    out = np.zeros(v.shape, dtype=dtype)
    for b in range(v.shape[2]):
        out = out + m[:, None, :, b] * v[:, :, b, None]
    return out


def _vecmat(v, m, dtype):
    """out[c][p][a] = sum_a' v[c][p][a'] m[c][a'][a], a' ascending from 0.0"""
    out = np.zeros(v.shape, dtype=dtype)
    for a in range(v.shape[2]):
        out = out + v[:, :, a, None] * m[:, None, a, :]
    return out


def log_table(pre, sib, m_sib, child, m_up, m_low, m_pend, weights, code_table, dtype=np.float64):
    """-> (T [P, X], bad [P]): bad where D is 0 or not finite (T is NaN there)."""
    cast = lambda x: None if x is None else np.asarray(x).astype(dtype)            # noqa: E731
    pre, sib, m_sib, child, m_up, m_low, m_pend = (cast(x) for x in (pre, sib, m_sib, child, m_up, m_low, m_pend))
    w, g = np.asarray(weights).astype(dtype), np.asarray(code_table).astype(dtype)
    C, P, S = pre.shape
    X = g.shape[0]
    u = pre if sib is None else pre * _matvec(m_sib, sib, dtype)
    t = u if m_up is None else _vecmat(u, m_up, dtype)
    e = t * _matvec(m_low, child, dtype)
    G = np.zeros((C, S, X), dtype=dtype)                                            # G[c][a][x] = sum_b Mpend[c][a][b] g[x][b]
    for b in range(S):
        G = G + m_pend[:, :, b, None] * g[None, None, :, b]
    D = np.zeros(P, dtype=dtype)
    N = np.zeros((P, X), dtype=dtype)
    for c in range(C):
        d = np.zeros(P, dtype=dtype)
        n = np.zeros((P, X), dtype=dtype)
        for a in range(S):
            d = d + e[c, :, a]
            n = n + e[c, :, a, None] * G[c, a][None, :]
        D = D + w[c] * d
        N = N + w[c] * n
    bad = ~(np.isfinite(D) & (D != 0))
    with np.errstate(divide="ignore", invalid="ignore"):
        T = np.log(N / np.where(bad, np.nan, D)[:, None])
    return T, bad


def log_tables(operands, weights, code_table, dtype=np.float64):
    """The tables of a list of candidates (Placement.read_back's tuples): [K, P, X]."""
    return np.stack([log_table(*op, weights, code_table, dtype=dtype)[0] for op in operands])


def scores(tables, site_patterns, query_codes, dtype=np.float64):
    """-> [Q, K]; a skipped site (pattern -1) or a missing code (255) adds nothing at all."""
    T = np.asarray(tables).astype(dtype)
    sites = np.asarray(site_patterns, dtype=np.int64).reshape(-1)
    codes = np.asarray(query_codes, dtype=np.int64).reshape(-1, len(sites))
    out = np.zeros((len(codes), T.shape[0]), dtype=dtype)
    for i, p in enumerate(sites):
        if p < 0:
            continue
        kept = codes[:, i] != MISSING
        if kept.any():
            out[kept] = out[kept] + T[:, p, codes[kept, i]].T
    return out


def gamma(T, S, C):
    return (3 * S + C + 12 + np.abs(np.asarray(T, dtype=np.float64))) * EPS


def score_bound(tables, site_patterns, query_codes, S, C):
    """Gamma [Q, K] = sum_i gamma(T_i) + siteCount eps sum_i |T_i| over the kept sites (infinite entries: an infinite bound)."""
    T = np.asarray(tables, dtype=np.float64)
    sites = np.asarray(site_patterns, dtype=np.int64).reshape(-1)
    with np.errstate(invalid="ignore"):
        return scores(gamma(T, S, C), sites, query_codes) + len(sites) * EPS * scores(np.abs(T), sites, query_codes)


def within(dev, f64, ld, floor):
    """|dev - ld| <= 8 max(|f64 - ld|, floor) entry by entry, equal infinities and NaN at the same places counting as agreement;
    -> (ok, largest |dev - ld| / max(|f64 - ld|, floor))."""
    dev, f64 = np.asarray(dev, dtype=np.longdouble), np.asarray(f64, dtype=np.longdouble)
    finite = np.isfinite(ld)
    same = np.array_equal(np.isnan(dev), np.isnan(ld)) and np.array_equal(dev[~finite & ~np.isnan(ld)], ld[~finite & ~np.isnan(ld)])
    if not finite.any():
        return same, 0.0
    yard = np.maximum(np.abs(f64[finite] - ld[finite]), np.asarray(floor, dtype=np.longdouble)[finite])
    ratio = np.abs(dev[finite] - ld[finite]) / yard
    return bool(same and np.all(np.isfinite(dev[finite])) and np.all(ratio <= 8)), float(np.max(ratio))
