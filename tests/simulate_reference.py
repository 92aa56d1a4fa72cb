"""Host restatement of beagleMi355SimulateSequences (include/beagle_mi355.h), vectorised over sites.

Written from the call's documented behaviour: a rate category per site (given, or drawn from the category weights when there is
more than one, else 0), a root state per site (given, or drawn from the state frequencies), and for every other row of the
pre-order list a draw from M[category][parent state][.] of the row's branch matrix.  A draw over p_0 .. p_{n-1} forms cum_i =
cum_{i-1} + p_i from 0.0 in index order — one IEEE addition each; numpy does not contract to FMA — and returns the first i with
u < cum_i; when there is none, the largest index with p_i > 0; and 0, flagged, when the total is not finite and > 0.  The random
numbers are the engine's stateless SplitMix64 outputs (ancestral_reference.splitmix64) with counter (row * site_count + site) * 2
for a state and site * 2 + 1 for the rate category.  The matrices come from ``matrix_of`` — the engine's getTransitionMatrix, an
oracle's, or any callable — so the states must agree with the device's byte for byte.
"""
import numpy as np

from ancestral_reference import DBL_MAX, UNDECIDED, splitmix64


def uniforms(seed, row, sites, site_count, kind):
    """u[site] for the counter (row * site_count + site) * 2 + kind."""
    sites = np.asarray(sites, dtype=np.uint64)
    with np.errstate(over="ignore"):
        ctr = (np.uint64(row) * np.uint64(site_count) + sites) * np.uint64(2) + np.uint64(kind)
    return (splitmix64(seed, ctr) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def cumulative(p):
    """p [..., n] -> (cum [..., n]: the running sums along the last axis in index order, starting from 0.0; last_positive [...]:
    the largest index with p > 0, 0 when there is none; bad [...]: the total is not finite and > 0)."""
    p = np.asarray(p, dtype=np.float64)
    cum = np.empty_like(p)
    run = np.zeros(p.shape[:-1])
    last_positive = np.zeros(p.shape[:-1], dtype=np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(p.shape[-1]):
            run = run + p[..., i]
            cum[..., i] = run
            last_positive = np.where(p[..., i] > 0.0, i, last_positive)
        bad = ~((run > 0.0) & (run <= DBL_MAX))
    return cum, last_positive, bad


def draw(cum, last_positive, bad, u, undecided=None):
    """One draw per leading index: cum [m, n], last_positive [m], bad [m], u [m] -> (choice int64 [m], bad [m]).  `undecided`: a bool
    array [m] that is set where u lies within UNDECIDED x total of some running sum (the draw could come out differently under that
    relative change of p)."""
    with np.errstate(invalid="ignore"):
        above = u[:, None] < cum
        if undecided is not None:
            undecided |= (np.abs(u[:, None] - cum) <= UNDECIDED * cum[:, -1:]).any(axis=1)
    first = np.argmax(above, axis=1)                       # the first True; 0 when there is none
    choice = np.where(above.any(axis=1), first, last_positive)
    return np.where(bad, 0, choice), bad


def simulate(rows, matrix_of, category_weights, frequencies, seed, site_count, root_states=None, rate_categories=None, sites=None,
             undecided=None):
    """The call for `rows` ([n][3] {outRow, matrixIndex, parentRow}, root first; outRow is not looked at).

    matrix_of(matrixIndex) -> [C, S, S] as getTransitionMatrix returns it.  `sites`: restate only these site indices (default all).
    `undecided`: a bool array [len(sites)] that is set where some draw of the site lies next to a boundary (``draw``).
    -> (states uint8 [n, len(sites)] BY ROW OF THE LIST, categories int32 [len(sites)], any_bad)."""
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, 3)
    w = np.asarray(category_weights, dtype=np.float64)
    f = np.asarray(frequencies, dtype=np.float64)
    C, S = len(w), len(f)
    sites = np.arange(site_count) if sites is None else np.asarray(sites, dtype=np.int64)
    n = len(sites)
    any_bad = False
    if rate_categories is not None:
        cats = np.asarray(rate_categories, dtype=np.int64)[sites]
    elif C > 1:
        cum, last, bad = cumulative(w)
        cats, b = draw(np.broadcast_to(cum, (n, C)), np.broadcast_to(last, n), np.broadcast_to(bad, n),
                       uniforms(seed, 0, sites, site_count, 1), undecided)
        any_bad |= bool(b.any())
    else:
        cats = np.zeros(n, dtype=np.int64)
    states = np.zeros((len(rows), n), dtype=np.uint8)
    if root_states is not None:
        states[0] = np.asarray(root_states, dtype=np.uint8)[sites]
    else:
        cum, last, bad = cumulative(f)
        s0, b = draw(np.broadcast_to(cum, (n, S)), np.broadcast_to(last, n), np.broadcast_to(bad, n),
                     uniforms(seed, 0, sites, site_count, 0), undecided)
        any_bad |= bool(b.any())
        states[0] = s0
    tables = {}
    for r in range(1, len(rows)):
        m, parent = int(rows[r, 1]), int(rows[r, 2])
        if m not in tables:
            tables[m] = cumulative(np.asarray(matrix_of(m), dtype=np.float64).reshape(C, S, S))
        cum, last, bad = tables[m]
        ps = states[parent].astype(np.int64)
        s, b = draw(cum[cats, ps], last[cats, ps], bad[cats, ps], uniforms(seed, r, sites, site_count, 0), undecided)
        any_bad |= bool(b.any())
        states[r] = s
    return states, cats.astype(np.int32), any_bad


def simulate_from_engine(beagle, rows, category_weights, frequencies, seed, site_count, **kw):
    """`simulate` over the branch matrices the engine instance behind `beagle` (a beagle.Beagle binding) reads back."""
    cache = {}

    def matrix_of(m):
        if m not in cache:
            cache[m] = beagle.getTransitionMatrix(m)
        return cache[m]

    return simulate(rows, matrix_of, category_weights, frequencies, seed, site_count, **kw)
