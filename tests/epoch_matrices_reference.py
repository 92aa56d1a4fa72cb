"""The yardstick of beagleMi355UpdateTransitionMatricesWithEpochs (include/beagle_mi355.h; csrc/kernels_epoch.hip) and the cases the
CPU and GPU tiers share.

The yardstick takes the float64 eigen system as it is — the same input the device reads — and forms every segment matrix
U exp(Lambda d) U^-1 and the left fold of the segments in ``np.longdouble`` (64-bit mantissa): real eigen systems and the real block
form of conjugate pairs (inputs.substmodel.decompose_complex; csrc/transition_body.h iexpEntry), negative entries clamped to 0 per
segment as beagleUpdateTransitionMatrices clamps them, the products not clamped.  Its own error is a few 2^-64 per operation: three
decimal digits below what it measures.
"""
import functools

import numpy as np

from beast_mcmc_amd.inputs import substmodel

LD = np.longdouble
EPS = 2.0 ** -53
CATEGORY_RATES = (0.1, 0.5, 1.0, 3.0)
EIGEN_SYSTEMS = 3

# (eigen system, length) per segment, root end first: n = 1, 2, 3 and 7; a zero-length segment alone, at the root end and inside an
# entry; the same eigen system twice in a row; lengths from 1e-6 to 10
ENTRIES = (
    ((0, 0.37),),
    ((1, 1e-6),),
    ((2, 10.0),),
    ((0, 0.0),),
    ((0, 0.2), (1, 0.5)),
    ((2, 1e-6), (2, 3.0)),
    ((1, 0.0), (0, 1.3)),
    ((2, 0.05), (1, 0.4), (0, 0.9)),
    ((0, 10.0), (1, 1e-3), (2, 0.1)),
    ((0, 0.1), (1, 0.2), (2, 0.3), (2, 0.0), (1, 1e-6), (0, 2.0), (0, 0.7)),
    ((2, 1e-4), (0, 5.0), (1, 0.01), (2, 1.0), (0, 0.3), (1, 0.05), (2, 0.6)),
)


def packed(entries=ENTRIES):
    """-> (offsets [n + 1], eigen index per segment, length per segment) as the call takes them"""
    offsets, eig, lengths = [0], [], []
    for entry in entries:
        for k, t in entry:
            eig.append(k); lengths.append(t)
        offsets.append(len(eig))
    return np.asarray(offsets, dtype=np.int32), np.asarray(eig, dtype=np.int32), np.asarray(lengths, dtype=np.float64)


@functools.lru_cache(maxsize=None)
def real_systems(S, seed=0):
    """EIGEN_SYSTEMS reversible models of S states (GTR at 4 states)"""
    rng = np.random.default_rng(1000 * S + seed)
    out = []
    for _ in range(EIGEN_SYSTEMS):
        if S == 4:
            out.append(substmodel.gtr(rng.gamma(2.0, 1.0, size=6) + 0.1, rng.dirichlet(np.full(4, 10.0))))
        else:
            out.append(substmodel.random_reversible(S, rng)[0])
    return tuple(out)


@functools.lru_cache(maxsize=None)
def complex_systems(S, seed=0):
    """EIGEN_SYSTEMS non-reversible models of S states in the real block form (eigenvalues [S real parts | S imaginary parts]); at
    least one of them has a conjugate pair"""
    rng = np.random.default_rng(2000 * S + seed)
    out = []
    for _ in range(EIGEN_SYSTEMS):
        q = rng.uniform(0.05, 5.0, size=(S, S))
        np.fill_diagonal(q, 0.0)
        np.fill_diagonal(q, -q.sum(axis=1))
        out.append(substmodel.decompose_complex(q)[1])
    assert any(np.any(e.evals[S:] != 0.0) for e in out)
    return tuple(out)


def segment_matrix(eig, d, complex_eigen=False):
    """U exp(Lambda d) U^-1 in longdouble from the float64 eigen system, negative entries clamped to 0"""
    U, Ui = np.asarray(eig.evec, dtype=LD), np.asarray(eig.ievc, dtype=LD)
    S = U.shape[0]
    lam = np.asarray(eig.evals, dtype=LD)
    d = LD(d)
    iexp = np.empty((S, S), dtype=LD)
    k = 0
    while k < S:
        im = lam[S + k] if complex_eigen else LD(0.0)
        if im == 0.0:
            iexp[k] = Ui[k] * np.exp(d * lam[k])
            k += 1
            continue
        expat = np.exp(d * lam[k])
        c, s = expat * np.cos(d * im), expat * np.sin(d * im)
        iexp[k] = c * Ui[k] + s * Ui[k + 1]
        iexp[k + 1] = c * Ui[k + 1] - s * Ui[k]
        k += 2
    m = U.dot(iexp)
    m[m < 0.0] = LD(0.0)
    return m


def yardstick(systems, entry, rate, complex_eigen=False):
    """((M_0 M_1) M_2) ... of an entry's segments at one category rate, longdouble.  The distance of a segment is the float64 product
    length * rate the device forms."""
    out = None
    for k, t in entry:
        m = segment_matrix(systems[k], float(np.float64(t) * np.float64(rate)), complex_eigen)
        out = m if out is None else out.dot(m)
    return out


def tolerance(e_stock, n, S):
    """8 max(e_stock, n S eps): the project's standing margin over float64's own error, floored by the rounding of n sums of S products
    of entries <= 1 (a lucky e_stock must not fail a correct kernel)"""
    return 8.0 * max(float(e_stock), n * S * EPS)


def replay_pool(log, matrix_buffer_count):
    """Walks a host-route log (epochs.EpochTransitionMatrices.log) and checks the pool discipline: a buffer of the pool (or the
    reserve) is never written while it holds a matrix nobody has consumed yet, and never read when it holds none.  -> the number of
    writes to buffers at or behind matrix_buffer_count."""
    live, writes = set(), 0

    def write(slot):
        nonlocal writes
        if slot >= matrix_buffer_count:
            assert slot not in live, ("written while live", slot)
            live.add(slot); writes += 1

    def read(slot):
        if slot >= matrix_buffer_count:
            assert slot in live, ("read while empty", slot)
            live.discard(slot)

    for rec in log:
        if rec[0] == "update":
            for slot in rec[2]:
                write(slot)
        else:
            _, first, second, result = rec
            assert len(set(result)) == len(result)
            for f, s in zip(first, second):
                read(f); read(s)
            for r in result:
                write(r)
    assert not live, ("left live", live)
    return writes
