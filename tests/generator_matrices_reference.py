"""Host restatement of beagleMi355UpdateTransitionMatricesFromGenerators (include/beagle_mi355.h; csrc/kernels_generator.hip) in
float64 numpy, a longdouble yardstick that no eigensolver takes part in, the eigen route it stands next to, and the generators the
tests use.

The restatement follows the header's arithmetic line by line: mu scanned upwards, B = Q / mu + I, the power table by ordered products
(markov_jumps_reference.mm: inner index upwards, one rounding per product and per sum), s and tau by exact scaling, the weights by the
recurrence, the combination k upwards, s ordered squarings.  The device fuses the multiply-adds of the combination and the squarings
and, from 16 states on, sums the inner index four at a time: its bits differ from the restatement's, its error bound does not —
every term is non-negative, so each entry carries a relative error of a few eps per operation of its own, doubled by each squaring.
"""
import functools
import math

import numpy as np

import markov_jumps_reference as mj
from beast_mcmc_amd.inputs import substmodel

EPS = 2.0 ** -52
TERMS = 21
MAX_SQUARINGS = 40
LENGTHS = (0.0, 1e-6, 1e-3, 0.1, 1.0, 10.0, 100.0)
CATEGORY_RATES = (0.1, 0.5, 1.0, 3.0)
LD = np.longdouble


# ---- the generators of the tests ---------------------------------------------------------------------------------------------
def _close(q):
    np.fill_diagonal(q, 0.0)
    q[np.diag_indices(len(q))] = -q.sum(axis=1)
    return q


def dense(S, rng):
    """every rate Gamma(1, 1)"""
    return _close(rng.gamma(1.0, 1.0, (S, S)))


def bssvs(S, rng):
    """rates kept with probability 3 / S, plus a ring i -> i + 1 of 0.3: most indicators off"""
    q = rng.gamma(1.0, 1.0, (S, S)) * (rng.random((S, S)) < 3.0 / S)
    np.fill_diagonal(q, 0.0)
    for i in range(S):
        q[i, (i + 1) % S] += 0.3
    return _close(q)


def stiff(S, rng):
    """rates 10^U(-4, 4)"""
    return _close(10.0 ** rng.uniform(-4, 4, (S, S)))


def chain(S=8):
    """the one-way chain i -> i + 1 at rate 1: a single Jordan block, no eigen system at all"""
    q = np.zeros((S, S))
    for i in range(S - 1):
        q[i, i + 1] = 1.0
        q[i, i] = -1.0
    return q


@functools.lru_cache(maxsize=None)
def generators(S):
    """name -> generator of the cases at S states: dense, BSSVS-like and stiff; at 8 states the chain takes the dense one's place."""
    rng = np.random.default_rng(7000 + S)
    out = {"dense": dense(S, rng), "bssvs": bssvs(S, rng), "stiff": stiff(S, rng)}
    if S == 8:
        del out["dense"]
        out["chain"] = chain(8)
    return out


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
def max_rate(q):
    """mu = max_i -Q_ii, scanned upwards: a later entry replaces an earlier one only if greater (engine_sampling.cpp uniformChain)"""
    m = -q[0, 0]
    for i in range(1, len(q)):
        if -q[i, i] > m:
            m = -q[i, i]
    return float(m)


def power_table(q):
    """-> (mu, [B^0 .. B^20])"""
    q = np.asarray(q, dtype=np.float64)
    S = len(q)
    mu = max_rate(q)
    B = q / mu
    B[np.diag_indices(S)] += 1.0
    table = [np.eye(S), B]
    for _ in range(2, TERMS):
        table.append(mj.mm(table[-1], B))
    return mu, table


def squarings(x):
    """-> (s, tau): the smallest s >= 0 with x 2^-s <= 1, and x 2^-s"""
    if not x > 1.0:
        return 0, x
    m, e = math.frexp(x)
    s = e - 1 if m == 0.5 else e
    return s, math.ldexp(x, -s)


def from_table(mu, table, d):
    """-> (T, s): exp(Q d) as the header forms it; NaN when s > 40"""
    s, tau = squarings(mu * d)
    if s > MAX_SQUARINGS or not math.isfinite(mu * d):
        return np.full_like(table[0], np.nan), s
    w = math.exp(-tau)
    T = w * table[0]
    for k in range(1, TERMS):
        w = w * tau / k
        T = T + w * table[k]
    for _ in range(s):
        T = mj.mm(T, T)
    return T, s


def restatement(q, d):
    mu, table = power_table(q)
    return from_table(mu, table, d)


# ---- the yardstick ---------------------------------------------------------------------------------------------------------------------
def yardstick(q, d):
    """exp(Q d) in longdouble: a 40-term Taylor series of Q d / 2^s, ||.||_inf / 2^s <= 1 / 16, squared s times"""
    A = np.asarray(q).astype(LD) * LD(d)
    n = float(np.abs(A).sum(axis=1).max())
    s = max(0, int(math.ceil(math.log2(n))) + 4) if n > 0 else 0
    A = A / LD(2) ** s
    T = np.eye(len(A), dtype=LD)
    term = np.eye(len(A), dtype=LD)
    for k in range(1, 40):
        term = term @ A / LD(k)
        T = T + term
    for _ in range(s):
        T = T @ T
    return T


def floor(s):
    """the Taylor tail 1 / 21! <= 2e-20 of the restatement, carried through s squarings"""
    return 2.0 ** s * 1e-19


def bound(s):
    """componentwise relative error the scheme is pinned to: 20 terms of a few eps each, doubled by every squaring"""
    return 8.0 * (2.0 ** s + 20.0) * EPS


def relative_error(T, Y, s):
    """max over entries of (|T - Y| - floor) / Y: e_ref when T is the restatement"""
    T, Y = np.asarray(T, dtype=LD), np.asarray(Y, dtype=LD)
    excess = np.maximum(np.abs(T - Y) - LD(floor(s)), 0)
    if np.any((Y <= 0) & (excess > 0)):
        return math.inf
    pos = Y > 0
    return float((excess[pos] / Y[pos]).max()) if pos.any() else 0.0


@functools.lru_cache(maxsize=None)
def reference(S, name, d):
    """-> (yardstick rounded to double as longdouble array, s, e_ref) of generator `name` at S states and distance d; computed once"""
    q = generators(S)[name]
    mu, table = _tables(S, name)
    T, s = from_table(mu, table, d)
    Y = yardstick(q, d)
    return Y, s, relative_error(T, Y, s)


@functools.lru_cache(maxsize=None)
def _tables(S, name):
    return power_table(generators(S)[name])


def device_tolerance(Y, s, e_ref):
    """|dev - Y| <= 8 max(e_ref, (2^s + 20) eps) Y + 2^s 1e-19, per entry"""
    return 8.0 * max(e_ref, (2.0 ** s + 20.0) * EPS) * np.asarray(Y, dtype=LD) + LD(floor(s))


# ---- the eigen route ---------------------------------------------------------------------------------------------------------------------
def eigen_route(q, d):
    """exp(Q d) as U exp(D d) U^-1 from inputs.substmodel.decompose_complex's real block form — what an EIGEN_COMPLEX instance is
    handed; q must be normalised already (decompose_complex normalises what it is given)."""
    e = substmodel.decompose_complex(q)[1]
    S = len(q)
    re, im = np.asarray(e.evals[:S]), np.asarray(e.evals[S:])
    X = np.zeros((S, S))
    k = 0
    while k < S:
        if im[k] == 0.0:
            X[k, k] = math.exp(re[k] * d)
            k += 1
            continue
        ea, c, sn = math.exp(re[k] * d), math.cos(im[k] * d), math.sin(im[k] * d)
        X[k, k], X[k, k + 1], X[k + 1, k], X[k + 1, k + 1] = ea * c, ea * sn, -ea * sn, ea * c
        k += 2
    return np.asarray(e.evec) @ X @ np.asarray(e.ievc)
