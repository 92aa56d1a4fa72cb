"""Host restatement of the multidimensional-scaling likelihood, in numpy: what tests/test_mds_host.py and tests/test_gpu_mds.py
hold libmds2_jni.so to.

`Core` restates MultiDimensionalScalingCoreImpl (src/dr/inference/multidimensionalscaling/MultiDimensionalScalingCoreImpl.java of
the reference tree), state machine included:
  * the N x N table of increments, filled for every (i, j) and summed in index order, the sum halved (:239-269);
  * the incremental path after exactly one single-location update: row k only, delta = sum_j (new - old) in index order, the old
    row kept for a restore (:271-302), the column made equal to the row on accept (:214-221);
  * updateLocation / setParameters / makeDirty / storeState / restoreState and their flags (:111-151, :176-212, :233-237);
  * the distance summed over the dimensions in index order (:304-311), the truncation term log Phi(d sqrt(tau)) off the diagonal
    only (:252-258, :313-315).
Two things are NOT the Java core's and follow include/mds_mi355.h: a NaN observation is a missing pair and contributes nothing
(the Java core would carry the NaN into the sum), and `sum_of_increments()` returns S with tau applied in both modes, which is
what MassivelyParallelMDSImpl.calculateLogLikelihood subtracts (MassivelyParallelMDSImpl.java:122-127); the untruncated Java
core keeps sum (d - y)^2 and scales on the way out (:165-171), and so does this class.

`dtype` is the type of every distance, residual, increment and sum (numpy.longdouble for the wide run).  log Phi itself is
evaluated in fp64 (scipy.special.log_ndtr) in either run: the wide run measures the rounding of the sums, not of that function.

`gradient` is the formula of the header; the Java core has none (getGradient throws, :223-226).
"""
import math

import numpy as np
from scipy.special import log_ndtr

LEFT_TRUNCATION = 32


def _distances(a, b, dtype):
    """|a_i - b_j| for a [n][D] against b [m][D], the squares added in the order of the dimensions."""
    s = np.zeros((a.shape[0], b.shape[0]), dtype=dtype)
    for c in range(a.shape[1]):
        t = a[:, c][:, None] - b[:, c][None, :]
        s += t * t
    return np.sqrt(s)


def _log_phi(z, dtype):
    return log_ndtr(np.asarray(z, dtype=np.float64)).astype(dtype)


def _ordered_sum(values):
    """The sum in index order (numpy.sum adds pairwise)."""
    flat = np.asarray(values).reshape(-1)
    return flat.dtype.type(0) if flat.size == 0 else np.cumsum(flat)[-1]


class Core:
    def __init__(self, dimension, location_count, flags=0, dtype=np.float64):
        self.d, self.n, self.dtype = dimension, location_count, dtype
        self.truncated = (flags & LEFT_TRUNCATION) != 0
        self.observations = np.zeros((self.n, self.n), dtype=dtype)
        self.increments = np.zeros((self.n, self.n), dtype=dtype)
        self.stored_increments = None
        self.increments_known = self.sum_known = False
        self.updated = -1
        self.locations = np.zeros((self.n, self.d), dtype=dtype)
        self.stored_locations = np.zeros((self.n, self.d), dtype=dtype)
        self.precision = self.stored_precision = dtype(0)
        self.sum = self.stored_sum = dtype(0)
        self.paths = []                          # "all" / "row" per evaluation that was made

    # -- the interface of MultiDimensionalScalingCore ------------------------------------------------------------
    def set_pairwise_data(self, observations):
        y = np.asarray(observations, dtype=np.float64).reshape(self.n, self.n)
        self.observations = y.astype(self.dtype)

    def set_parameters(self, parameters):
        self.precision = self.dtype(parameters[0])
        if self.truncated:
            self.increments_known = self.sum_known = False

    def update_location(self, index, location):
        if self.updated != -1 or index == -1:
            self.increments_known = False
            self.stored_increments = None
        if index != -1:
            self.updated = index
            self.locations[index] = np.asarray(location, dtype=np.float64).reshape(self.d).astype(self.dtype)
        else:
            self.locations = np.asarray(location, dtype=np.float64).reshape(self.n, self.d).astype(self.dtype)
        self.sum_known = False

    def store_state(self):
        self.stored_sum = self.sum
        self.stored_increments = None
        self.stored_locations = self.locations.copy()
        self.updated = -1
        self.stored_precision = self.precision

    def restore_state(self):
        self.sum = self.stored_sum
        self.sum_known = True
        if self.stored_increments is not None:
            self.increments[self.updated] = self.stored_increments
            self.increments_known = True
        else:
            self.increments_known = False
        self.locations, self.stored_locations = self.stored_locations, self.locations
        self.precision = self.stored_precision

    def accept_state(self):
        if self.stored_increments is not None:
            self.increments[:, self.updated] = self.increments[self.updated]

    def make_dirty(self):
        self.sum_known = self.increments_known = False

    # -- the arithmetic --------------------------------------------------------------------------------------------
    def _row_increments(self, rows):
        """increments[i][j] for i in rows, every j."""
        x = self.locations
        dist = _distances(x[rows], x, self.dtype)
        y = self.observations[rows]
        residual = dist - y
        inc = residual * residual
        if self.truncated:
            inc = (self.dtype(0.5) * self.precision) * inc
            off = np.ones_like(inc, dtype=bool)
            off[np.arange(len(rows)), rows] = False
            inc = inc + np.where(off, _log_phi(dist * np.sqrt(self.precision), self.dtype), self.dtype(0))
        return np.where(np.isnan(y), self.dtype(0), inc)

    def _evaluate(self):
        if self.sum_known:
            return
        if not self.increments_known:
            total = self.dtype(0)
            for start in range(0, self.n, 256):                  # row blocks: the same index order, bounded memory
                rows = np.arange(start, min(self.n, start + 256))
                block = self._row_increments(rows)
                self.increments[rows] = block
                total = np.cumsum(np.concatenate(([total], block.reshape(-1))))[-1]
            self.sum = total / self.dtype(2)
            self.increments_known = True
            self.paths.append("all")
        else:
            i = self.updated
            self.stored_increments = self.increments[i].copy()
            new = self._row_increments(np.array([i]))[0]
            self.sum = self.sum + _ordered_sum(new - self.increments[i])
            self.increments[i] = new
            self.paths.append("row")
        self.sum_known = True

    def sum_of_increments(self):
        """S of the header: tau applied in both modes."""
        self._evaluate()
        return self.sum if self.truncated else self.dtype(0.5) * self.precision * self.sum

    def absolute_sum(self):
        """sum_{i<j} |increment(i,j)| at the current locations and tau, computed afresh: the scale of S's rounding error."""
        total = self.dtype(0)
        for start in range(0, self.n, 256):
            rows = np.arange(start, min(self.n, start + 256))
            block = np.abs(self._row_increments(rows))
            if not self.truncated:
                block = self.dtype(0.5) * self.precision * block
            total += block.sum()
        return total / self.dtype(2)

    def observation_count(self):
        y = self.observations
        return int(np.count_nonzero(~np.isnan(y[np.triu_indices(self.n, 1)])))

    def log_likelihood(self, count=None):
        """MassivelyParallelMDSImpl.calculateLogLikelihood (:122-127) with n = the pairs that are not missing."""
        count = self.observation_count() if count is None else count
        tau = self.precision
        return self.dtype(0.5) * (np.log(tau) - self.dtype(math.log(2.0 * math.pi))) * count - self.sum_of_increments()

    def gradient(self):
        """(g, scale): g[i][c] = dlogL/dx_ic by the header's formula, each row's terms added in the order of j; scale[i][c] =
        sum_j |term_ijc|, what an error bound on g[i][c] has to be relative to (a row's terms cancel)."""
        x, tau, dt = self.locations, self.precision, self.dtype
        g, scale = np.zeros((self.n, self.d), dtype=dt), np.zeros((self.n, self.d), dtype=dt)
        for start in range(0, self.n, 256):
            rows = np.arange(start, min(self.n, start + 256))
            dist = _distances(x[rows], x, dt)
            y = self.observations[rows]
            coef = tau * (dist - y)
            if self.truncated:
                z = np.asarray(dist * np.sqrt(tau), dtype=np.float64)
                coef = coef + np.sqrt(tau) * np.exp(-0.5 * z * z - log_ndtr(z) - 0.5 * math.log(2.0 * math.pi)).astype(dt)
            use = ~np.isnan(y) & (dist > 0)
            use[np.arange(len(rows)), rows] = False
            with np.errstate(divide="ignore", invalid="ignore"):
                coef = np.where(use, coef / dist, dt(0))
            for c in range(self.d):
                terms = -coef * (x[rows, c][:, None] - x[:, c][None, :])
                g[rows, c] = np.cumsum(terms, axis=1)[:, -1]
                scale[rows, c] = np.abs(terms).sum(axis=1)
        return g, scale


def synthetic(n, d, seed, missing=0.05, sigma=0.3, spread=2.0):
    """The test inputs: locations N(0, spread^2), observations |true distance + N(0, sigma^2)| symmetrised, a zero diagonal, the
    given share of the pairs NaN (both halves)."""
    rng = np.random.default_rng(seed)
    x = rng.normal(0.0, spread, size=(n, d))
    dist = _distances(x, x, np.float64)
    noise = np.triu(rng.normal(0.0, sigma, size=(n, n)), 1)
    y = np.abs(dist + noise + noise.T)
    if missing > 0.0:
        gone = np.triu(rng.random((n, n)) < missing, 1)
        y[gone | gone.T] = np.nan
    np.fill_diagonal(y, 0.0)
    return x, y
