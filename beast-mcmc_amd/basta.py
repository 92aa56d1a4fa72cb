"""BASTA, the structured-coalescent approximation, on the device: the caller's side of
``BeagleBastaLikelihoodDelegate`` (src/dr/evomodel/coalescent/basta/BeagleBastaLikelihoodDelegate.java) over the
``beagleBasta*`` calls of include/beagle_mi355.h.

``traverse`` restates ``CoalescentIntervalTraversal.traverseReverseCoalescentLevelOrder`` (CoalescentIntervalTraversal.java:
259-480): the tree's sampling and coalescent events in time order, every lineage alive in an interval pushed through that
interval's matrix (``sub_intervals`` matrices per interval), two lineages multiplied at a coalescence.  A lineage's vector
gets a new buffer with every step — ``offset * nodeCount + node``, the accumulation buffer of a coalescing child is
``nodeCount + node`` — and that sparse numbering is compacted to first-use order as the delegate's ``CACHE_FRIENDLY`` map
does (:452-507).  As in the reference, the matrix / interval number of an interval's first sub-interval is
``(sub-intervals so far) * sub_intervals``: with more than one sub-interval the numbers have gaps.

``BastaLikelihood.log_likelihood`` follows ``BastaLikelihood.calculateLogLikelihood`` (BastaLikelihood.java:479-526): eigen
system, population sizes, matrices, update, accumulate.  The decomposition it is given is used as it is: BASTA wants the
TRANSPOSED one (``updateEigenDecomposition``, :384-394) and ``transpose_eigen`` makes it.
"""
import numpy as np

from . import beagle as _beagle
from .inputs.substmodel import EigenDecomposition

OPERATION_SIZE = _beagle.BASTA_OPERATION_SIZE
COALESCENT_BUFFER_COUNT = 5              # probabilities, e, f, g, h
COALESCENT_PROBABILITY_INDEX = 0


def transpose_eigen(eigen):
    """The eigen system of Q^T from that of Q (EigenDecomposition.java:55-84): vectors and inverse vectors change places; in the
    real block form of a complex pair the second vector of the pair changes sign."""
    s = eigen.evec.shape[0]
    evec, ievc = eigen.ievc.T.copy(), eigen.evec.T.copy()
    if eigen.evals.shape[0] == 2 * s:
        i = 0
        while i < s:
            if eigen.evals[s + i] != 0.0:
                evec[:, i + 1] *= -1.0
                ievc[i + 1, :] *= -1.0
                i += 1
            i += 1
    return EigenDecomposition(evec, ievc, eigen.evals.copy())


class Traversal:
    """What one traversal yields: ``operations`` [n][8] (compacted buffer numbers), ``intervals`` (offsets, the last n),
    ``lengths`` per interval, ``matrices`` = [(matrix number, rate-scaled length)], ``buffer_count``, ``interval_count`` (largest
    interval number + 1), ``sparse`` = the operations before compaction."""


def traverse(tree, rate=1.0, sub_intervals=1):
    t, n_nodes, h = tree.tip_count, tree.node_count, tree.height
    order = sorted(range(n_nodes), key=lambda x: (h[x], x >= t, x))
    if order[0] >= t:
        raise ValueError("the most recent event is not a sampled tip")
    offset = [0] * n_nodes
    active = {order[0]: None}            # insertion-ordered, as the reference's LinkedHashSet
    ops, starts, lengths, matrices = [], [0], [], []
    state = {"interval": 0, "matrix": -1}

    def buffer(node):
        o = offset[node]
        return (o + 1 if o > 0 else 0) * n_nodes + node

    def matrix(sub, length):
        if sub != state["matrix"]:
            matrices.append((sub, rate * length))
            state["matrix"] = sub
        return sub

    def propagate(sub, node, length):
        in1 = buffer(node)
        offset[node] += 1
        out = buffer(node)
        ops.append((out, in1, matrix(sub, length), -1, -1, out, -1, sub))

    def close(length):
        state["interval"] += 1
        starts.append(len(ops))
        lengths.append(length)

    for k in range(1, n_nodes):
        node, length = order[k], float(h[order[k]] - h[order[k - 1]])
        if node < t:                     # a sampling event: a zero-length interval adds the tip and nothing else
            if length > 0.0:
                sub_length, sub = length / sub_intervals, state["interval"] * sub_intervals
                for _ in range(sub_intervals):
                    for a in active:
                        propagate(sub, a, sub_length)
                    sub += 1
                    close(sub_length)
            active[node] = None
            continue
        sub_length, sub = length / sub_intervals, state["interval"] * sub_intervals
        if sub_length <= 0.0:
            raise ValueError("a coalescence in no time")
        left, right = int(tree.left[node]), int(tree.right[node])
        for _ in range(sub_intervals - 1):
            for a in active:
                propagate(sub, a, sub_length)
            sub += 1
            close(sub_length)
        active[node] = None
        m = matrix(sub, sub_length)
        ops.append((buffer(node), buffer(left), m, buffer(right), m, n_nodes + left, n_nodes + right, sub))
        del active[left], active[right]
        for a in active:
            if a != node:
                propagate(sub, a, sub_length)
        close(sub_length)
    if order[-1] < t:
        raise ValueError("no coalescence at the top")

    out = Traversal()
    out.sparse = np.asarray(ops, dtype=np.int64).reshape(-1, OPERATION_SIZE)
    mapped, used = {}, t
    dense = out.sparse.copy()
    for row in dense:                    # first-use order: dest, in1, in2, acc1, acc2
        for col in (0, 1, 3, 5, 6):
            b = int(row[col])
            if b >= t:
                if b not in mapped:
                    mapped[b] = used
                    used += 1
                row[col] = mapped[b]
    out.operations = dense.astype(np.int32)
    out.intervals = np.asarray(starts, dtype=np.int32)
    out.lengths = np.asarray(lengths, dtype=np.float64)
    out.matrices = matrices
    out.buffer_count = used
    out.interval_count = int(out.operations[:, 7].max()) + 1
    return out


def interval_distances(traversal):
    """Per list interval, the rate-scaled length its matrix was formed with (``TransitionMatrixOperation.time``; 0 for an interval
    without operations)."""
    time = dict(traversal.matrices)
    ops, starts = traversal.operations, traversal.intervals
    return np.asarray([time[int(ops[starts[k], 2])] if starts[k + 1] > starts[k] else 0.0 for k in range(len(starts) - 1)])


def migration_rate_chain_rule(w, frequencies):
    """From the S x S intermediate to the rates parameter's order (StructuredCoalescentLikelihoodGradient.java:134-154): the upper
    triangle row by row, then the lower triangle column by column, each (W[i][j] - W[i][i]) pi_j."""
    w, pi = np.asarray(w), np.asarray(frequencies)
    s = w.shape[0]
    upper = [(w[i, j] - w[i, i]) * pi[j] for i in range(s) for j in range(i + 1, s)]
    lower = [(w[i, j] - w[i, i]) * pi[j] for j in range(s) for i in range(j + 1, s)]
    return np.asarray(upper + lower, dtype=w.dtype)


def population_size_chain_rule(theta_gradient, sizes):
    """d/dN from d/d(1/N) (StructuredCoalescentLikelihoodGradient.java:181-190)."""
    sizes = np.asarray(sizes)
    return np.asarray(theta_gradient) / -(sizes * sizes)


class BastaLikelihood:
    """The BASTA log-density of ``tree`` with the tips in ``tip_demes`` (a deme index per tip, or [T][S] vectors).

    ``eigen``: the (already transposed) decomposition of the migration-rate matrix, real (S eigenvalues) or in the real block
    form of an EIGEN_COMPLEX instance (2 S).  ``population_sizes``: one per deme."""

    def __init__(self, tree, tip_demes, eigen, population_sizes, rate=1.0, sub_intervals=1, library=None):
        self.tree, self.rate, self.sub_intervals = tree, float(rate), int(sub_intervals)
        self.sizes = np.asarray(population_sizes, dtype=np.float64).copy()
        self.state_count = s = self.sizes.shape[0]
        self.eigen = eigen
        demes = np.asarray(tip_demes)
        if demes.ndim == 1:
            self.tips = np.zeros((tree.tip_count, s))
            self.tips[np.arange(tree.tip_count), demes.astype(np.int64)] = 1.0
        else:
            self.tips = np.asarray(demes, dtype=np.float64).reshape(tree.tip_count, s).copy()
        # every matrix / interval number a traversal of a tree this size can produce
        self.max_intervals = tree.node_count * self.sub_intervals * self.sub_intervals + self.sub_intervals
        self.partials_count = 2 * tree.node_count
        self.beagle = _beagle.Beagle(0, self.partials_count, 0, s, 1, 2, self.max_intervals, 1, 1,
                                     requirementFlags=_beagle.FLAG_EIGEN_COMPLEX, library=library)
        self.beagle.setCategoryRates([1.0])
        self.beagle.allocateCoalescentBuffers(COALESCENT_BUFFER_COUNT, self.max_intervals, self.partials_count, 1)
        self.sizes_index = 0
        self.traversal = None
        self.resizes = 0
        for i in range(tree.tip_count):
            self.beagle.setPartials(i, self.tips[i])

    def close(self):
        if self.beagle is not None:
            self.beagle.finalize()
            self.beagle = None

    def make_dirty(self):
        self.traversal = None

    def set_node_height(self, node, height):
        self.tree.height[node] = height
        self.traversal = None

    def set_population_sizes(self, sizes, flip=False):
        """``flip``: the sizes go to the other of the two indices (the delegate's OffsetBufferIndexHelper)."""
        self.sizes = np.asarray(sizes, dtype=np.float64).copy()
        if flip:
            self.sizes_index = 1 - self.sizes_index

    def _eigen_arrays(self):
        s, lam = self.state_count, np.asarray(self.eigen.evals, dtype=np.float64)
        if lam.shape[0] == s:
            lam = np.concatenate([lam, np.zeros(s)])
        return self.eigen.evec, self.eigen.ievc, lam

    def log_likelihood(self, matrices=None):
        """One evaluation.  ``matrices`` ({matrix number: S x S array}): uploaded as they are instead of being computed from
        the eigen system."""
        b = self.beagle
        if self.traversal is None:
            self.traversal = traverse(self.tree, self.rate, self.sub_intervals)
        tr = self.traversal
        if matrices is None:
            b.setEigenDecomposition(0, *self._eigen_arrays())
        b.setStateFrequencies(self.sizes_index, self.sizes)
        if matrices is None:
            idx = [m for m, _ in tr.matrices]
            b.updateTransitionMatrices(0, idx, None, None, [length for _, length in tr.matrices], len(idx))
        else:
            for m, _ in tr.matrices:
                b.setTransitionMatrix(m, np.asarray(matrices[m], dtype=np.float64))
        if tr.buffer_count + 1 > self.partials_count:      # (BeagleBastaLikelihoodDelegate.resize)
            self.partials_count = tr.buffer_count + 2
            b.allocateCoalescentBuffers(COALESCENT_BUFFER_COUNT, self.max_intervals, self.partials_count, 0)
            self.resizes += 1
        n, m = tr.operations.shape[0], tr.intervals.shape[0]
        b.updateBastaPartials(tr.operations, n, tr.intervals, m, self.sizes_index, COALESCENT_PROBABILITY_INDEX)
        out = np.zeros(1)
        b.accumulateBastaPartials(tr.operations, n, tr.intervals, m, tr.lengths, self.sizes_index,
                                  COALESCENT_PROBABILITY_INDEX, out)
        return float(out[0])

    def sample_states(self, replicates=1, seed=0, map=False, as_written=False, states=True, occupancy=False, changes=False,
                      root_frequencies=None):
        """Demes of every lineage at every sub-interval boundary, ``replicates`` draws from the vectors and matrices of the last
        ``log_likelihood`` (``BastaLikelihood.traverseSampleByCoalescentIntervals``, BastaLikelihood.java:755-943; the rule is in
        include/beagle_mi355.h beagleBastaSampleStates).  ``root_frequencies``: the substitution model's frequencies (uniform by
        default); they go to the frequencies index the population sizes do not occupy.  ``as_written``: the matrix indexed as the
        reference's interval-by-interval route indexes it.  -> a dict of the arrays asked for: ``states`` uint8
        [replicates][partials_count] (255: a buffer the list does not touch), ``occupancy`` [intervals][S], ``changes`` [S][S];
        ``bad``: a draw met a total that is not finite and positive."""
        if self.traversal is None:
            raise ValueError("sample_states draws from the last evaluation: call log_likelihood first")
        tr, b = self.traversal, self.beagle
        f = np.full(self.state_count, 1.0 / self.state_count) if root_frequencies is None else np.asarray(root_frequencies, dtype=np.float64)
        b.setStateFrequencies(1 - self.sizes_index, f)
        flags = (1 if map else 0) | (b.BASTA_STATES_AS_WRITTEN if as_written else 0)
        return b.sampleBastaStates(tr.operations, tr.operations.shape[0], tr.intervals, tr.intervals.shape[0], 1 - self.sizes_index,
                                   replicates, seed, flags, states=states, occupancy=occupancy, changes=changes)

    def gradient(self, wrt="both", frequencies=None, adjoints=False):
        """The gradient of the last ``log_likelihood`` (include/beagle_mi355.h beagleBastaGradient; what
        ``StructuredCoalescentLikelihoodGradient`` returns for wrtParameter "migrationRate" / "populationSize").  ``wrt``:
        "migration", "population" or "both".  -> a dict of
          ``theta`` [S]            with respect to 1 / size (the reference's intermediate)
          ``population_sizes`` [S] = -theta / N^2 (StructuredCoalescentLikelihoodGradient.java:181-190)
          ``migration`` [S][S]     the intermediate W
          ``migration_rates`` [S (S - 1)], with ``frequencies``: ``migration_rate_chain_rule(W, frequencies)``
          ``adjoints`` [partials_count][S], when asked for;   ``bad``: a value is not finite."""
        if wrt not in ("both", "migration", "population"):
            raise ValueError("wrt: 'migration', 'population' or 'both'")
        if self.traversal is None:
            raise ValueError("gradient differentiates the last evaluation: call log_likelihood first")
        tr, b = self.traversal, self.beagle
        migration, population = wrt != "population", wrt != "migration"
        out = b.bastaGradient(tr.operations, tr.operations.shape[0], tr.intervals, tr.intervals.shape[0], tr.lengths,
                              interval_distances(tr) if migration else None, self.sizes_index, COALESCENT_PROBABILITY_INDEX,
                              population_sizes=population, migration=migration, adjoints=adjoints)
        if population:
            out["population_sizes"] = population_size_chain_rule(out["theta"], self.sizes)
        if migration and frequencies is not None:
            out["migration_rates"] = migration_rate_chain_rule(out["migration"], frequencies)
        return out

    def partials(self, buffer):
        return self.beagle.getPartials(buffer).reshape(self.state_count)

    def coalescent_probabilities(self):
        return self.beagle.getBastaBuffer(COALESCENT_PROBABILITY_INDEX)

    def transition_matrix(self, index):
        return self.beagle.getTransitionMatrix(index).reshape(self.state_count, self.state_count)
