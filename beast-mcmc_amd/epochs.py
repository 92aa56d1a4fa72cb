"""Branch matrices of epoch models: the caller's side of the reference's EpochBranchModel (branchmodel/EpochBranchModel.java) and of
what SubstitutionModelDelegate does for a branch model that ``requiresMatrixConvolution``
(treelikelihood/SubstitutionModelDelegate.java:162-405, repeated in treedatalikelihood/SubstitutionModelDelegate.java:213-288), over the
``beagle.Beagle`` method set.

An epoch model has ``model_count`` substitution models and ``model_count - 1`` transition times; model k holds between time k - 1 and
time k (heights, growing towards the root).  A branch that crosses boundaries gets the product of its segments' transition matrices,
root end first.

``route="host"`` is the reference's protocol, restated call for call: every segment of such a branch takes a buffer from a pool of
``pool_size`` extra matrix buffers, one ``updateTransitionMatrices`` per eigen system fills them, rounds of
``convolveTransitionMatrices`` fold them — with the early flush when the pool has fewer free buffers than the next branch needs, the
flush in the middle of a round, and the reserve buffer.  It is the only route a library without the extension offers (the CPU oracle),
the comparator of the tests and the baseline of tools/epoch_matrices_bench.py.  ``route="device"`` names every branch's segments in ONE
call (``Beagle.updateTransitionMatricesWithEpochs``, include/beagle_mi355.h beagleMi355UpdateTransitionMatricesWithEpochs): no pool
buffer, no intermediate matrix in memory.
"""
from collections import deque

import numpy as np

SYMBOL = "beagleMi355UpdateTransitionMatricesWithEpochs"
POOL_SIZE_DEFAULT = 100                                  # SubstitutionModelDelegate.BUFFER_POOL_SIZE_DEFAULT


class EpochBranchModel:
    """``transition_times`` [model_count - 1], ascending heights."""

    def __init__(self, transition_times, model_count):
        self.transition_times = [float(t) for t in np.asarray(transition_times, dtype=np.float64).reshape(-1)]
        self.model_count = int(model_count)
        if self.model_count != len(self.transition_times) + 1:
            raise ValueError("an epoch model has one more model than transition times")

    def mapping(self, node_height, parent_height):
        """-> (order, weights): the models the branch passes through, root end first, and the time it spends in each
        (EpochBranchModel.getBranchModelMapping, :74-127, loop for loop: a height ON a boundary belongs to the epoch above it)."""
        epoch_count = self.model_count - 1
        times = self.transition_times
        weight_list, order_list = [], []
        # find the epoch that the node height is in...
        epoch = 0
        while epoch < epoch_count and node_height >= times[epoch]:
            epoch += 1
        current = node_height
        # find the epoch that the parent height is in...
        while epoch < epoch_count and parent_height >= times[epoch]:
            weight_list.append(times[epoch] - current)
            order_list.append(epoch)
            current = times[epoch]
            epoch += 1
        weight_list.append(parent_height - current)
        order_list.append(epoch)
        return order_list[::-1], weight_list[::-1]


class EpochTransitionMatrices:
    """The branch matrices of ``tree`` (anything with ``height`` and ``parent`` arrays) under ``branch_model``.

    Branch b's matrix goes to slot ``matrix_index(b)`` (default: b itself) and model k's eigen system is in eigen slot ``eigen_index(k)``
    (default: k) — what matrixBufferHelper / eigenBufferHelper.getOffsetIndex answer.  The host route's pool is the ``pool_size`` slots
    from ``matrix_buffer_count`` on, the reserve buffer the one behind them: an instance for the host route needs
    ``matrix_count`` matrix buffers, one for the device route only ``matrix_buffer_count``.  ``category_rate_index``: the rate set of
    every branch (0: the stock ``updateTransitionMatrices``; another one: ``updateTransitionMatricesWithMultipleModels``)."""

    def __init__(self, branch_model, tree, matrix_buffer_count, pool_size=POOL_SIZE_DEFAULT, matrix_index=None, eigen_index=None,
                 category_rate_index=0):
        self.model, self.tree = branch_model, tree
        self.eigen_count = branch_model.model_count
        self.matrix_buffer_count = int(matrix_buffer_count)
        self.pool_size = int(pool_size) if pool_size > 0 else POOL_SIZE_DEFAULT
        if self.pool_size < self.eigen_count:
            raise ValueError("at least %d extra buffers to convolve matrices" % self.eigen_count)
        self.reserve = self.matrix_buffer_count + self.pool_size
        self.available = deque()
        for i in range(self.pool_size):
            self.available.appendleft(i + self.matrix_buffer_count)       # (pushAvailableBuffer: a stack)
        self.matrix_index = matrix_index or (lambda b: int(b))
        self.eigen_index = eigen_index or (lambda k: int(k))
        self.rate_index = int(category_rate_index)
        self.native_calls = 0                            # natives the last update issued
        self.flushes = {"early": 0, "mid_round": 0, "reserve": 0}      # ... and the flushes of each kind it went through (host route)
        self.log = None                                  # a list: the host route appends ("update", eigen slot, slots, lengths) / ("convolve", first, second, result)

    @property
    def matrix_count(self):
        """Matrix buffers of an instance the host route runs on (plus one for the reserve buffer)."""
        return self.matrix_buffer_count + self.pool_size + 1

    def branch_mapping(self, branch):
        return self.model.mapping(float(self.tree.height[branch]), float(self.tree.height[self.tree.parent[branch]]))

    def update(self, beagle, branch_indices, edge_lengths, route="device"):
        """The matrices of the listed branches (``edge_lengths``: rate x time of each, as updateTransitionMatrices takes them)."""
        if route not in ("device", "host"):
            raise ValueError("route is 'device' or 'host'")
        branches = [int(b) for b in np.asarray(branch_indices).reshape(-1)]
        lengths = [float(t) for t in np.asarray(edge_lengths, dtype=np.float64).reshape(-1)]
        if len(branches) != len(lengths):
            raise ValueError("one length per branch")
        self.native_calls = 0
        self.flushes = {"early": 0, "mid_round": 0, "reserve": 0}
        if route == "device":
            if not hasattr(beagle.lib.lib, SYMBOL):
                raise ValueError("this library forms no epoch products: route='host'")
            self._update_device(beagle, branches, lengths)
        else:
            self._update_host(beagle, branches, lengths)

    # -- one call ------------------------------------------------------------------------------------------------------------------
    def segments(self, branches, lengths):
        """-> (offsets [n + 1], eigen slot per segment, length per segment), int32 / int32 / float64 arrays: ``mapping`` for every listed
        branch at once.  The segment lengths are (weights[j] * edgeLength) / sum with sum accumulated from 0.0 in the order of the
        weights, the Java expression's evaluation order (:183-186, :212); a branch inside one epoch keeps its edge length as it is
        (:176-180).  Vectorised over the branches — the epoch of a height is the number of transition times <= it, which is what
        ``mapping``'s two loops count — with every float operation the one ``mapping`` and the host route perform, so the values are
        theirs to the bit (tests/test_epoch_matrices_host.py)."""
        times = np.asarray(self.model.transition_times, dtype=np.float64)
        if times.size > 1 and np.any(np.diff(times) < 0.0):
            raise ValueError("transition times must ascend")
        b = np.asarray(branches, dtype=np.int64).reshape(-1)
        t = np.asarray(lengths, dtype=np.float64).reshape(-1)
        height = np.asarray(self.tree.height, dtype=np.float64)
        hn, hp = height[b], height[np.asarray(self.tree.parent)[b]]
        en = np.searchsorted(times, hn, side="right")
        ep = np.maximum(np.searchsorted(times, hp, side="right"), en)
        n = ep - en + 1
        width = int(n.max()) if n.size else 0
        padded = np.concatenate([times, [0.0]])                     # (an index past the last boundary is never used where it counts)
        weights = np.zeros((b.size, width))
        epochs_ = np.zeros((b.size, width), dtype=np.int64)
        for j in range(width):                                      # j = 0: the root end
            i = n - 1 - j                                           # ... counted from the node end
            valid = i >= 0
            k = np.where(valid, en + i, 0)
            upper = np.where(j == 0, hp, padded[np.clip(k, 0, times.size)])
            lower = np.where(i == 0, hn, padded[np.clip(k - 1, 0, times.size)])
            weights[:, j] = np.where(valid, upper - lower, 0.0)
            epochs_[:, j] = k
        total = np.zeros(b.size)
        for j in range(width):
            total = np.where(j < n, total + weights[:, j], total)
        crossing = n > 1
        with np.errstate(divide="ignore", invalid="ignore"):
            seg = np.where(crossing[:, None], weights * t[:, None] / total[:, None], t[:, None])
        keep = np.arange(width)[None, :] < n[:, None]
        lut = np.asarray([self.eigen_index(k) for k in range(self.model.model_count)], dtype=np.int32)
        offsets = np.concatenate([[0], np.cumsum(n)]).astype(np.int32)
        return offsets, lut[epochs_[keep]], seg[keep]

    def _update_device(self, beagle, branches, lengths):
        if not branches:
            return
        offsets, eig, seg = self.segments(branches, lengths)
        slots = np.asarray([self.matrix_index(b) for b in branches], dtype=np.int32)
        rates = None if self.rate_index == 0 else np.full(len(branches), self.rate_index, dtype=np.int32)
        beagle.updateTransitionMatricesWithEpochs(offsets, eig, seg, rates, slots)
        self.native_calls = 1

    # -- the reference's protocol ------------------------------------------------------------------------------------------------------
    def _pop_available(self):
        return self.available.popleft() if self.available else -1

    def _update_host(self, beagle, branches, lengths):
        """updateTransitionMatrices, :162-232"""
        K = self.eigen_count
        probability_indices = [[] for _ in range(K)]
        edge_lengths = [[] for _ in range(K)]
        convolution_list = []
        for b, t in zip(branches, lengths):
            order, weights = self.branch_mapping(b)
            if len(order) == 1:
                k = order[0]
                probability_indices[k].append(self.matrix_index(b))
                edge_lengths[k].append(t)
            else:
                total = 0.0
                for w in weights:
                    total += w
                if len(self.available) < len(order):
                    # too few buffers available, process what we have and continue...
                    self.flushes["early"] += 1
                    self._compute(beagle, probability_indices, edge_lengths)
                    self._convolve(beagle, convolution_list)
                    probability_indices = [[] for _ in range(K)]
                    edge_lengths = [[] for _ in range(K)]
                buffer_indices = deque()
                for j, k in enumerate(order):
                    buffer = self._pop_available()
                    if buffer < 0:
                        raise RuntimeError("Ran out of buffers for transition matrices - computing current list.")
                    probability_indices[k].append(buffer)
                    edge_lengths[k].append(weights[j] * t / total)
                    buffer_indices.append(buffer)
                buffer_indices.append(self.matrix_index(b))
                convolution_list.append(buffer_indices)
        self._compute(beagle, probability_indices, edge_lengths)
        self._convolve(beagle, convolution_list)

    def _compute(self, beagle, probability_indices, edge_lengths):
        """computeTransitionMatrices, :234-272"""
        for k in range(self.eigen_count):
            n = len(probability_indices[k])
            if n > 0:
                e = self.eigen_index(k)
                if self.rate_index == 0:
                    beagle.updateTransitionMatrices(e, probability_indices[k], None, None, edge_lengths[k], n)
                else:
                    beagle.updateTransitionMatricesWithMultipleModels([e] * n, [self.rate_index] * n, probability_indices[k], None, None,
                                                                      edge_lengths[k], n)
                self.native_calls += 1
                if self.log is not None:
                    self.log.append(("update", e, list(probability_indices[k]), list(edge_lengths[k])))

    def _convolve(self, beagle, convolution_list):
        """convolveMatrices, :274-378.  A deque's front is its next operand: pop / push work there, add at the other end."""
        while len(convolution_list) > 0:
            first, second, result = [], [], []
            for convolve in convolution_list:
                if len(convolve) > 3:
                    f, s = convolve.popleft(), convolve.popleft()
                    while True:
                        buffer = self._pop_available()
                        if buffer >= 0:
                            break
                        # we have run out of buffers, process what we have and continue...
                        if len(first) > 0:
                            self.flushes["mid_round"] += 1
                            self._convolve_and_release(beagle, first, second, result)
                            first, second, result = [], [], []
                            # there should be enough spare buffers to get a result buffer for this operation now
                        else:
                            # only one partially set up operation, so there would be none to free up: the reserve buffer
                            self.flushes["reserve"] += 1
                            self._convolve_and_release(beagle, [f], [s], [self.reserve])
                            convolve.appendleft(self.reserve)
                            break
                    if buffer >= 0:
                        first.append(f); second.append(s); result.append(buffer)
                        convolve.appendleft(buffer)
                elif len(convolve) == 3:
                    first.append(convolve.popleft()); second.append(convolve.popleft()); result.append(convolve.popleft())
                else:
                    raise RuntimeError("Unexpected convolve list size")
            self._convolve_and_release(beagle, first, second, result)
            convolution_list[:] = [c for c in convolution_list if len(c) > 0]

    def _convolve_and_release(self, beagle, first, second, result):
        """convolveAndRelease, :380-405 (a round whose every operation went through the reserve buffer has none left to issue)"""
        if len(first) == 0:
            return
        beagle.convolveTransitionMatrices(first, second, result, len(first))
        self.native_calls += 1
        if self.log is not None:
            self.log.append(("convolve", list(first), list(second), list(result)))
        for f, s in zip(first, second):
            if f >= self.matrix_buffer_count and f != self.reserve:
                self.available.appendleft(f)
            if s >= self.matrix_buffer_count and s != self.reserve:
                self.available.appendleft(s)
