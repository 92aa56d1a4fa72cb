"""Node-height gradients and diagonal Hessians: the host side of the one-call device route
(include/beagle_mi355.h ``beagleMi355NodeHeightDerivatives``).

The reference's NodeHeightGradient / NodeHeightHessian traits
(src/dr/evomodel/treedatalikelihood/discrete/DiscreteTraitNodeHeightDelegate.java:63-200) read every post-order and every pre-order
partial and every branch matrix back and loop on the host.  Everything they read is resident after a gradient pass over
``gradient.BranchGradient``'s buffer plan, so this class runs that pass — post-order partials, root lnL, pre-order partials, the
rate-scaled infinitesimal matrix — and then asks the engine for both derivatives of every internal node in one call.  Branch
lengths are rate x height difference (a strict or relaxed clock: one rate per branch).
"""
import numpy as np

from . import beagle as _b
from .gradient import BranchGradient


class NodeHeightGradient(BranchGradient):
    """d lnL / d h_i and d^2 lnL / d h_i^2 for the internal nodes i of the workload's tree."""

    def __init__(self, workload, rates=None, **kwargs):
        """rates: one clock rate per node's branch (the root's entry is unused); default all 1."""
        super().__init__(workload, **kwargs)
        self.rates = np.ones(self.N) if rates is None else np.array(rates, dtype=float)
        if self.rates.shape != (self.N,):
            raise ValueError("rates must have one entry per node")
        self.heights = np.array(self.tree.height, dtype=float)
        self.internal = np.arange(self.T, self.N)
        self._apply_heights()

    def _apply_heights(self):
        tr = self.tree
        for n in self.edges:
            self.branch_lengths[n] = self.rates[n] * (self.heights[tr.parent[n]] - self.heights[n])

    def set_height(self, node, height):
        self.heights[node] = height
        self._apply_heights()

    def node_rows(self):
        """The call's two tables for the buffers of the current evaluation: rows {pre(i), post(j), matrix(j), dmatrix(j), post(k),
        matrix(k), dmatrix(k), dmatrix(i)} and {r_j, r_k, r_i}, one per internal node in node order."""
        tr, q, v = self.tree, self.q_index, self._set
        i = self.internal
        j, k = tr.left[i].astype(np.int64), tr.right[i].astype(np.int64)
        root = i == tr.root
        rows = np.empty((len(i), 8), dtype=np.int32)
        rows[:, 0] = self.pre_offset + i
        for col, child in ((1, j), (4, k)):
            rows[:, col] = np.where(child < self.T, child, child + v * self._partial_set)      # post_index, all rows at once
            rows[:, col + 1] = child + v * self._matrix_set                                     # matrix_index
            rows[:, col + 2] = q
        rows[:, 7] = np.where(root, -1, q)
        rates = np.stack([self.rates[j], self.rates[k], np.where(root, 0.0, self.rates[i])], axis=1)
        return rows, rates

    def prepare(self):
        """Everything the call reads, left on the device: -> lnL."""
        lnl = self.log_likelihood()
        self.b.setPartials(self.pre_offset + self.tree.root, self._root_pre)
        self.b.updatePrePartials(self._pre_ops, len(self._pre_ops) // 7, _b.NONE)
        self.b.setDifferentialMatrix(self.q_index, self.infinitesimal(1))
        return lnl

    def derivatives(self, second=True):
        """-> (lnL, first, second): arrays over the internal nodes in node order (node T + r at entry r); second is None when
        not asked for."""
        lnl = self.prepare()
        rows, rates = self.node_rows()
        first, sec = self.b.nodeHeightDerivatives(rows, rates, 0, first=True, second=second)
        return lnl, first, sec

    def first_from_branch_gradient(self, branch_gradient):
        """The chain rule of DiscreteTraitNodeHeightDelegate.java:69-85 over d lnL / d t per node (BranchGradient.gradient)."""
        tr = self.tree
        out = np.zeros(len(self.internal))
        for r, i in enumerate(self.internal):
            for child in (int(tr.left[i]), int(tr.right[i])):
                out[r] += branch_gradient[child] * self.rates[child]
            if i != tr.root:
                out[r] -= branch_gradient[i] * self.rates[i]
        return out
