"""Ancestral-state draws on the device: the caller-side mirror of
``dr.evomodel.treelikelihood.AncestralStateBeagleTreeLikelihood`` (src/dr/evomodel/treelikelihood/AncestralStateBeagleTreeLikelihood.java).

The reference walks the tree top-down and reads a ``getPartials`` per internal node and a ``getTransitionMatrix`` per branch
before it draws in Java (``traverseSample``, :414-625).  Here the whole draw is ONE engine call
(include/beagle_mi355.h ``beagleMi355SampleAncestralStates``): this class only turns the tree and the caller's current buffer
and matrix indices (which follow its double buffering) into the pre-order node list, and hands the states back per tree node.

The partials must be current: sample after ``getLogLikelihood``, as the reference does (its states are redrawn from the
partials of the last evaluation).
"""
import numpy as np

from . import beagle as _b


class AncestralStateSampler:
    """Draws every node's state per site for a ``treelikelihood.BeagleTreeLikelihood`` (the C++ caller stand-in)."""

    def __init__(self, tree_likelihood):
        self.tl = tree_likelihood
        self.beagle = _b.Beagle.attach(tree_likelihood)

    def preorder(self):
        """Tree nodes in the order traverseSample visits them: a node, then its first child's subtree, then its second's."""
        tree = self.tl.tree
        order, stack = [], [tree.root]
        while stack:
            n = stack.pop()
            order.append(n)
            if n >= tree.tip_count:
                stack.append(int(tree.right[n]))
                stack.append(int(tree.left[n]))
        return order

    def node_list(self):
        """-> (rows int32 [node_count, 3] = {bufferIndex, matrixIndex, parentRow}, tree node of each row)."""
        tree, tl = self.tl.tree, self.tl
        order = self.preorder()
        row_of = np.full(tree.node_count, -1, dtype=np.int64)
        rows = np.zeros((len(order), 3), dtype=np.int32)
        for r, n in enumerate(order):
            row_of[n] = r
            parent = int(tree.parent[n])
            rows[r, 0] = tl.node_buffer_index(n)
            rows[r, 1] = 0 if parent < 0 else tl.node_matrix_index(n)
            rows[r, 2] = -1 if parent < 0 else row_of[parent]
        return rows, np.asarray(order, dtype=np.int64)

    def sample(self, seed, map=False, category_weights_index=0, state_frequencies_index=0):
        """-> (states uint8 [node_count, P] indexed by tree node number, tips included — getStatesForNode's rows;
        rate categories int32 [P]).  ``map``: the argmax of every conditional instead of a draw (useMAP)."""
        rows, order = self.node_list()
        drawn, cats = self.beagle.sampleAncestralStates(rows, category_weights_index, state_frequencies_index, seed, map=map)
        states = np.empty_like(drawn)
        states[order] = drawn
        return states, cats
