"""Sequence simulation on the device: the caller-side mirror of ``dr.app.beagle.tools.BeagleSequenceSimulator`` / ``Partition``
(src/dr/app/beagle/tools/Partition.java).

The reference walks the tree top-down, reads a ``getTransitionMatrix`` per branch and draws every site in Java
(``traverse``, :292-387; ``randomChoicePDF``, :519-536).  Here a replicate is ONE engine call (include/beagle_mi355.h
``beagleMi355SimulateSequences``): this class only turns the tree and the caller's current matrix indices (which follow its double
buffering) into the pre-order node list, and hands the states back per tree node.

The branch matrices must be current — simulate after ``getLogLikelihood``, or after any call sequence that has run
``updateTransitionMatrices`` for every branch; partials are never read.
"""
import numpy as np

from . import beagle as _b
from .ancestral import AncestralStateSampler
from .inputs import patterns as _patterns


class SequenceSimulator:
    """Draws alignments from the model of a ``treelikelihood.BeagleTreeLikelihood`` (the C++ caller stand-in)."""

    def __init__(self, tree_likelihood):
        self.tl = tree_likelihood
        self.beagle = _b.Beagle.attach(tree_likelihood)

    def node_list(self, ancestral=False):
        """-> (rows int32 [node_count, 3] = {outRow, matrixIndex, parentRow}, tree node of each row).  outRow: the tree node's number
        (tips first, so tip t is output row t), or -1 for an internal node when ``ancestral`` is false."""
        tree, tl = self.tl.tree, self.tl
        order = AncestralStateSampler.preorder(self)          # (the same walk: a node, its first child's subtree, its second's)
        row_of = np.full(tree.node_count, -1, dtype=np.int64)
        rows = np.zeros((len(order), 3), dtype=np.int32)
        for r, n in enumerate(order):
            row_of[n] = r
            parent = int(tree.parent[n])
            rows[r, 0] = n if (ancestral or n < tree.tip_count) else -1
            rows[r, 1] = 0 if parent < 0 else tl.node_matrix_index(n)
            rows[r, 2] = -1 if parent < 0 else row_of[parent]
        return rows, np.asarray(order, dtype=np.int64)

    def simulate(self, site_count, seed, ancestral=False, root_states=None, rate_categories=None, category_weights_index=0,
                 state_frequencies_index=0):
        """-> (tip states uint8 [tip_count, site_count] by tip number, internal states uint8 [node_count - tip_count, site_count] by
        node number - tip_count or None, rate categories int32 [site_count]).  ``root_states``: the root's sequence instead of a draw
        from the frequencies (setRootSequence); ``rate_categories``: the sites' categories instead of a draw from the weights."""
        rows, _ = self.node_list(ancestral)
        states, cats = self.beagle.simulateSequences(rows, site_count, category_weights_index, state_frequencies_index, seed,
                                                     root_states=root_states, rate_categories=rate_categories)
        t = self.tl.tree.tip_count
        return states[:t], (states[t:] if ancestral else None), cats

    @staticmethod
    def to_patterns(states):
        """A simulated alignment ([taxa][sites]) -> (unique patterns int32 [taxa][P], weights [P]): what a new
        ``BeagleTreeLikelihood`` takes as tip states and pattern weights — one step of a parametric bootstrap."""
        return _patterns.site_patterns(np.asarray(states, dtype=np.int32), unique=True)
