"""Complete substitution histories on the device: the caller-side mirror of ``dr.app.beagle.tools.CompleteHistorySimulator``
(src/dr/app/beagle/tools/CompleteHistorySimulator.java).

The reference walks the tree top-down and, per branch and site, runs ``StateHistory.simulateUnconditionalOnEndingState`` from the
parent's realised state (``traverse`` / ``simulateAlongBranch``, :420-496), keeps the history's ending state as the child's and the
realised value of every registered jump process (``processHistory``, :460-476).  Here a simulant is ONE engine call
(include/beagle_mi355.h ``beagleMi355SimulateCompleteHistories``): this class turns the tree into the pre-order node list, the
branch lengths and heights, keeps the registers and the generators, and hands the results back per tree node.

The call reads the instance's category rates, category weights and state frequencies only: built from a tree likelihood, simulate
after ``getLogLikelihood`` (the driver has set the model arrays by then); built with ``from_model``, the class owns a small instance
that only ever has its model setters called.  ``scaleByTime`` is not a parameter of ``add_register``: the reference parses it and
ignores it (CompleteHistorySimulator.java:286).
"""
import numpy as np

from . import beagle as _b
from .markovjumps import JUMPS_REWARDS


class _TreeOnly:
    """What ``from_model`` keeps in place of a tree likelihood: the tree, unit branch rates, the heights as given."""

    def __init__(self, tree, state_count, branch_rates=None):
        self.tree, self.state_count = tree, int(state_count)
        self.branch_rates = None if branch_rates is None else np.asarray(branch_rates, dtype=np.float64)

    def node_branch_time(self, node):
        p = int(self.tree.parent[node])
        rate = 1.0 if self.branch_rates is None else float(self.branch_rates[node])
        return float(self.tree.height[p] - self.tree.height[node]), rate

    def node_height(self, node):
        return float(self.tree.height[node])


class CompleteHistorySimulator:
    """Complete histories under the model of a ``treelikelihood.BeagleTreeLikelihood`` (the C++ caller stand-in), or of a tree, a
    site model and a substitution model (``from_model``)."""

    def __init__(self, tree_likelihood, infinitesimal_matrix=None):
        self.tl = tree_likelihood
        self.beagle = _b.Beagle.attach(tree_likelihood)
        self._owned = None
        eig = tree_likelihood.eig
        Q = (eig.evec * eig.evals[None, :]) @ eig.ievc if infinitesimal_matrix is None else infinitesimal_matrix
        self._init_model(Q)

    @classmethod
    def from_model(cls, tree, cat_rates, cat_weights, freqs, infinitesimal_matrix, branch_rates=None, library=None):
        """A simulator of its own: ``tree`` (inputs.trees.Tree), the site model's category rates and weights, the substitution
        model's frequencies and generator Q [S][S]; ``branch_rates`` per tree node (default 1)."""
        self = cls.__new__(cls)
        freqs = np.asarray(freqs, dtype=np.float64)
        S, C = len(freqs), len(cat_rates)
        self.tl = _TreeOnly(tree, S, branch_rates)
        self.beagle = self._owned = _b.Beagle(tree.tip_count, tree.node_count, tree.tip_count, S, 16, 1, 1, C, 0, library=library)
        self.beagle.setStateFrequencies(0, freqs)
        self.beagle.setCategoryRates(cat_rates)
        self.beagle.setCategoryWeights(0, cat_weights)
        self._init_model(infinitesimal_matrix)
        return self

    def _init_model(self, Q):
        S = self.tl.state_count
        self.generators = [np.array(Q, dtype=np.float64).reshape(S, S)]
        self.branch_generator = None
        self.tags, self.kinds, self.registers = [], [], []

    def close(self):
        if self._owned is not None:
            self._owned.finalize()
            self._owned = None

    def add_register(self, tag, values, kind="counts"):
        """``values``: an S x S registration matrix for counts (COUNTS; its diagonal is never reached by a jump), an S-vector of
        rewards (REWARDS).  Returns the register's index k."""
        S = self.tl.state_count
        if kind == "counts":
            R = np.array(values, dtype=np.float64).reshape(S, S)
        elif kind == "rewards":
            R = np.diag(np.asarray(values, dtype=np.float64).reshape(S))
        else:
            raise ValueError("kind must be 'counts' or 'rewards'")
        if len(self.registers) >= 8:
            raise ValueError("at most 8 registers")
        self.tags.append(tag)
        self.kinds.append(kind)
        self.registers.append(R)
        return len(self.registers) - 1

    def set_branch_generators(self, generators, generator_of_node):
        """branchSpecificLambda: ``generators`` [qCount][S][S], one per distinct branch value, and for every tree node the index of
        the generator its branch evolves under (the root's entry is ignored)."""
        S = self.tl.state_count
        self.generators = [np.array(q, dtype=np.float64).reshape(S, S) for q in generators]
        self.branch_generator = np.asarray(generator_of_node, dtype=np.int64)
        if self.branch_generator.shape[0] != self.tl.tree.node_count or self.branch_generator.min() < 0 or \
                self.branch_generator.max() >= len(self.generators):
            raise ValueError("one generator index per tree node")

    def flags(self):
        return np.array([JUMPS_REWARDS if kind == "rewards" else 0 for kind in self.kinds], dtype=np.int32)

    def preorder(self):
        """Tree nodes in the order traverse visits them: a node, then its first child's subtree, then its second's."""
        tree = self.tl.tree
        order, stack = [], [tree.root]
        while stack:
            n = stack.pop()
            order.append(n)
            if n >= tree.tip_count:
                stack.append(int(tree.right[n]))
                stack.append(int(tree.left[n]))
        return order

    def node_list(self, ancestral=True):
        """-> (rows int32 [node_count, 3] = {outRow, qIndex, parentRow}, tree node of each row).  outRow: the tree node's number
        (tips first, so tip t is output row t), or -1 for an internal node when ``ancestral`` is false."""
        tree = self.tl.tree
        order = self.preorder()
        row_of = np.full(tree.node_count, -1, dtype=np.int64)
        rows = np.zeros((len(order), 3), dtype=np.int32)
        for r, n in enumerate(order):
            row_of[n] = r
            parent = int(tree.parent[n])
            rows[r, 0] = n if (ancestral or n < tree.tip_count) else -1
            rows[r, 1] = 0 if (parent < 0 or self.branch_generator is None) else self.branch_generator[n]
            rows[r, 2] = -1 if parent < 0 else row_of[parent]
        return rows, np.asarray(order, dtype=np.int64)

    def branch_lengths(self, order):
        """branch rate x (parent height - node height) per row of the node list; row 0 (the root) 0."""
        out = np.zeros(len(order))
        for r, n in enumerate(order):
            if r > 0:
                time, rate = self.tl.node_branch_time(int(n))
                out[r] = rate * time
        return out

    def node_heights(self, order):
        return np.array([self.tl.node_height(int(n)) for n in order], dtype=np.float64)

    def simulate(self, n_sites, seed, ancestral=True, per_site=True, history=False, root_states=None, rate_categories=None,
                 category_rates_index=0, category_weights_index=0, state_frequencies_index=0):
        """One simulant.  -> dict: "alignment" uint8 [tip_count, n_sites] by tip number; "ancestral" uint8 [node_count - tip_count,
        n_sites] by node number - tip_count (``ancestral``); "categories" int32 [n_sites]; "values" [K, node_count, n_sites] by
        tree node (``per_site``); "sum_across_sites" [K, node_count] by tree node; "site_totals" [K, n_sites]; with ``history``
        "events": {"node", "site", "height", "states" [E, 2]} in (site, row, time) order, and "event_counts" [node_count, n_sites]
        by tree node."""
        if not self.registers:
            raise ValueError("add a register first")
        tree = self.tl.tree
        rows, order = self.node_list(ancestral)
        heights = self.node_heights(order) if history else None
        res = self.beagle.simulateCompleteHistories(rows, n_sites, self.branch_lengths(order), np.stack(self.generators),
                                                    np.stack(self.registers), self.flags(), seed, nodeHeights=heights,
                                                    categoryRatesIndex=category_rates_index,
                                                    categoryWeightsIndex=category_weights_index,
                                                    stateFrequenciesIndex=state_frequencies_index, root_states=root_states,
                                                    rate_categories=rate_categories, values=per_site, history=history)
        t = tree.tip_count
        out = {"alignment": res["states"][:t], "ancestral": res["states"][t:] if ancestral else None,
               "categories": res["categories"], "site_totals": res["site_totals"]}
        by_node = np.empty(len(order), dtype=np.int64)
        by_node[order] = np.arange(len(order))                # the row of every tree node
        out["sum_across_sites"] = res["row_totals"][:, by_node]
        if per_site:
            out["values"] = res["values"][:, by_node]
        if history:
            counts = res["event_counts"]
            out["event_counts"] = counts[by_node]
            flat = counts.T.reshape(-1)                       # (site, row) order, as the events are
            cell = np.repeat(np.arange(flat.size), flat)
            out["events"] = {"node": order[cell % len(order)], "site": cell // len(order), "height": res["event_heights"],
                             "states": res["event_states"]}
        return out
