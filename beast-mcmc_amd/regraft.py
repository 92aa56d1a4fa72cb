"""Scores of every regraft point of a pruned subtree: the host side of the one-call device route (include/beagle_mi355.h
``beagleMi355RegraftScores``) and a restatement of the reference's Gibbs tree operator.

``GibbsPruneAndRegraft`` (src/dr/evomodel/operators/GibbsPruneAndRegraft.java: ``gibbsProposal`` :89-160, ``prunedGibbsProposal``
:162-269, ``getNodeDistance`` :271-287, ``pruneAndRegraft`` :301-) picks a node i, keeps its parent iP at its height, and for every
branch (j, jP) that spans that height edits the tree, asks for the whole likelihood and edits the tree back; it then draws the regraft
point from the normalised likelihoods.  After ONE gradient pass over T' — the tree without i's subtree and iP, i's sibling hung from
i's grandparent — the engine holds what every one of those likelihoods is made of.  ``Regraft.prune`` runs that pass on
``gradient.BranchGradient``'s buffer plan, ``regraft_candidates`` forms the upper and lower matrix of every candidate in spare matrix
slots, and ``scores(route="device")`` asks the engine for lnL(T' + subtree at candidate) - lnL(T') of every candidate in one call.
``route="host"`` is the reference's loop as written, through the stock API on the same instance.

The operator's prior term is the caller's.  ``GibbsSubtreeSwap`` moves two subtrees and is not served by this call.
"""
import math

import numpy as np

from . import beagle as _b
from .inputs.synth import Workload
from .inputs.trees import Tree
from .placement import Placement, expand_states


def select(probabilities, u):
    """The reference's draw (GibbsPruneAndRegraft.java:132-146): refuse when the sum is <= 1e-100; ran = u * sum; subtract the
    probabilities in order while ran > 0; -> the index of the last one subtracted."""
    total = 0.0
    for p in probabilities:
        total += p
    if total <= 1e-100:
        raise RuntimeError("Couldn't find another proposal with a decent likelihood.")
    ran = u * total
    index = 0
    while ran > 0.0:
        ran -= probabilities[index]
        index += 1
    return index - 1


def node_distance(parent, height, a, b):
    """getNodeDistance (:271-287): steps to the meeting point of the walks up from a and b, the lower node moving first."""
    count = 0
    while a != b:
        count += 1
        if height[a] < height[b]:
            a = int(parent[a])
        else:
            b = int(parent[b])
    return count


class Regraft(Placement):
    """lnL(tree with the subtree of node i cut off and hung on another branch at its parent's height), for every such branch."""

    def __init__(self, workload, max_distance=None, **kwargs):
        """max_distance: the pruned variant's MAX_DISTANCE (default: nodeCount / 10 as an integer, :70)."""
        super().__init__(workload, **kwargs)
        self.max_distance = self.N // 10 if max_distance is None else int(max_distance)
        spare = self.extra_index + 3 * self.max_candidates
        self.merged_slot, self.pendant_slot = spare - 1, spare - 2       # the last two spare matrix slots; the candidates' come first
        self.pruned = None                   # the node whose subtree is cut off, while the instance holds the passes over T'
        self.lnl_pruned = None               # lnL(T')
        self.subtree_scale = _b.NONE
        self.candidate_nodes = []            # j of every row of the last list; the last row is the original position (i's sibling)
        self.host_evaluations = 0

    # -- T' ----------------------------------------------------------------------------------------------------------------
    def _family(self, i):
        tr = self.tree
        i = int(i)
        if i == tr.root or int(tr.parent[i]) == tr.root:
            raise ValueError("the operator moves no child of the root (GibbsPruneAndRegraft.java:99)")
        iP = int(tr.parent[i])
        sib = int(tr.right[iP]) if int(tr.left[iP]) == i else int(tr.left[iP])
        return i, iP, sib, int(tr.parent[iP])

    def _subtree(self, i):
        tr, out, stack = self.tree, [], [int(i)]
        while stack:
            n = stack.pop()
            out.append(n)
            if n >= self.T:
                stack += [int(tr.left[n]), int(tr.right[n])]
        return out

    def _pruned_arrays(self, i):
        """(parent, left, right) of T' on the tree's own numbering; iP and i's subtree keep their old entries and are never reached."""
        tr = self.tree
        i, iP, sib, iG = self._family(i)
        parent, left, right = tr.parent.copy(), tr.left.copy(), tr.right.copy()
        parent[sib] = iG
        if left[iG] == iP:
            left[iG] = sib
        else:
            right[iG] = sib
        return parent, left, right

    def _matrix_of(self, n):
        return self.merged_slot if self.pruned is not None and n == self._sib else self.matrix_index(n)

    def prune(self, i):
        """The post-order and pre-order passes over T' on the instance's own buffers -> lnL(T').  The merged branch of i's sibling
        has its matrix in a spare slot; i's subtree is evaluated into its own buffers; with rescaling its factors are accumulated
        into the scale buffer of iP, which T' does not use."""
        tr, T = self.tree, self.T
        i, iP, sib, iG = self._family(i)
        self.pruned, self._iP, self._sib, self._iG = i, iP, sib, iG
        parent, left, right = self._arrays = self._pruned_arrays(i)
        below = set(self._subtree(i))
        idx = self._nodes
        slots = np.r_[self._edge_matrix[self._set], self.merged_slot].astype(np.int32)
        lengths = np.r_[self.branch_lengths[idx], float(tr.height[iG] - tr.height[sib])]
        self.b.updateTransitionMatrices(0, slots, None, None, lengths, len(slots))
        post, kept = [], []
        for n in tr.postorder():
            if n < T or n == iP:
                continue
            l, r = int(left[n]), int(right[n])
            post += [self.post_index(n), self.scale_index(n), _b.NONE, self.post_index(l), self._matrix_of(l), self.post_index(r), self._matrix_of(r)]
            if n not in below:
                kept.append(n)
        self.b.updatePartials(np.asarray(post, dtype=np.int32), len(post) // 7, _b.NONE)
        self.subtree_scale = _b.NONE
        if self.rescale:
            self.b.resetScaleFactors(self.cum_scale)
            s = np.asarray([self.scale_index(n) for n in kept], dtype=np.int32)
            self.b.accumulateScaleFactors(s, len(s), self.cum_scale)
            inner = [n for n in below if n >= T]
            if inner:
                self.subtree_scale = self.scale_index(iP)
                self.b.resetScaleFactors(self.subtree_scale)
                s = np.asarray([self.scale_index(n) for n in inner], dtype=np.int32)
                self.b.accumulateScaleFactors(s, len(s), self.subtree_scale)
        out, zero = [0.0], None
        try:
            self.b.calculateRootLogLikelihoods([self.post_index(tr.root)], [0], [0], [self.cum_scale], 1, out)
        except _b.BeagleException as e:      # a pattern T' cannot produce: the passes are finished first, then the caller hears of it
            if e.code != -8:
                raise
            out[0], zero = float("nan"), e
        self.lnl_pruned = out[0]
        pre, stack = [], [tr.root]
        while stack:
            n = stack.pop()
            if n < T or n in below:
                continue
            l, r = int(left[n]), int(right[n])
            for child, other in ((l, r), (r, l)):
                if child not in below:
                    pre += [self.pre_offset + child, _b.NONE, _b.NONE, self.pre_offset + n, self._matrix_of(child), self.post_index(other),
                            self._matrix_of(other)]
            stack += [r, l]
        self.b.setPartials(self.pre_offset + tr.root, self._root_pre)
        self.b.updatePrePartials(np.asarray(pre, dtype=np.int32), len(pre) // 7, _b.NONE)
        if zero is not None:
            raise zero
        return self.lnl_pruned

    def admissible(self, i, max_distance=None):
        """The reference's candidate set in node order: j != root, j != i, h(j) < h(iP) < h(jP) (and, with max_distance,
        getNodeDistance(iP, jP) <= max_distance), on the tree as it stands."""
        tr = self.tree
        i, iP, _, _ = self._family(i)
        h = float(tr.height[iP])
        out = []
        for j in range(self.N):
            if j == tr.root or j == i:
                continue
            jP = int(tr.parent[j])
            if tr.height[j] < h < tr.height[jP] and (max_distance is None or node_distance(tr.parent, tr.height, iP, jP) <= max_distance):
                out.append(j)
        return out

    def regraft_candidates(self, i, max_distance=None):
        """-> the call's table [K][7] after prune(i): a row per node of admissible(i, max_distance) and one more for the original
        position, the merged branch of T'.  The upper and lower matrices are formed in the spare slots; every row shares the one
        pendant slot, h(iP) - h(i)."""
        if self.pruned != int(i):
            raise ValueError("prune(%d) first" % int(i))
        tr = self.tree
        parent, left, right = self._arrays
        iP, sib = self._iP, self._sib
        h = float(tr.height[iP])
        nodes = self.admissible(i, max_distance) + [sib]
        K = len(nodes)
        if 2 * K + 2 > 3 * self.max_candidates:
            raise ValueError("%d candidates, room for %d (max_candidates)" % (K, (3 * self.max_candidates - 2) // 2))
        base = self.extra_index
        rows = np.empty((K, 7), dtype=np.int32)
        slots, lengths = [self.pendant_slot], [h - float(tr.height[i])]
        for k, j in enumerate(nodes):
            jP = int(parent[j])
            other = int(right[jP]) if int(left[jP]) == j else int(left[jP])
            slots += [base + 2 * k, base + 2 * k + 1]
            lengths += [float(tr.height[jP]) - h, h - float(tr.height[j])]
            rows[k] = [self.pre_offset + jP, self.post_index(other), self._matrix_of(other), self.post_index(j), base + 2 * k, base + 2 * k + 1,
                       self.pendant_slot]
        self.b.updateTransitionMatrices(0, np.asarray(slots, dtype=np.int32), None, None, np.asarray(lengths, dtype=float), len(slots))
        self.candidate_nodes = nodes
        self.where = [(j, h - float(tr.height[j]), float(tr.height[int(parent[j])]) - h, h - float(tr.height[i])) for j in nodes]
        self.rows = rows
        return rows

    # -- the two routes ----------------------------------------------------------------------------------------------------
    def scores(self, route="device", candidates=None):
        """-> lnL of the tree with the subtree at each candidate of the last list (regraft_candidates), and the return code."""
        if route == "device":
            rows = self.rows if candidates is None else np.asarray(candidates, dtype=np.int32).reshape(-1, 7)
            s, _, rc = self.b.regraftScores(rows, self.post_index(self.pruned), self.subtree_scale)
            return self.lnl_pruned + s, rc
        if route == "host":
            return self._host_scores(), 0
        raise ValueError("route is 'device' or 'host'")

    def log_ratios(self, candidates=None):
        """-> (scores [K], R [K, P], return code) of the device call."""
        rows = self.rows if candidates is None else np.asarray(candidates, dtype=np.int32).reshape(-1, 7)
        return self.b.regraftScores(rows, self.post_index(self.pruned), self.subtree_scale, pattern_log_ratios=True)

    def stats(self):
        return self.b.regraftStats()

    def read_subtree(self):
        """What the call reads of the subtree, read back: its root's partials [C, P, S] (a compact tip expanded from its states) and
        its log scale factors [P], or None when no scale buffer is named."""
        i = self.pruned
        if i < self.T and i not in self.partial_tips:
            x = expand_states(self.wl.tip_states[i], self.S, self.C)
        else:
            x = self.b.getPartials(self.post_index(i), _b.NONE).reshape(self.C, self.P, self.S)
        return x, (None if self.subtree_scale == _b.NONE else self.b.getLogScaleFactors(self.subtree_scale))

    def regrafted(self, i, j):
        """(parent, left, right) of the tree after pruneAndRegraft(i, iP, j, jP) (:301-), on the tree's own numbering: iP keeps its
        index and its height."""
        i, iP, sib, _ = self._family(i)
        parent, left, right = self._pruned_arrays(i)
        j = int(j)
        jP = int(parent[j])
        if left[jP] == j:
            left[jP] = iP
        else:
            right[jP] = iP
        parent[iP], parent[j], parent[i] = jP, iP, iP
        left[iP], right[iP] = i, j
        return parent, left, right

    def regrafted_workload(self, i, j):
        """The workload over the tree of regrafted(i, j): what an ordinary evaluation of the moved tree is given."""
        wl = self.wl
        _, left, right = self.regrafted(i, j)
        return Workload(wl.name + "~", Tree(left, right, self.tree.height, self.tree.root), wl.eig, wl.freqs, wl.cat_rates, wl.cat_weights,
                        wl.tip_states, wl.weights, self.S)

    def _evaluate(self, parent, left, right, nodes, touched):
        """A stock evaluation of the tree (parent, left, right) on the instance's own buffers: the branch matrices of ``touched`` from
        the tree's heights, the partials of the internal nodes of ``nodes`` in post-order, the root sum."""
        tr = self.tree
        touched = [n for n in touched if n != tr.root]
        slots = np.asarray([self.matrix_index(n) for n in touched], dtype=np.int32)
        lengths = np.asarray([float(tr.height[int(parent[n])] - tr.height[n]) for n in touched], dtype=float)
        self.b.updateTransitionMatrices(0, slots, None, None, lengths, len(slots))
        ops = []
        for n in sorted((n for n in nodes if n >= self.T), key=lambda n: tr.height[n]):       # (a time tree: children lie below their parents)
            l, r = int(left[n]), int(right[n])
            ops += [self.post_index(n), self.scale_index(n), _b.NONE, self.post_index(l), self.matrix_index(l), self.post_index(r),
                    self.matrix_index(r)]
        self.b.updatePartials(np.asarray(ops, dtype=np.int32), len(ops) // 7, _b.NONE)
        if self.rescale:
            self.b.resetScaleFactors(self.cum_scale)
            s = self._scale_indices_by_set[self._set]
            self.b.accumulateScaleFactors(s, len(s), self.cum_scale)
        out = [0.0]
        self.b.calculateRootLogLikelihoods([self.post_index(tr.root)], [0], [0], [self.cum_scale], 1, out)
        self.host_evaluations += 1
        return out[0]

    def _host_scores(self):
        """The reference's loop: per candidate the tree edit, a stock evaluation (the nodes above the two edits, as a caller with the
        branch-move fast path updates them) and the edit back, whose dirty nodes the next evaluation recomputes.  The instance is
        left holding the unmoved tree's evaluation: prune(i) again before a device call."""
        tr = self.tree
        i, iP, sib, iG = self._family(self.pruned)
        nodes = list(self.candidate_nodes)
        self.pruned = None

        def above(parent, n):
            out = set()
            while n != -1:
                out.add(int(n))
                n = int(parent[n])
            return out

        internal = set(range(self.T, self.N))
        self._evaluate(tr.parent, tr.left, tr.right, internal, list(range(self.N)))
        stale, moved, out = set(), set(), np.empty(len(nodes))
        for k, j in enumerate(nodes):
            parent, left, right = (tr.parent, tr.left, tr.right) if j == sib else self.regrafted(i, j)
            dirty = above(parent, iP) | above(parent, iG)
            touch = {iP, sib, j}
            out[k] = self._evaluate(parent, left, right, dirty | stale, touch | moved)
            stale, moved = dirty, touch
        self._evaluate(tr.parent, tr.left, tr.right, above(tr.parent, iP) | stale, {iP, sib} | moved)
        return out

    # -- the operator --------------------------------------------------------------------------------------------------------
    def proposal_from_scores(self, i, u, lnl, pruned=False):
        """gibbsProposal (pruned=False) / prunedGibbsProposal (pruned=True) from lnL per row of the last list, which regraft_candidates
        built WITHOUT a distance limit (the pruned variant's two neighbourhoods are cut out of it here: they share T').  u: the
        uniform the reference draws.  -> (chosen j, log Hastings ratio, the forward probabilities, forward / sum)."""
        tr = self.tree
        i, iP, sib, iG = self._family(i)
        nodes = self.candidate_nodes
        if len(lnl) != len(nodes) or nodes[-1] != sib:
            raise ValueError("one lnL per row of regraft_candidates(i)")
        lnl_of = {j: float(x) for j, x in zip(nodes, lnl)}
        backward_likelihood = lnl_of[sib]
        offset = int(-backward_likelihood)
        backward = math.exp(backward_likelihood + offset)
        forward_nodes = nodes[:-1]
        if pruned:
            forward_nodes = [j for j in forward_nodes if node_distance(tr.parent, tr.height, iP, int(tr.parent[j])) <= self.max_distance]
        probabilities = [math.exp(lnl_of[j] + offset) for j in forward_nodes]
        index = select(probabilities, u)
        if index < 0:
            raise IndexError("u = 0 selects nothing (the reference's list lookup at -1 throws)")
        total = 0.0
        for p in probabilities:
            total += p
        j = forward_nodes[index]
        forward = probabilities[index]
        forward_prob = forward / total
        if pruned:
            parent, _, _ = self.regrafted(i, j)
            sum_backward = 0.0
            for n in sorted(nodes):
                if n != j and node_distance(parent, tr.height, iP, int(parent[n])) <= self.max_distance:
                    sum_backward += math.exp(lnl_of[n] + offset)
            backward_prob = backward / sum_backward
        else:
            backward_prob = backward / (total - forward + backward)
        return j, math.log(backward_prob / forward_prob), np.asarray(probabilities) / total

    def gibbs_proposal(self, i, u, pruned=False, route="device"):
        """-> (chosen j, log Hastings ratio, probabilities): one prune, one list of every admissible candidate, one call (or the
        host route's loop), the draw."""
        self.prune(i)
        self.regraft_candidates(i)
        lnl, _ = self.scores(route=route)
        return self.proposal_from_scores(i, u, lnl, pruned=pruned)
