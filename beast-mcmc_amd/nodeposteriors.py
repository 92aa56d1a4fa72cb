"""Marginal node state posteriors: the host side of the one-call device route (include/beagle_mi355.h
``beagleMi355NodePosteriors``).

The reference's ``<nodePosteriorLikelihood>`` (src/dr/oldevomodel/treelikelihood/NodePosteriorTreeLikelihood.java:119-235, tree trait
"posteriors") reads every node's partials and branch matrix back and rebuilds the pre-order side with host loops over nodes x patterns
x states^2.  Everything it reads is resident after a gradient pass over ``gradient.BranchGradient``'s buffer plan, so this class runs
that pass — post-order partials, root lnL, the root's pre-order partial, the pre-order list — and then asks the engine for the
posteriors of every listed node in one call.  ``route="host"`` is the reference's way over the same instance: what the device route
replaces and what tools/node_posteriors_bench.py measures it against.
"""
import time

import numpy as np

from . import beagle as _b
from .gradient import BranchGradient


class NodePosteriors(BranchGradient):
    """P(state of node i = s | pattern) for the nodes of the workload's tree, tips included."""

    def __init__(self, workload, **kwargs):
        super().__init__(workload, **kwargs)
        self.partial_tips = set()            # tips that were given partials (set_tip_partials): the host route reads them back
        self.host_seconds = {}               # the last host route's time, split: getPartials, getTransitionMatrix, numpy

    def set_tip_partials(self, tip, partials):
        self.b.setTipPartials(tip, np.asarray(partials, dtype=float).ravel())
        self.partial_tips.add(int(tip))

    def prepare(self):
        """Everything the call reads, left on the device: -> lnL."""
        lnl = self.log_likelihood()
        self.b.setPartials(self.pre_offset + self.tree.root, self._root_pre)
        self.b.updatePrePartials(self._pre_ops, len(self._pre_ops) // 7, _b.NONE)
        return lnl

    def rows(self, nodes=None):
        """The call's table for the buffers of the current evaluation: rows {post(i), pre(i)}, one per node of ``nodes`` (default:
        every node in node order)."""
        nodes = np.arange(self.N) if nodes is None else np.asarray(nodes, dtype=np.int64).reshape(-1)
        rows = np.empty((len(nodes), 2), dtype=np.int32)
        rows[:, 0] = [self.post_index(int(n)) for n in nodes]
        rows[:, 1] = self.pre_offset + nodes
        return rows

    def posteriors(self, nodes=None, full=True, map=False, totals=False, categories=False, route="device", out=None):
        """-> dict of what was asked for, after prepare(): "posteriors" [n, P, S], "map_states" / "map_probabilities" [n, P],
        "totals" [n, S] (pattern-weighted sums), "categories" [P, C] (of the first listed node), and "code": 0, or -8 when some
        pattern's likelihood was 0 or not finite (NaN there).  out: the dict of an earlier device call of the same shape, whose
        arrays are written again instead of new ones."""
        if route == "device":
            out, rc = self.b.nodePosteriors(self.rows(nodes), 0, full=full, map=map, totals=totals, categories=categories, out=out)
            out["code"] = rc
            return out
        if route != "host":
            raise ValueError("route is 'device' or 'host'")
        return self._host(np.arange(self.N) if nodes is None else np.asarray(nodes, dtype=np.int64).reshape(-1), full, map, totals, categories)

    # -- the reference's route: NodePosteriorTreeLikelihood.traverseForward / calculatePosteriors over read-back arrays ---------
    def _host(self, nodes, full, map, totals, categories):
        tr, S, P, C, T = self.tree, self.S, self.P, self.C, self.T
        t_partials = t_matrices = 0.0

        def post_of(n):
            nonlocal t_partials
            if n < T and n not in self.partial_tips:
                st = np.asarray(self.wl.tip_states[n]).astype(np.int64)
                x = np.zeros((P, S))
                known = st < S
                x[np.nonzero(known)[0], st[known]] = 1.0
                x[~known] = 1.0
                return np.broadcast_to(x, (C, P, S))
            t0 = time.perf_counter()
            x = self.b.getPartials(self.post_index(n), _b.NONE).reshape(C, P, S)
            t_partials += time.perf_counter() - t0
            return x

        def matrix_of(n):
            nonlocal t_matrices
            t0 = time.perf_counter()
            m = self.b.getTransitionMatrix(self.matrix_index(n)).reshape(C, S, S)
            t_matrices += time.perf_counter() - t0
            return m

        start = time.perf_counter()
        cw = np.asarray(self.wl.cat_weights, dtype=float)
        pw = np.asarray(self.wl.weights, dtype=float)
        where = {}
        for r, n in enumerate(nodes):
            where.setdefault(int(n), []).append(r)
        R = len(nodes)
        out = {"code": 0}
        if full:
            out["posteriors"] = np.empty((R, P, S))
        if map:
            out["map_states"] = np.empty((R, P), dtype=np.uint8)
            out["map_probabilities"] = np.empty((R, P))
        if totals:
            out["totals"] = np.empty((R, S))

        def finish(n, forward_n, post_n):              # calculatePosteriors for one node: joint / its sum over the states
            joint = forward_n * post_n
            m = np.einsum("c,cps->ps", cw, joint)
            z = m.sum(axis=1)
            bad = ~(np.isfinite(z) & (z != 0.0))
            with np.errstate(divide="ignore", invalid="ignore"):
                post = m / np.where(bad, np.nan, z)[:, None]
            if bad.any():
                out["code"] = -8
            for r in where[n]:
                if full:
                    out["posteriors"][r] = post
                if map:
                    best = np.where(bad, 0, np.argmax(np.where(np.isnan(post), -1.0, post), axis=1))
                    out["map_states"][r] = best
                    out["map_probabilities"][r] = post[np.arange(P), best]
                if totals:
                    out["totals"][r] = pw @ post
                if categories and r == 0:
                    n_c = joint.sum(axis=2) * cw[:, None]                                   # [C, P]
                    with np.errstate(divide="ignore", invalid="ignore"):
                        out["categories"] = (n_c / n_c.sum(axis=0)[None, :]).T.copy()

        root = tr.root
        stack = [(root, np.broadcast_to(np.asarray(self.wl.freqs, dtype=float), (C, P, S)))]
        while stack:                                                   # traverseForward: parent first; a node's forwardProbs live
            n, forward_n = stack.pop()                                 # until both children have theirs
            if n in where:
                finish(n, forward_n, post_of(n))
            if n < T:
                continue
            l, r = int(tr.left[n]), int(tr.right[n])
            below = {l: post_of(l) @ matrix_of(l).transpose(0, 2, 1), r: post_of(r) @ matrix_of(r).transpose(0, 2, 1)}
            for child, sib in ((r, l), (l, r)):
                f = forward_n * below[sib]                                                  # accumulateMatrixMultiply
                stack.append((child, f @ matrix_of(child)))                                 # matrixMultiplyBackward
        total = time.perf_counter() - start
        self.host_seconds = {"getPartials": t_partials, "getTransitionMatrix": t_matrices, "numpy": total - t_partials - t_matrices}
        return out
