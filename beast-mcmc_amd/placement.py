"""Scores of attaching new sequences on every branch: the host side of the one-call device route (include/beagle_mi355.h
``beagleMi355PlacementScores``).

The reference's online inference (src/dr/app/realtime: ``CheckPointUpdaterApp``, ``CheckPointTreeModifier.incorporateAdditionalTaxa``
:434-800, ``SimpleDistanceMatrix.calculatePairwiseDistance`` :63-93) places each new taxon next to the existing taxon with the smallest
p-distance.  That stands in for the likelihood of the new sequence attached at a point of the tree given everything already there —
and after a gradient pass the engine holds everything that likelihood is made of.  This class runs the pass over
``gradient.BranchGradient``'s buffer plan, forms the three matrices of every candidate attachment in spare matrix slots, and asks the
engine for lnL(tree + query at candidate) - lnL(tree) of every (query, candidate) in one call.  ``route="host"`` is the numpy
restatement over ``getPartials`` / ``getTransitionMatrix`` of the same instance (what the device route replaces and
tools/placement_bench.py measures it against); ``route="distance"`` is the reference's own rule.
"""
import time

import numpy as np

from . import beagle as _b
from .gradient import BranchGradient
from .inputs.synth import Workload
from .inputs.trees import Tree

MISSING = 255


class Placement(BranchGradient):
    """lnL(tree with a new sequence attached at a candidate point) - lnL(tree), for lists of sequences and candidates."""

    def __init__(self, workload, max_candidates=None, **kwargs):
        """max_candidates: how many candidates one list may hold (three matrix slots each; default: two per node and eight)."""
        n = workload.tree.node_count
        self.max_candidates = 2 * n + 8 if max_candidates is None else int(max_candidates)
        kwargs.setdefault("extra_matrices", 3 * self.max_candidates)
        super().__init__(workload, **kwargs)
        self.partial_tips = set()            # tips that were given partials (set_tip_partials): the host route reads them back
        self.host_seconds = {}               # the last host route's time, split: getPartials, getTransitionMatrix, numpy
        self.rows = np.zeros((0, 7), dtype=np.int32)      # the last list (candidates())
        self.where = []                      # per candidate of the last list: (node or None above the root, lower, upper, pendant)

    def set_tip_partials(self, tip, partials):
        self.b.setTipPartials(tip, np.asarray(partials, dtype=float).ravel())
        self.partial_tips.add(int(tip))

    def prepare(self):
        """Everything the call reads, left on the device: -> lnL."""
        lnl = self.log_likelihood()
        self.b.setPartials(self.pre_offset + self.tree.root, self._root_pre)
        self.b.updatePrePartials(self._pre_ops, len(self._pre_ops) // 7, _b.NONE)
        return lnl

    def candidates(self, edges=None, fractions=(0.5,), pendant_lengths=None, tip_height=None, above_root=()):
        """-> the call's table [K][7] for the buffers of the current evaluation.  Per node of ``edges`` (default: every branch) and
        per fraction f a candidate at f of the branch above the node (0: at the node, 1: at its parent); per length x of
        ``above_root`` one at x above the root.  The pendant branch: ``pendant_lengths`` (one length, or one per candidate), or on a
        time tree the attachment's height less ``tip_height``; by default the mean branch length.  The upper, lower and pendant
        matrices are formed in the spare matrix slots; distinct pendant lengths share a slot."""
        tr = self.tree
        edges = self.edges if edges is None else [int(n) for n in edges]
        where = []
        for n in edges:
            if n == tr.root:
                raise ValueError("the root has no branch: use above_root")
            t = float(self.branch_lengths[n])
            for f in fractions:
                where.append([n, f * t, (1.0 - f) * t, float(tr.height[n]) + f * (float(tr.height[tr.parent[n]]) - float(tr.height[n]))])
        for x in above_root:
            where.append([None, float(x), 0.0, float(tr.height[tr.root]) + float(x)])
        K = len(where)
        if K > self.max_candidates:
            raise ValueError("%d candidates, room for %d (max_candidates)" % (K, self.max_candidates))
        if tip_height is not None:
            pend = np.array([w[3] - float(tip_height) for w in where])
        elif pendant_lengths is None:
            pend = np.full(K, float(np.mean(self.branch_lengths[self._nodes])))
        else:
            pend = np.broadcast_to(np.asarray(pendant_lengths, dtype=float), (K,)).copy()
        if np.any(pend < 0):
            raise ValueError("a pendant branch of negative length")
        distinct, which = np.unique(pend, return_inverse=True)
        base = self.extra_index
        rows = np.empty((K, 7), dtype=np.int32)
        slots, lengths = [], []
        for k, (n, lower, upper, _) in enumerate(where):
            low_slot, pend_slot = base + 2 * k + 1, base + 2 * K + int(which[k])
            slots.append(low_slot); lengths.append(lower)
            if n is None:
                rows[k] = [self.pre_offset + tr.root, _b.NONE, _b.NONE, self.post_index(tr.root), _b.NONE, low_slot, pend_slot]
            else:
                p = int(tr.parent[n])
                sib = int(tr.right[p]) if int(tr.left[p]) == n else int(tr.left[p])
                slots.append(base + 2 * k); lengths.append(upper)
                rows[k] = [self.pre_offset + p, self.post_index(sib), self.matrix_index(sib), self.post_index(n), base + 2 * k, low_slot, pend_slot]
        slots += [base + 2 * K + j for j in range(len(distinct))]
        lengths += [float(x) for x in distinct]
        self.b.updateTransitionMatrices(0, np.asarray(slots, dtype=np.int32), None, None, np.asarray(lengths, dtype=float), len(slots))
        self.where = [(w[0], w[1], w[2], float(pend[k])) for k, w in enumerate(where)]
        self.rows = rows
        return rows

    # -- the three routes ------------------------------------------------------------------------------------------------
    def scores(self, site_patterns, query_codes, code_table, route="device", candidates=None):
        """-> after prepare() and candidates(): scores [Q, K] and the return code (0, or -8 when some pattern's likelihood was 0 or
        not finite: NaN there).  route="distance": (closest taxon [Q], p-distance [Q]) as the reference finds them."""
        rows = self.rows if candidates is None else np.asarray(candidates, dtype=np.int32).reshape(-1, 7)
        if route == "device":
            s, _, rc = self.b.placementScores(rows, site_patterns, query_codes, code_table)
            return s, rc
        if route == "host":
            return self._host_scores(rows, site_patterns, query_codes, code_table)
        if route == "distance":
            return self.distances(site_patterns, query_codes, code_table)
        raise ValueError("route is 'device', 'host' or 'distance'")

    def log_table(self, code_table, route="device", candidates=None):
        """-> T [K, P, codeCount] = log(N / D), and the return code."""
        rows = self.rows if candidates is None else np.asarray(candidates, dtype=np.int32).reshape(-1, 7)
        if route == "device":
            P = self.P
            _, t, rc = self.b.placementScores(rows, np.zeros(1, dtype=np.int32), np.full((1, 1), MISSING, dtype=np.uint8), code_table,
                                              log_table=True)
            assert t.shape[1] == P
            return t, rc
        return self._host_table(rows, code_table)

    def stats(self):
        return self.b.placementStats()

    def operands(self, rows=None, keep_partials=True):
        """What a list names, read back from the instance candidate by candidate: (pre, sib or None, Msib or None, child, Mup or None,
        Mlow, Mpend), partials as [C, P, S] (compact tips expanded from their states) and matrices as [C, S, S].  keep_partials: a
        buffer named twice is read once (a list over a large alignment cannot keep them)."""
        rows = self.rows if rows is None else np.asarray(rows).reshape(-1, 7)
        S, P, C = self.S, self.P, self.C
        hs = self.host_seconds = {"getPartials": 0.0, "getTransitionMatrix": 0.0}
        partials, matrices = {}, {}

        def partial(i):
            if i in partials:
                return partials[i]
            if i < self.T and i not in self.partial_tips:
                x = expand_states(self.wl.tip_states[i], S, C)
            else:
                t0 = time.perf_counter()
                x = self.b.getPartials(i, _b.NONE).reshape(C, P, S)
                hs["getPartials"] += time.perf_counter() - t0
            if keep_partials:
                partials[i] = x
            return x

        def matrix(i):
            if i not in matrices:
                t0 = time.perf_counter()
                matrices[i] = self.b.getTransitionMatrix(i).reshape(C, S, S)
                hs["getTransitionMatrix"] += time.perf_counter() - t0
            return matrices[i]

        for pre, sib, msib, child, mup, mlow, mpend in (tuple(int(x) for x in r) for r in rows):
            yield (partial(pre), None if sib == _b.NONE else partial(sib), None if msib == _b.NONE else matrix(msib), partial(child),
                   None if mup == _b.NONE else matrix(mup), matrix(mlow), matrix(mpend))

    def read_back(self, rows=None):
        return list(self.operands(rows))

    def _host_tables(self, rows, code_table, keep_partials=True):
        """The log table of one candidate after the other, and whether its D was 0 or not finite somewhere."""
        w = np.asarray(self.wl.cat_weights, dtype=float)
        g = np.asarray(code_table, dtype=float).reshape(-1, self.S)
        for pre, sib, msib, child, mup, mlow, mpend in self.operands(rows, keep_partials):
            u = pre if sib is None else pre * (sib @ msib.transpose(0, 2, 1))
            t = u if mup is None else u @ mup
            e = t * (child @ mlow.transpose(0, 2, 1))
            d = np.einsum("c,cpa->p", w, e)
            n = np.einsum("c,cpx->px", w, e @ (mpend @ g.T))
            bad = ~(np.isfinite(d) & (d != 0.0))
            with np.errstate(divide="ignore", invalid="ignore"):
                yield np.log(n / np.where(bad, np.nan, d)[:, None]), bool(bad.any())

    def _host_table(self, rows, code_table):
        start = time.perf_counter()
        tables, bad = zip(*self._host_tables(rows, code_table))
        self.host_seconds["numpy"] = time.perf_counter() - start - self.host_seconds["getPartials"] - self.host_seconds["getTransitionMatrix"]
        return np.stack(tables), (-8 if any(bad) else 0)

    def _host_scores(self, rows, site_patterns, query_codes, code_table):
        """The scores candidate by candidate, so that no more than one log table is ever held."""
        start = time.perf_counter()
        X = np.asarray(code_table).reshape(-1, self.S).shape[0]
        n = count_table(site_patterns, query_codes, self.P, X).reshape(-1, self.P * X)
        dense = n.astype(float)
        out, rc = np.empty((len(n), len(rows))), 0
        for k, (table, bad) in enumerate(self._host_tables(rows, code_table, keep_partials=self.P * len(rows) <= 1 << 22)):
            flat = table.reshape(-1)
            if np.isfinite(flat).all():
                out[:, k] = dense @ flat
            else:                                               # an entry no site of a query uses must not reach its score
                for q, row in enumerate(n):
                    used = np.nonzero(row)[0]
                    out[q, k] = flat[used] @ row[used].astype(float) if len(used) else 0.0
            rc = -8 if bad else rc
        self.host_seconds["numpy"] = time.perf_counter() - start - self.host_seconds["getPartials"] - self.host_seconds["getTransitionMatrix"]
        return out, rc

    def distances(self, site_patterns, query_codes, code_table, gap_codes=(MISSING,)):
        """SimpleDistanceMatrix.calculatePairwiseDistance (:63-93) between every query and every taxon of the tree, and
        CheckPointUpdaterApp's getClosestTaxon over them: a site counts when neither state is a gap (a query code of ``gap_codes``; a
        taxon state >= S), and is a difference when neither is ambiguous (a code whose row is no unit vector) and they differ; the
        distance is differences / sites counted (0 / 0 = NaN, as in Java), the closest taxon the first with the strictly smallest
        distance (taxon 0 when no distance is below Double.MAX_VALUE).  -> (closest [Q], distance to it [Q])."""
        sites = np.asarray(site_patterns, dtype=np.int64).reshape(-1)
        codes = np.asarray(query_codes, dtype=np.int64).reshape(-1, len(sites))
        g = np.asarray(code_table, dtype=float).reshape(-1, self.S)
        unit = (np.sum(g == 1.0, axis=1) == 1) & (np.sum(g != 0.0, axis=1) == 1)
        state_of = np.where(unit, np.argmax(g, axis=1), -1)
        kept = sites >= 0
        taxa = np.asarray(self.wl.tip_states)[:, sites[kept]].astype(np.int64)                 # [T, sites kept]
        closest, distance = np.zeros(len(codes), dtype=np.int64), np.empty(len(codes))
        for q, row in enumerate(codes[:, kept]):
            gap = np.isin(row, np.asarray(gap_codes))
            state = np.where(gap, -1, state_of[np.where(gap, 0, row)])                      # -1: ambiguous (or gap)
            best, best_d = 0, np.finfo(float).max
            for t in range(self.T):
                counted = ~gap & (taxa[t] < self.S)
                differ = counted & (state >= 0) & (state != taxa[t])
                with np.errstate(divide="ignore", invalid="ignore"):
                    d = np.float64(differ.sum()) / np.float64(counted.sum())
                if d < best_d:
                    best, best_d = t, d
            closest[q] = best
            counted = ~gap & (taxa[best] < self.S)
            with np.errstate(divide="ignore", invalid="ignore"):
                distance[q] = np.float64((counted & (state >= 0) & (state != taxa[best])).sum()) / np.float64(counted.sum())
        return closest, distance

    # -- the augmented tree ----------------------------------------------------------------------------------------------
    def attach(self, query_codes_row, candidate, site_patterns, code_table):
        """The tree with the query attached at candidate ``candidate`` of the last list, as a Workload over the distinct (pattern,
        code) columns of the kept sites with their counts as weights: a new tip T (the old internal nodes move up by one) under a
        new internal node 2T.  ``patterns`` are the columns' patterns, ``new_tip`` is the tip's index and ``new_tip_partials`` [columns, S] its rows of ``code_table`` (its
        tip_states say "unknown": give the instance the partials); ``base`` is the old tree over the same columns, so that
        log_likelihood(augmented) - log_likelihood(augmented.base) is the score's meaning."""
        tr, T, S = self.tree, self.T, self.S
        node, lower, upper, pendant = self.where[candidate]
        sites = np.asarray(site_patterns, dtype=np.int64).reshape(-1)
        row = np.asarray(query_codes_row, dtype=np.int64).reshape(-1)
        kept = (sites >= 0) & (row != MISSING)
        keys, counts = np.unique(sites[kept] * 256 + row[kept], return_counts=True)
        pats, codes = keys // 256, keys % 256
        g = np.asarray(code_table, dtype=float).reshape(-1, S)
        old = np.asarray(self.wl.tip_states)[:, pats]
        shift = lambda n: int(n) if n < T else int(n) + 1                      # noqa: E731
        N = tr.node_count
        left, right, height = [-1] * (N + 2), [-1] * (N + 2), [0.0] * (N + 2)
        for n in range(N):
            height[shift(n)] = float(tr.height[n])
            if n >= T:
                left[shift(n)], right[shift(n)] = shift(tr.left[n]), shift(tr.right[n])
        new_tip, new_node = T, N + 1
        below = tr.root if node is None else node
        at = float(tr.height[below]) + lower
        height[new_node], height[new_tip] = at, at - pendant
        left[new_node], right[new_node] = shift(below), new_tip
        root = shift(tr.root)
        if node is None:
            root = new_node
        else:
            p = shift(tr.parent[node])
            if left[p] == shift(node):
                left[p] = new_node
            else:
                right[p] = new_node
        wl = self.wl
        states = np.concatenate([old, np.full((1, len(pats)), S, dtype=old.dtype)], axis=0).astype(np.int32)
        aug = Workload(wl.name + "+1", Tree(left, right, height, root), wl.eig, wl.freqs, wl.cat_rates, wl.cat_weights,
                       np.ascontiguousarray(states), counts.astype(np.float64), S)
        aug.new_tip, aug.new_tip_partials, aug.patterns = new_tip, np.ascontiguousarray(g[codes]), pats
        aug.base = Workload(wl.name, tr, wl.eig, wl.freqs, wl.cat_rates, wl.cat_weights, np.ascontiguousarray(old.astype(np.int32)),
                            counts.astype(np.float64), S)
        return aug


def log_likelihood(workload, partial_tips=None, **kwargs):
    """lnL of a workload through an ordinary evaluation (library=...: which engine); a workload from Placement.attach gets its new
    tip's partials, ``partial_tips`` {tip: [P, S]} any others."""
    g = BranchGradient(workload, **kwargs)
    try:
        tips = dict(partial_tips or {})
        if hasattr(workload, "new_tip"):
            tips[workload.new_tip] = workload.new_tip_partials
        for tip, x in tips.items():
            g.b.setTipPartials(int(tip), np.asarray(x, dtype=float).ravel())
        return g.log_likelihood()
    finally:
        g.close()


def expand_states(states, S, C):
    """Compact tip states as partials [C, P, S]: 1.0 at the state, all ones for a state >= S."""
    st = np.asarray(states).astype(np.int64)
    x = np.zeros((len(st), S))
    known = st < S
    x[np.nonzero(known)[0], st[known]] = 1.0
    x[~known] = 1.0
    return np.broadcast_to(x, (C, len(st), S))


def count_table(site_patterns, query_codes, P, X):
    """n [Q, P, X]: kept sites of each query per (pattern, code)."""
    sites = np.asarray(site_patterns, dtype=np.int64).reshape(-1)
    codes = np.asarray(query_codes, dtype=np.int64).reshape(-1, len(sites))
    n = np.zeros((len(codes), P * X), dtype=np.int64)
    for q, row in enumerate(codes):
        kept = (sites >= 0) & (row != MISSING)
        np.add.at(n[q], sites[kept] * X + row[kept], 1)
    return n.reshape(len(codes), P, X)


def score_product(table, site_patterns, query_codes):
    """score [Q, K] = sum_{p, x} n[q][p][x] T_k[p][x] over the entries with n != 0."""
    K, P, X = table.shape
    n = count_table(site_patterns, query_codes, P, X).reshape(-1, P * X)
    flat = table.reshape(K, P * X)
    out = np.empty((len(n), K))
    for q, row in enumerate(n):
        used = np.nonzero(row)[0]
        out[q] = flat[:, used] @ row[used].astype(float) if len(used) else 0.0
    return out
