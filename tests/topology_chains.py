"""Seeded MCMC-style chains whose proposals CHANGE THE TOPOLOGY, as plain records, and a driver that executes them on any engine library.

A BEAST chain spends about half of its tree proposals on narrow and wide exchange, subtree slide and Wilson-Balding.  As far as the
BEAGLE surface goes these are two moves:

  narrow   node i (its parent p is not the root) and its uncle u, the sibling of p, swap places.  No height changes; u must lie
           below p.
  prune    prune and regraft: i has parent p, sibling s, grandparent g.  s takes p's place under g (or becomes the root when p was the
           root); p goes onto the branch above a target j outside what is pruned (the subtree of i, and p itself; not s, above which p
           already sits) at a new height, and becomes the root when j is the root.  Node numbers follow BEAST: p travels with i.

besides which a chain here makes

  height   a new height for one internal node, and
  model    new category rates and the eigen system in the other eigen slot: every node is dirty and the operation list is closed.

``Driver`` is a Python restatement of the caller stand-in (tools/host/tree_likelihood.cpp: BufferIndexHelper flips for partials,
matrices, the eigen slot and the scale buffers with storeState / restoreState; prepare / attempt / finish with the NONE, ALWAYS and
DYNAMIC schemes and a settable rescaling frequency; POST_ORDER and REVERSE_LEVEL_ORDER traversal) over a ``beagle.Beagle`` of the engine
or of the CPU oracle — with a tree that can change.  The dirty set is the stand-in's rule and no other: a node named by a tree-changed
event is dirty together with both of its children (updateNodeAndChildren), a dirty node that has a parent gets a new branch matrix in
the other flip, and a node gets an operation when the subtree of one of its children was updated.  A rejected move puts topology and
heights back and calls restoreState; nothing is recomputed, as in BEAST.

``generate(shape, seed, steps)`` draws the records from the shape's tree alone (no likelihood): they survive a JSON round trip, and a
failing chain is dumped with ``dump`` and run again with ``python tests/topology_chains.py --replay FILE``.  New heights come from the
middle 90 % of the admissible interval, so no branch collapses.  Every chain of 40 steps or more holds each move kind at least five
times, a rejected topology move, an accepted root change in both directions (p onto the branch above the root; a child of the root
pruned, so that its sibling becomes the root) and a run of five model moves — the first rejected — which sends the same closed list
more than once in read mode.

This module is plain Python and numpy and loads no library: the tests hand it the binding class and the library.
"""
import json

import numpy as np

NONE = -1
SCHEME_NONE, SCHEME_ALWAYS, SCHEME_DYNAMIC = 0, 1, 2          # tools/host/tree_likelihood.cpp Scheme
POST_ORDER, REVERSE_LEVEL_ORDER = 0, 1
SCHEME_NAMES = {SCHEME_NONE: "none", SCHEME_ALWAYS: "always", SCHEME_DYNAMIC: "dynamic"}
MOVES = ("height", "narrow", "prune", "model")
TOPOLOGY_MOVES = ("narrow", "prune")
RESCALING_FREQUENCY = 7                                      # write-mode cycles fall inside a chain of 60 proposals
BOUND = 1e-10                                                # tests/test_gpu_parity.py REL_TOL, tests/call_sequences.py BOUND
# No branch of a chain is shorter than this (substitutions per site at rate 1).  A transition matrix out of an eigen system has entries
# with an ABSOLUTE error of some 1e-16 x a few units, whoever computes it; over a cherry of two different states whose branches are both
# of length t every entry of the partial is of order t, so the comparison against the pattern's largest entry sees 1e-15 / t — at the
# 3e-5 a coalescent tree's youngest branch or a few height moves in a row reach, above the 1e-11 these chains are asked to be conditioned to
# (tests/test_topology_chains_host.py).  At 0.004 that term is 3e-13.
MIN_BRANCH = 0.004


# ---- the tree -----------------------------------------------------------------------------------------------------------------------
class MutableTree:
    """left / right / parent / height over node numbers (tips 0..T-1) and the root, as lists of plain numbers."""

    def __init__(self, left, right, height, root):
        self.left, self.right = [int(x) for x in left], [int(x) for x in right]
        self.height = [float(x) for x in height]
        self.root = int(root)
        self.node_count = len(self.left)
        self.tip_count = (self.node_count + 1) // 2
        self.parent = [-1] * self.node_count
        for n in range(self.tip_count, self.node_count):
            self.parent[self.left[n]] = n
            self.parent[self.right[n]] = n

    def snapshot(self):
        return (list(self.left), list(self.right), list(self.parent), list(self.height), self.root)

    def put_back(self, snap):
        self.left, self.right, self.parent, self.height = (list(x) for x in snap[:4])
        self.root = snap[4]

    def sibling(self, n):
        p = self.parent[n]
        return self.right[p] if self.left[p] == n else self.left[p]

    def below(self, n, top):
        while n >= 0:
            if n == top:
                return True
            n = self.parent[n]
        return False

    def _replace_child(self, p, old, new):
        if self.left[p] == old:
            self.left[p] = new
        else:
            self.right[p] = new
        self.parent[new] = p

    def narrow_exchange(self, i):
        """-> (nodes whose parent changed, nodes whose children changed)"""
        p = self.parent[i]
        g, u = self.parent[p], self.sibling(p)
        self._replace_child(p, i, u)
        self._replace_child(g, u, i)
        return [i, u], [p, g]

    def prune_regraft(self, i, j, height):
        p, s = self.parent[i], self.sibling(i)
        g = self.parent[p]
        assert not self.below(j, i) and j != p and j != s
        children_changed = [p]
        if g >= 0:
            self._replace_child(g, p, s)
            children_changed.append(g)
        else:
            self.root, self.parent[s] = s, -1
        jp = self.parent[j]
        if self.left[p] == s:
            self.left[p] = j
        else:
            self.right[p] = j
        if jp >= 0:
            self._replace_child(jp, j, p)
            if jp != g:
                children_changed.append(jp)
        else:
            self.root, self.parent[p] = p, -1
        self.parent[j] = p
        self.height[p] = float(height)
        return [s, p, j], children_changed

    def check(self):
        """every branch has positive length, every node but the root one parent"""
        seen = [0] * self.node_count
        for n in range(self.tip_count, self.node_count):
            for c in (self.left[n], self.right[n]):
                assert self.parent[c] == n and self.height[n] - self.height[c] >= MIN_BRANCH * (1 - 1e-9), (n, c)
                seen[c] += 1
        assert self.parent[self.root] == -1 and seen[self.root] == 0 and sum(seen) == self.node_count - 1


# ---- workloads ------------------------------------------------------------------------------------------------------------------------
_workloads = {}
# (96, 300, 4): the rule's seed, 1676, draws a tree whose memory definitions are never evaluated from memory in these chains — no sub-run
# (tests/test_gpu_topology_chains.py asks for one); 502 is the seed tests/test_gpu_memdef_tables.py makes that case with on this shape
WORKLOAD_SEEDS = {(4, 4, 96, 300, "compressed"): 502}


def workload(shape):
    """shape = (states, categories, tips, patterns[, kind]).  kind "compressed": the alignments tests/test_gpu_repeats.py draws (a shallow
    coalescent tree, root_to_tip 0.15, 1 % unknown: sub-patterns repeat); "shipped": a Yule tree; default: helpers.random_workload's."""
    if shape not in _workloads:
        import helpers
        S, C, T, P = shape[:4]
        kind = shape[4] if len(shape) > 4 else "plain"
        seed = WORKLOAD_SEEDS.get(shape, 700 + 7 * T + P + S)
        if kind == "compressed":
            wl = helpers.random_workload(T, P, S, C, seed=seed, unknown_fraction=0.01, root_to_tip=0.15)
        elif kind == "shipped":
            wl = helpers.random_workload(T, P, S, C, seed=seed, tree_kind="yule", unknown_fraction=0.01)
        else:
            wl = helpers.random_workload(T, P, S, C, seed=seed)
        _workloads[shape] = wl
    return _workloads[shape]


def shape_id(shape):
    return "S%d-C%d-T%d-P%d" % tuple(shape[:4]) + ("-" + shape[4] if len(shape) > 4 else "")


def initial_tree(shape):
    """The shape's tree with every branch at least MIN_BRANCH long: a node lower than that above a child is lifted, children first."""
    wl = workload(shape)
    tree = MutableTree(wl.tree.left, wl.tree.right, wl.tree.height, wl.tree.root)
    order, stack = [], [tree.root]
    while stack:
        n = stack.pop()
        if n >= tree.tip_count:
            order.append(n)
            stack += [tree.left[n], tree.right[n]]
    for n in reversed(order):                                 # (children before parents)
        tree.height[n] = max(tree.height[n], max(tree.height[tree.left[n]], tree.height[tree.right[n]]) + MIN_BRANCH)
    tree.check()
    return tree


# ---- the generator ----------------------------------------------------------------------------------------------------------------------
def _middle(rng, lo, hi):
    return float(lo + (0.05 + 0.9 * rng.random()) * (hi - lo))


def _height_interval(tree, n):
    """the admissible interval of internal node n's height: every branch it touches stays MIN_BRANCH long"""
    lo = max(tree.height[tree.left[n]], tree.height[tree.right[n]]) + MIN_BRANCH
    hi = tree.height[tree.parent[n]] - MIN_BRANCH if tree.parent[n] >= 0 else max(tree.height[n], lo) + 0.25 * (tree.height[n] - lo + MIN_BRANCH)
    return lo, hi


def _draw_narrow(tree, rng):
    for _ in range(400):
        i = int(rng.integers(tree.node_count))
        if i == tree.root or tree.parent[i] == tree.root:
            continue
        p = tree.parent[i]
        if tree.height[tree.sibling(p)] + MIN_BRANCH <= tree.height[p]:
            return {"move": "narrow", "i": i}
    return None


def _prune_record(tree, rng, i, j):
    lo = max(tree.height[i], tree.height[j]) + MIN_BRANCH
    jp = tree.parent[j]
    if jp == tree.parent[i]:                                  # (j == s is excluded by the callers; here jp is p only then)
        return None
    hi = tree.height[jp] - MIN_BRANCH if jp >= 0 else tree.height[j] * 1.25 + MIN_BRANCH
    if not lo < hi:
        return None
    return {"move": "prune", "i": i, "j": j, "height": _middle(rng, lo, hi)}


def _draw_prune(tree, rng, force=None):
    """force "up": j is the root (p becomes the root); "down": a child of the root is pruned (its sibling becomes the root)"""
    if force == "down":
        a, b = tree.left[tree.root], tree.right[tree.root]
        s, i = (a, b) if tree.height[a] > tree.height[b] else (b, a)      # (the higher child is internal: s, and i lies below it)
        first = rng.random() < 0.5
        for j in ((tree.left[s], tree.right[s]) if first else (tree.right[s], tree.left[s])):
            rec = _prune_record(tree, rng, i, j)
            if rec is not None:
                return rec
        return None
    for _ in range(400):
        i = int(rng.integers(tree.node_count))
        j = tree.root if force == "up" else int(rng.integers(tree.node_count))
        if i == tree.root or (force == "up" and tree.parent[i] == tree.root):
            continue
        if tree.below(j, i) or j == tree.parent[i] or j == tree.sibling(i):
            continue
        rec = _prune_record(tree, rng, i, j)
        if rec is not None:
            return rec
    return None


def apply_move(tree, rec):
    """The move of `rec` on `tree`.  -> the nodes the tree-changed events name: (parent changed, children changed); a model move: None"""
    if rec["move"] == "height":
        tree.height[rec["node"]] = rec["height"]
        return [], [rec["node"]]
    if rec["move"] == "narrow":
        return tree.narrow_exchange(rec["i"])
    if rec["move"] == "prune":
        return tree.prune_regraft(rec["i"], rec["j"], rec["height"])
    return None


def generate(shape, seed, steps=60, scheme=SCHEME_DYNAMIC, checkpoints=True):
    """The records of one chain: {"move", its arguments, "accept", "level" (reverse level order; else post order), "reads"}.  reads:
    "site" on every fifth step; "nodes" — every current node buffer and scale buffer — at two seeded checkpoints (`checkpoints`) and at
    the end.  lnL is read at every step.  `scheme` does not change the moves: a record's "write" says whether the stand-in's policy
    makes its evaluation a write-mode (rescaling) one under that scheme, evaluation 0 being the one before the chain."""
    rng = np.random.default_rng([seed, 17, shape[2], shape[3]])
    tree = initial_tree(shape)
    # the kinds: about a third heights, a quarter each of the two topology moves, the rest model moves; the forced ones at seeded places
    n_top = max(3, (steps * 13) // 56)
    n_model = max(1, steps // 20)
    block = 5 if steps >= 40 else 3
    kinds = ["narrow"] * n_top + ["prune"] * n_top + ["model"] * n_model
    kinds += ["height"] * max(0, steps - len(kinds) - 2 - block)
    kinds = [kinds[k] for k in rng.permutation(len(kinds))]
    for forced in ("prune-up", "prune-down"):
        kinds.insert(int(rng.integers(1, len(kinds))), forced)
    at = int(rng.integers(1, len(kinds)))
    kinds[at:at] = ["model-rejected"] + ["model-accepted"] * (block - 1)
    cps = sorted(int(x) for x in rng.choice(np.arange(2, len(kinds) - 2), size=2, replace=False))
    if not checkpoints:
        cps = []                                              # (drawn all the same: the moves do not depend on what is read)
    block_level = bool(rng.random() < 0.5)
    records, evaluation, rejected_topology = [], 0, False
    for step in range(len(kinds)):
        kind, rec = kinds[step], None
        if kind == "narrow":
            rec = _draw_narrow(tree, rng)
        elif kind.startswith("prune"):
            rec = _draw_prune(tree, rng, force=kind[6:] or None)
            if rec is None and kind != "prune":               # no room for it on this tree: it changes places with a later height move
                later = [k for k in range(step + 1, len(kinds)) if kinds[k] == "height"]
                assert later, "no %s on this tree" % kind
                kinds[later[0]], kind = kind, "height"
        elif kind.startswith("model"):
            rec = {"move": "model", "factor": float(rng.uniform(0.8, 1.25))}
        while rec is None:
            n = int(rng.integers(tree.tip_count, tree.node_count))
            lo, hi = _height_interval(tree, n)
            if lo < hi:
                rec = {"move": "height", "node": n, "height": _middle(rng, lo, hi)}
        rec["accept"] = bool(rng.random() < 2.0 / 3.0)
        if kind in ("prune-up", "prune-down", "model-accepted"):
            rec["accept"] = True
        elif kind == "model-rejected":
            rec["accept"] = False
        elif rec["move"] in TOPOLOGY_MOVES and not rejected_topology and step >= len(kinds) // 2:
            rec["accept"] = False                              # (no seed goes without a rejected topology move)
        rejected_topology = rejected_topology or (rec["move"] in TOPOLOGY_MOVES and not rec["accept"])
        rec["level"] = bool(rng.random() < 0.5)
        if kind in ("model-rejected", "model-accepted"):
            rec["level"] = block_level                        # (one traversal order through the run of model moves: the same list comes again)
        evaluation += 1
        rec["write"] = scheme == SCHEME_ALWAYS or (scheme == SCHEME_DYNAMIC and evaluation % (RESCALING_FREQUENCY + 1) == 0)
        rec["reads"] = (["site"] if step % 5 == 4 else []) + (["nodes"] if step in cps or step == len(kinds) - 1 else [])
        rec["last"] = step == len(kinds) - 1
        rec["gradient"] = step % 4 == 3 or rec["last"]
        if rec["accept"]:
            apply_move(tree, rec)
            tree.check()
        records.append(rec)
    return records


def census(records, shape):
    """what a chain holds: moves by kind, rejected topology moves, accepted root changes by direction, write-mode evaluations"""
    tree = initial_tree(shape)
    out = {k: 0 for k in MOVES}
    out.update(rejected_topology=0, root_to_parent=0, root_to_sibling=0, root_restored=0, write=0, topology=0)
    for rec in records:
        out[rec["move"]] += 1
        out["topology"] += rec["move"] in TOPOLOGY_MOVES
        out["write"] += bool(rec["write"])
        out["rejected_topology"] += rec["move"] in TOPOLOGY_MOVES and not rec["accept"]
        if rec["move"] == "prune":
            snap, before, p = tree.snapshot(), tree.root, tree.parent[rec["i"]]
            apply_move(tree, rec)
            if tree.root != before:
                if not rec["accept"]:
                    out["root_restored"] += 1
                elif tree.root == p:
                    out["root_to_parent"] += 1
                else:
                    out["root_to_sibling"] += 1
            if not rec["accept"]:
                tree.put_back(snap)
        elif rec["accept"]:
            apply_move(tree, rec)
    return out


def dump(path, shape, seed, scheme, records):
    with open(path, "w") as fh:
        json.dump({"shape": list(shape), "seed": seed, "scheme": scheme, "records": records}, fh)


def load(path):
    with open(path) as fh:
        d = json.load(fh)
    return tuple(d["shape"]), d["seed"], d["scheme"], d["records"]


def describe(rec):
    args = ", ".join("%s=%s" % (k, rec[k]) for k in ("node", "i", "j", "height", "factor") if k in rec)
    return "%s(%s) %s" % (rec["move"], args, "accepted" if rec["accept"] else "rejected")


# ---- the driver -------------------------------------------------------------------------------------------------------------------------
class BufferIndexHelper:
    """src/dr/evomodel/treedatalikelihood/BufferIndexHelper.java:40-116, as tools/host/tree_likelihood.cpp restates it"""

    def __init__(self, max_index, min_index):
        self.min, self.dbl = min_index, max_index - min_index
        self.offsets, self.stored, self.flipped = [0] * self.dbl, [0] * self.dbl, [False] * self.dbl

    def buffer_count(self):
        return 2 * self.dbl + self.min

    def flip(self, i):
        k = i - self.min
        if not self.flipped[k]:                              # only once before accept / reject
            self.offsets[k] = self.dbl - self.offsets[k]
            self.flipped[k] = True

    def index(self, i):
        return i if i < self.min else self.offsets[i - self.min] + i

    def store(self):
        self.flipped = [False] * self.dbl
        self.stored = list(self.offsets)

    def restore(self):
        self.offsets, self.stored = self.stored, self.offsets
        self.flipped = [False] * self.dbl


def create(shape, factory, gradients=False, **kw):
    """An instance with the stand-in's buffer counts (btlCreate), the shape's tip states (all compact) and pattern weights.  gradients:
    a pre-order partials buffer per node behind the post-order ones and a differential matrix slot behind the branch matrices
    (beast_mcmc_amd/gradient.py's buffer plan over the stand-in's two flips)."""
    wl = workload(shape)
    T, N = wl.tree.tip_count, wl.tree.node_count
    extra_partials, extra_matrices = (N, 1) if gradients else (0, 0)
    S, C, P = wl.state_count, len(wl.cat_rates), wl.tip_states.shape[1]
    b = factory(T, T + 2 * (N - T) + extra_partials, T, S, P, 2, 2 * N + extra_matrices, C, 2 * (N - T + 1), **kw)
    for t in range(T):
        b.setTipStates(t, np.asarray(wl.tip_states[t], dtype=np.int32))
    b.setPatternWeights(wl.weights)
    return b


class Driver:
    """tools/host/tree_likelihood.cpp TreeLikelihood over `b`, with a tree that changes.  ``step(rec)`` runs one record:
    storeState, the move, one evaluation, accept or reject, the record's reads."""

    def __init__(self, b, shape, scheme, delay_rescaling=False, frequency=RESCALING_FREQUENCY):
        wl = workload(shape)
        self.b, self.wl = b, wl
        self.tree = initial_tree(shape)
        T, N = self.tree.tip_count, self.tree.node_count
        self.T, self.N, self.internal = T, N, N - T
        self.scheme, self.delay, self.frequency = scheme, delay_rescaling, frequency
        self.partial_helper = BufferIndexHelper(N, T)
        self.scale_helper = BufferIndexHelper(self.internal + 1, 0)
        self.matrix_helper = BufferIndexHelper(N, 0)
        self.eigen_helper = BufferIndexHelper(1, 0)
        self.scale_indices, self.stored_scale_indices = [0] * self.internal, [0] * self.internal
        self.update_node = [True] * N
        self.update_substitution_model = self.update_site_model = True
        self.rescaling_count = self.rescaling_count_inner = 0
        self.ever_underflowed = self.use_scale_factors = self.recompute_scale_factors = False
        self.cat_rates = [float(x) for x in wl.cat_rates]
        self.log_likelihood = self.stored_log_likelihood = float("nan")
        self.traversal = REVERSE_LEVEL_ORDER
        self.operations, self.branch_nodes, self.branch_lengths = [], [], []
        self.evaluations = self.write_evaluations = 0
        self.closed_lists = {}                                # a full evaluation's operation list -> times sent
        self.last_write = False
        self.evaluated_root = self.tree.root
        self.cherry_sets = set()                              # the sets of nodes over two tips that a gradient was taken on

    # -- traversal (runTraversal): branches in pre-order, operations in post-order or by level, deepest first
    def _orders(self):
        tree, pre, post, depth = self.tree, [], [], [0] * self.N
        stack = [(tree.root, 0)]
        pre.append(tree.root)
        while stack:
            node, k = stack.pop()
            if node < self.T or k == 2:
                post.append(node)
                continue
            stack.append((node, k + 1))
            c = tree.left[node] if k == 0 else tree.right[node]
            depth[c] = depth[node] + 1
            pre.append(c)
            stack.append((c, 0))
        return pre, post, depth

    def run_traversal(self, flip):
        tree = self.tree
        pre, post, depth = self._orders()
        updated = [False] * self.N
        self.branch_nodes, self.branch_lengths = [], []
        for node in pre:
            if tree.parent[node] >= 0 and self.update_node[node]:
                length = tree.height[tree.parent[node]] - tree.height[node]
                assert length > 0.0, (node, length)
                if flip:
                    self.matrix_helper.flip(node)
                self.branch_nodes.append(node)
                self.branch_lengths.append(length)
                updated[node] = True
        ops = []
        for node in post:
            if node < self.T:
                continue
            c1, c2 = tree.left[node], tree.right[node]
            if not (updated[c1] or updated[c2]):
                continue
            updated[node] = True
            if flip:
                self.partial_helper.flip(node)
            write = read = NONE
            if self.use_scale_factors:
                n = node - self.T
                if self.recompute_scale_factors:
                    self.scale_helper.flip(n)
                    self.scale_indices[n] = self.scale_helper.index(n)
                    write = self.scale_indices[n]
                else:
                    read = self.scale_indices[n]
            ops.append((depth[node], [self.partial_helper.index(node), write, read, self.partial_helper.index(c1), self.matrix_helper.index(c1),
                                      self.partial_helper.index(c2), self.matrix_helper.index(c2)]))
        if self.traversal != POST_ORDER:
            ops.sort(key=lambda x: -x[0])                    # (stable: a level's operations stay in post-order)
        self.operations = [op for _, op in ops]

    def update_all_nodes(self):
        self.update_node = [True] * self.N

    def prepare(self):
        self.recompute_scale_factors = False
        if not self.delay or self.ever_underflowed:
            if self.scheme == SCHEME_ALWAYS:
                self.use_scale_factors = self.recompute_scale_factors = True
            elif self.scheme == SCHEME_DYNAMIC:
                self.use_scale_factors = True
                if self.rescaling_count > self.frequency:
                    self.rescaling_count = self.rescaling_count_inner = 0
                if self.rescaling_count_inner < 1:
                    self.recompute_scale_factors = True
                    self.update_all_nodes()
                    self.rescaling_count_inner += 1
                self.rescaling_count += 1
        if self.scheme == SCHEME_NONE:
            self.use_scale_factors = self.recompute_scale_factors = False
        self.run_traversal(True)
        b, eig = self.b, self.wl.eig
        if self.update_substitution_model:
            self.eigen_helper.flip(0)
            b.setEigenDecomposition(self.eigen_helper.index(0), eig.evec, eig.ievc, eig.evals)
        if self.update_site_model:
            b.setCategoryRates(self.cat_rates)
        if self.branch_nodes:
            b.updateTransitionMatrices(self.eigen_helper.index(0), [self.matrix_helper.index(n) for n in self.branch_nodes], None, None,
                                       self.branch_lengths, len(self.branch_nodes))
        self.first_rescale_attempt = True

    def attempt(self):
        b = self.b
        flat = [x for op in self.operations for x in op]
        b.updatePartials(flat, len(self.operations), NONE)
        if len(self.operations) == self.internal:
            key = tuple(flat)
            self.closed_lists[key] = self.closed_lists.get(key, 0) + 1
        cum = NONE
        if self.use_scale_factors:
            if self.recompute_scale_factors:
                self.scale_helper.flip(self.internal)
                cum = self.scale_helper.index(self.internal)
                b.resetScaleFactors(cum)
                b.accumulateScaleFactors(self.scale_indices, self.internal, cum)
            else:
                cum = self.scale_helper.index(self.internal)
        b.setCategoryWeights(0, self.wl.cat_weights)
        b.setStateFrequencies(0, self.wl.freqs)
        out = [0.0]
        b.calculateRootLogLikelihoods([self.partial_helper.index(self.tree.root)], [0], [0], [cum], 1, out)
        self.evaluated_root = self.tree.root
        self.evaluations += 1
        return float(out[0])

    def finish(self, value):
        """-> (done, value)"""
        if np.isnan(value) or np.isinf(value):
            self.ever_underflowed = True
            value = float("-inf")
            if self.first_rescale_attempt and self.delay and self.scheme != SCHEME_NONE:
                self.use_scale_factors = self.recompute_scale_factors = True
                self.update_all_nodes()
                self.run_traversal(False)                    # the failed attempt's buffers are overwritten; the scale indices flip
                self.first_rescale_attempt = False
                return False, value
        self.update_node = [False] * self.N
        self.update_substitution_model = self.update_site_model = False
        return True, value

    def evaluate(self):
        self.prepare()
        self.last_write = self.recompute_scale_factors
        self.write_evaluations += self.last_write
        while True:
            done, value = self.finish(self.attempt())
            if done:
                self.log_likelihood = value
                return value

    def store_state(self):
        for h in (self.partial_helper, self.matrix_helper, self.eigen_helper):
            h.store()
        if self.use_scale_factors:
            self.scale_helper.store()
            self.stored_scale_indices = list(self.scale_indices)
        self.stored_log_likelihood = self.log_likelihood

    def restore_state(self):
        self.update_site_model = True
        for h in (self.partial_helper, self.matrix_helper, self.eigen_helper):
            h.restore()
        if self.use_scale_factors:
            self.scale_helper.restore()
            self.scale_indices, self.stored_scale_indices = self.stored_scale_indices, self.scale_indices
        self.log_likelihood = self.stored_log_likelihood

    # -- gradients behind the current topology (beast_mcmc_amd/gradient.py BranchGradient.gradient for a tree that changes): the root's
    # pre-order partial, the whole-tree pre-order list over the current flips, and calculateEdgeDifferentials on every branch
    def pre_buffer(self, node):
        return self.T + 2 * self.internal + node

    def cherries(self):
        return frozenset(n for n in range(self.T, self.N) if self.tree.left[n] < self.T and self.tree.right[n] < self.T)

    def gradient(self):
        """-> the edge sums d lnL / d t of every branch of the current tree, by node number (needs an instance made with gradients=True;
        unscaled chains only)"""
        assert not self.use_scale_factors
        b, tree, wl = self.b, self.tree, self.wl
        P, C = wl.tip_states.shape[1], len(self.cat_rates)
        b.setPartials(self.pre_buffer(tree.root), np.tile(wl.freqs, P * C))
        ops, stack = [], [tree.root]
        while stack:
            n = stack.pop()
            if n < self.T:
                continue
            l, r = tree.left[n], tree.right[n]
            for child, sib in ((l, r), (r, l)):
                ops += [self.pre_buffer(child), NONE, NONE, self.pre_buffer(n), self.matrix_helper.index(child),
                        self.partial_helper.index(sib), self.matrix_helper.index(sib)]
            stack += [r, l]
        b.updatePrePartials(ops, len(ops) // 7, NONE)
        e = wl.eig
        q = (np.asarray(e.evec) * np.asarray(e.evals)[None, :]) @ np.asarray(e.ievc)
        q_index = 2 * self.N
        b.setDifferentialMatrix(q_index, np.concatenate([(q * r).ravel() for r in self.cat_rates]))
        edges = [n for n in range(self.N) if n != tree.root]
        s1, _, _ = b.calculateEdgeDifferentials([self.partial_helper.index(n) for n in edges], [self.pre_buffer(n) for n in edges],
                                                [q_index] * len(edges), [0], len(edges), want_squared=False)
        out = np.zeros(self.N)
        out[edges] = s1
        return out

    def read_pre_partials(self):
        return [("partials", self.b.getPartials(self.pre_buffer(n), NONE).copy()) for n in range(self.N)]

    # -- the chain
    def node_buffer(self, node):
        return self.partial_helper.index(node)

    def cumulative_scale(self):
        return self.scale_helper.index(self.internal) if self.use_scale_factors else NONE

    def read_nodes(self, every=1):
        """every current node buffer, unscaled, and every current scale buffer with the cumulative one"""
        nodes = list(range(self.T, self.N))[::every]
        reads = [("partials", self.b.getPartials(self.node_buffer(n), NONE).copy()) for n in nodes]
        if self.use_scale_factors:
            reads += [("scale", self.b.getLogScaleFactors(self.scale_indices[n - self.T]).copy()) for n in nodes]
            reads.append(("scale", self.b.getLogScaleFactors(self.cumulative_scale()).copy()))
        return reads

    def initial(self):
        """the evaluation before the chain -> reads"""
        return [("sum", np.array([self.evaluate()]))]

    def step(self, rec, skip_restore=False, node_stride=1, gradients=False):
        """-> reads: lnL of the proposal, then — after accept / reject — what the record asks for.  skip_restore: a rejected move's
        restoreState is left out (the negative control of tests/test_topology_chains_host.py).  gradients: the edge sums of the
        current tree ("deriv") where the record says "gradient" — every fourth proposal, accepted or rejected — and with the end
        state every pre-order partial."""
        self.store_state()
        snap, rates = self.tree.snapshot(), list(self.cat_rates)
        if rec["move"] == "model":
            self.cat_rates = [r * rec["factor"] for r in self.cat_rates]
            self.update_substitution_model = self.update_site_model = True
            self.update_all_nodes()
        else:
            parent_changed, children_changed = apply_move(self.tree, rec)
            for n in parent_changed:
                self.update_node[n] = True
            for n in children_changed:                       # updateNodeAndChildren
                self.update_node[n] = True
                if n >= self.T:
                    self.update_node[self.tree.left[n]] = self.update_node[self.tree.right[n]] = True
        self.traversal = REVERSE_LEVEL_ORDER if rec["level"] else POST_ORDER
        reads = [("sum", np.array([self.evaluate()]))]
        assert self.delay or self.last_write == bool(rec["write"]), (self.last_write, rec["write"])      # (the generator's account of the policy)
        if not rec["accept"]:
            self.tree.put_back(snap)
            self.cat_rates = rates
            if not skip_restore:
                self.restore_state()
        if "site" in rec["reads"]:
            reads.append(("site", self.b.getSiteLogLikelihoods().copy()))
        if "nodes" in rec["reads"]:
            reads += self.read_nodes(node_stride)
        if gradients and rec["gradient"]:
            reads.append(("deriv", self.gradient()))
            self.cherry_sets.add(self.cherries())
            if rec["last"]:
                reads += self.read_pre_partials()
        return reads


def run_step(driver, rec, first=False, **kw):
    """-> (return code, reads): a BeagleException's code instead of the exception, as a caller sees it"""
    try:
        return 0, (driver.initial() if first else driver.step(rec, **kw))
    except Exception as e:                                    # (BeagleException: the binding class is the caller's)
        if hasattr(e, "code"):
            return int(e.code), []
        raise


def deviation(kind, got, want):
    """The error of a read, normalised so that the bound is 1e-10 for every kind (tests/call_sequences.py deviation): sums and site
    values relative, log scale factors relative against max(1, |value|), node partials and pre-order partials against each pattern's
    largest entry, edge sums of derivatives against max(1, the largest of them)."""
    got, want = np.asarray(got, dtype=float), np.asarray(want, dtype=float)
    if got.shape != want.shape:
        return float("inf")
    if not (np.isfinite(got).all() and np.isfinite(want).all()):
        return float("nan")
    if kind in ("sum", "site"):
        return float(np.max(np.abs(got - want) / np.maximum(np.abs(want), 1e-300)))
    if kind == "scale":
        return float(np.max(np.abs(got - want) / np.maximum(np.abs(want), 1.0)))
    if kind == "partials":
        scale = np.maximum(np.abs(want).max(axis=(0, 2), keepdims=True), 1e-300)
        return float(np.max(np.abs(got - want) / scale))
    if kind == "deriv":                                       # tests/test_gpu_gradients.py ``close``
        return float(np.max(np.abs(got - want)) / max(1.0, float(np.max(np.abs(want)))))
    raise ValueError(kind)


def replay(path, out=print):
    """Engine and oracle side by side; prints the first diverging read.  -> the step it stopped at, or None"""
    import os
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    for p in (here, os.path.dirname(here)):
        if p not in sys.path:
            sys.path.insert(0, p)
    import beast_mcmc_amd as bm
    import helpers
    shape, seed, scheme, records = load(path)
    eng, ora = create(shape, bm.beagle.Beagle), create(shape, bm.beagle.Beagle, library=helpers.oracle_library())
    try:
        de, do = Driver(eng, shape, scheme), Driver(ora, shape, scheme)
        for step, rec in enumerate([None] + records):
            (rc_e, got), (rc_o, want) = run_step(de, rec, first=rec is None), run_step(do, rec, first=rec is None)
            what = "the evaluation before the chain" if rec is None else describe(rec)
            if rc_e or rc_o:
                out("step %d %s: return codes engine %d, oracle %d" % (step - 1, what, rc_e, rc_o))
                return step - 1
            worst = max([deviation(k, g, w) for (k, g), (_, w) in zip(got, want)] + [0.0], key=lambda x: (x != x, x))
            if not worst <= BOUND:
                out("step %d %s: first diverging read, deviation %.3e (bound %.0e)" % (step - 1, what, worst, BOUND))
                return step - 1
        out("shape %s seed %d scheme %s: no read diverges in %d steps" % (shape, seed, SCHEME_NAMES[scheme], len(records)))
        return None
    finally:
        eng.finalize()
        ora.finalize()


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser(description="replay a recorded topology chain on the engine and the oracle")
    ap.add_argument("--replay", required=True, metavar="FILE")
    replay(ap.parse_args().replay)
