"""Host restatement of marginal node state posteriors (include/beagle_mi355.h beagleMi355NodePosteriors) in numpy.

Three independent routes to P(state of node i = s | pattern):

``posteriors`` / ``category_posteriors``  the call's own arithmetic over a pre-order and a post-order partial per row, in the order the
    header states — m[s] = sum_c (pre_c * post_c) * w_c with c upwards from 0.0 and every product rounded on its own, Z = sum_s m[s]
    with s upwards from 0.0, m[s] / Z — in float64 (what the device agrees with bit for bit) or, as the yardstick, np.longdouble.
``forward_backward``  NodePosteriorTreeLikelihood.traverseForward / calculatePosteriors
    (src/dr/oldevomodel/treelikelihood/NodePosteriorTreeLikelihood.java:119-235) from tip partials and branch matrices: the pruning
    pass, forwardProbs down the tree by accumulateMatrixMultiply and matrixMultiplyBackward, the product with the node's partials.
    The reference reads one category's matrices; here every category goes the same way and the call's arithmetic joins them.
``enumerate_marginals``  the definition: the sum over every assignment of states to the internal nodes.
"""
import itertools

import numpy as np


def expand_states(states, S, C):
    """uint/int states [P] -> partials [C, P, S]: the unit vector of the state, all ones for a state >= S."""
    states = np.asarray(states).astype(np.int64)
    x = np.zeros((len(states), S))
    known = states < S
    x[np.nonzero(known)[0], states[known]] = 1.0
    x[~known] = 1.0
    return np.broadcast_to(x, (C,) + x.shape).copy()


def posteriors(pre, post, category_weights, dtype=np.float64):
    """pre, post [R, C, P, S] -> (posterior [R, P, S], Z [R, P], bad [R, P]): NaN where Z is 0 or not finite."""
    pre, post = np.asarray(pre, dtype=dtype), np.asarray(post, dtype=dtype)
    w = np.asarray(category_weights, dtype=dtype)
    R, C, P, S = pre.shape
    m = np.zeros((R, P, S), dtype=dtype)
    for c in range(C):
        m = m + (pre[:, c] * post[:, c]) * w[c]
    z = np.zeros((R, P), dtype=dtype)
    for s in range(S):
        z = z + m[:, :, s]
    bad = ~(np.isfinite(z) & (z != 0))
    with np.errstate(divide="ignore", invalid="ignore"):
        out = m / np.where(bad, np.nan, z)[:, :, None]
    return out, z, bad


def map_states(posterior):
    """-> (states uint8 [R, P], probabilities [R, P]): the first s with the strictly largest posterior; state 0 on a NaN row."""
    best = np.zeros(posterior.shape[:2], dtype=np.int64)
    value = posterior[:, :, 0].copy()
    for s in range(1, posterior.shape[2]):
        better = posterior[:, :, s] > value
        best[better] = s
        value = np.where(better, posterior[:, :, s], value)
    return best.astype(np.uint8), value


def category_posteriors(pre, post, category_weights, dtype=np.float64):
    """pre, post [C, P, S] of one row -> [P, C]: n_c = (sum_s pre_c * post_c) * w_c, s upwards from 0.0; n_c / sum_c n_c, c upwards."""
    pre, post = np.asarray(pre, dtype=dtype), np.asarray(post, dtype=dtype)
    w = np.asarray(category_weights, dtype=dtype)
    C, P, S = pre.shape
    n = np.zeros((C, P), dtype=dtype)
    for s in range(S):
        n = n + pre[:, :, s] * post[:, :, s]
    n = n * w[:, None]
    d = np.zeros(P, dtype=dtype)
    for c in range(C):
        d = d + n[c]
    bad = ~(np.isfinite(d) & (d != 0))
    with np.errstate(divide="ignore", invalid="ignore"):
        return (n / np.where(bad, np.nan, d)[None, :]).T.copy()


def state_totals(posterior, pattern_weights, dtype=np.longdouble):
    """[R, P, S] -> [R, S]: sum_p weight_p posterior[p][s]."""
    post = np.asarray(posterior, dtype=dtype)
    w = np.asarray(pattern_weights, dtype=dtype)
    return (post * w[None, :, None]).sum(axis=1)


def state_totals_in_device_order(posterior, pattern_weights):
    """The float64 totals as the header forms them: per 64 patterns v[i] += v[i + off] for off = 32, 16 .. 1 (patterns past the end
    0.0), then those sums in ascending order from 0.0."""
    post = np.asarray(posterior, dtype=np.float64)
    R, P, S = post.shape
    blocks = (P + 63) // 64
    v = np.zeros((R, blocks * 64, S))
    v[:, :P] = np.asarray(pattern_weights, dtype=np.float64)[None, :, None] * post
    v = v.reshape(R, blocks, 64, S)
    off = 32
    while off:
        v = v[:, :, :off] + v[:, :, off:2 * off]
        off //= 2
    out = np.zeros((R, S))
    for b in range(blocks):
        out = out + v[:, b, 0]
    return out


# ---- from the tree ------------------------------------------------------------------------------------------------------------
def branch_matrices(wl, dtype=np.float64):
    """node -> [C, S, S] transition matrices of its branch from the workload's eigen system (None at the root)."""
    tr, e = wl.tree, wl.eig
    out = {}
    for n in range(tr.node_count):
        if n == tr.root:
            out[n] = None
            continue
        t = tr.branch_length(n)
        out[n] = np.stack([(e.evec * np.exp(e.evals * r * t)[None, :]) @ e.ievc for r in wl.cat_rates]).astype(dtype)
    return out


def tip_partials(wl):
    return {t: expand_states(wl.tip_states[t], wl.state_count, wl.category_count) for t in range(wl.tree.tip_count)}


def forward_backward(tree, tips, matrices, freqs, dtype=np.float64):
    """-> (post, pre): node -> [C, P, S].  post by pruning; pre = forwardProbs after the node's own branch (what it multiplies its
    partials by): the root's are the frequencies, a child's matrixMultiplyBackward(P_child, forward(parent) * P_sib post(sib))."""
    post = {t: np.asarray(x, dtype=dtype) for t, x in tips.items()}
    for n in tree.postorder():
        if n < tree.tip_count:
            continue
        l, r = int(tree.left[n]), int(tree.right[n])
        post[n] = np.einsum("cij,cpj->cpi", matrices[l], post[l]) * np.einsum("cij,cpj->cpi", matrices[r], post[r])
    C, P, S = post[tree.root].shape
    pre = {tree.root: np.broadcast_to(np.asarray(freqs, dtype=dtype), (C, P, S)).copy()}
    stack = [tree.root]
    while stack:
        n = stack.pop()
        if n < tree.tip_count:
            continue
        l, r = int(tree.left[n]), int(tree.right[n])
        for child, sib in ((l, r), (r, l)):
            f = np.einsum("cij,cpj->cpi", matrices[sib], post[sib]) * pre[n]               # accumulateMatrixMultiply
            pre[child] = np.einsum("cji,cpj->cpi", matrices[child], f)                     # matrixMultiplyBackward
        stack += [r, l]
    return post, pre


def restatement(wl, tips=None, dtype=np.float64):
    """Every node's posterior [N, P, S] the reference's way, plus the (pre, post) stacks [N, C, P, S] it was formed from."""
    tr = wl.tree
    post, pre = forward_backward(tr, tip_partials(wl) if tips is None else tips, branch_matrices(wl, dtype), wl.freqs, dtype)
    pre_s = np.stack([pre[n] for n in range(tr.node_count)])
    post_s = np.stack([post[n] for n in range(tr.node_count)])
    return posteriors(pre_s, post_s, wl.cat_weights, dtype)[0], pre_s, post_s


def enumerate_marginals(wl, tips=None):
    """[N, P, S] by the definition, in np.longdouble: the joint probability of the pattern and an assignment of states to the
    internal nodes, summed over the assignments (and, weighted, over the categories), normalised per node."""
    tr = wl.tree
    T, N, S, C = tr.tip_count, tr.node_count, wl.state_count, wl.category_count
    ld = np.longdouble
    tips = tip_partials(wl) if tips is None else tips
    mats = branch_matrices(wl, ld)
    P = tips[0].shape[1]
    freqs = np.asarray(wl.freqs, dtype=ld)
    cw = np.asarray(wl.cat_weights, dtype=ld)
    joint = np.zeros((N, P, S), dtype=ld)
    internal = list(range(T, N))
    for c in range(C):
        for assignment in itertools.product(range(S), repeat=len(internal)):
            a = dict(zip(internal, assignment))
            base = freqs[a[tr.root]] * cw[c]
            for n in internal:
                if n != tr.root:
                    base = base * mats[n][c, a[int(tr.parent[n])], a[n]]
            g = [mats[t][c, a[int(tr.parent[t])], :][None, :] * np.asarray(tips[t][c], dtype=ld) for t in range(T)]      # [P, S] per tip
            factor = [x.sum(axis=1) for x in g]
            everything = base * np.prod(np.stack(factor), axis=0)                                                    # [P]
            for n in internal:
                joint[n, :, a[n]] += everything
            for t in range(T):
                others = base * np.prod(np.stack([factor[u] for u in range(T) if u != t]), axis=0)
                joint[t] += others[:, None] * g[t]
    return joint / joint.sum(axis=2)[:, :, None]
