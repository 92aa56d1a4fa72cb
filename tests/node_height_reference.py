"""Host restatement of DiscreteTraitNodeHeightDelegate.getNodeDerivatives
(src/dr/evomodel/treedatalikelihood/discrete/DiscreteTraitNodeHeightDelegate.java:63-200) in numpy.

It works the reference's way: from the post-order AND the pre-order partial of every node and the branch matrix of every branch, as
getPartials / getTransitionMatrix of some engine library hand them over, plus the rate-scaled infinitesimal matrix of every branch.
Per branch n (:126-134) the per-pattern first derivative and diagonal second derivative in the branch length are
    g_n = <pre(n) . Q_n post(n)> / <pre(n) . post(n)>,   h_n = <pre(n) . Q_n Q_n post(n)> / <pre(n) . post(n)> - g_n^2
with <.> the sum over states and, weighted, over rate categories; per internal node i with children j, k (:137-197) the mixed terms are
    h_jk = <(Q_j P_j post(j)) (Q_k P_k post(k)) pre(i)> / <(P_j post(j)) (P_k post(k)) pre(i)> - g_j g_k
    h_ij = <(Q_j P_j post(j)) (P_k post(k)) (Q_i^T pre(i))> / <(P_j post(j)) (P_k post(k)) pre(i)> - g_j g_i     (h_ik likewise)
and the node's derivatives are the pattern-weighted sums of
    first  = r_j g_j + r_k g_k - r_i g_i                                                                        (:69-85)
    second = r_j^2 h_j + r_k^2 h_k + 2 r_j r_k h_jk + r_i^2 h_i - 2 r_i r_j h_ij - 2 r_i r_k h_ik                (:159-193)
(no i terms at the root).  Compact tips are expanded here: the unit vector of the state, all ones for a state >= stateCount.
"""
import numpy as np


def _mv(M, x):          # [C,S,S] . [C,P,S] -> [C,P,S]: y_i = sum_j M[i][j] x_j   (getMatrixVectorProduct)
    return np.einsum("cij,cpj->cpi", M, x)


def _mtv(M, x):         # y_i = sum_j M[j][i] x_j   (getMatrixTransformVectorProduct)
    return np.einsum("cji,cpj->cpi", M, x)


def expand_states(states, S, C):
    """uint/int states [P] -> partials [C, P, S]."""
    states = np.asarray(states).astype(np.int64)
    x = np.zeros((len(states), S))
    known = states < S
    x[np.nonzero(known)[0], states[known]] = 1.0
    x[~known] = 1.0
    return np.broadcast_to(x, (C,) + x.shape).copy()


def node_derivatives(tree, post_of, pre_of, matrix_of, q_of, rates, category_weights, pattern_weights, second=True):
    """post_of(n), pre_of(n) -> [C, P, S] for EVERY node n; matrix_of(n), q_of(n) -> [C, S, S] for every non-root node;
    rates[n]: branch rate.  -> (first, second) over the internal nodes in node order (second None when not asked for)."""
    cw = np.asarray(category_weights, dtype=float)
    pw = np.asarray(pattern_weights, dtype=float)
    N, T, root = tree.node_count, tree.tip_count, tree.root

    def red(v):                                        # sum over states, weighted sum over categories -> [P]
        return np.einsum("c,cp->p", cw, v.sum(axis=2))

    post = {n: post_of(n) for n in range(N)}
    pre = {n: pre_of(n) for n in range(N)}
    g, h = {}, {}
    for n in range(N):
        if n == root:
            continue
        Q = q_of(n)
        qx = _mv(Q, post[n])
        den = red(post[n] * pre[n])
        g[n] = red(pre[n] * qx) / den
        if second:
            h[n] = red(pre[n] * _mv(Q, qx)) / den - g[n] * g[n]
    first = np.zeros(N - T)
    sec = np.zeros(N - T) if second else None
    for r, i in enumerate(range(T, N)):
        j, k = int(tree.left[i]), int(tree.right[i])
        rj, rk = rates[j], rates[k]
        f = rj * g[j] + rk * g[k]
        if i != root:
            f = f - rates[i] * g[i]
        first[r] = float(np.dot(pw, f))
        if not second:
            continue
        aj, ak = _mv(matrix_of(j), post[j]), _mv(matrix_of(k), post[k])
        bj, bk = _mv(q_of(j), aj), _mv(q_of(k), ak)
        den = red(aj * ak * pre[i])
        hjk = red(bj * bk * pre[i]) / den - g[j] * g[k]
        s = rj * rj * h[j] + rk * rk * h[k] + 2.0 * rj * rk * hjk
        if i != root:
            ri = rates[i]
            u = _mtv(q_of(i), pre[i])
            hij = red(bj * ak * u) / den - g[j] * g[i]
            hik = red(bk * aj * u) / den - g[k] * g[i]
            s = s + ri * ri * h[i] - 2.0 * ri * rj * hij - 2.0 * ri * rk * hik
        sec[r] = float(np.dot(pw, s))
    return first, sec


def row_derivatives(rows, rates, post_of, pre_of, matrix_of, category_weights, pattern_weights, first=True, second=True):
    """The call's own rows, each from the buffers and slots it names and nothing else (include/beagle_mi355.h
    beagleMi355NodeHeightDerivatives: D, g and h as written there), so that it is defined in any state of an instance — ``node_derivatives``
    above wants every node's pre-order partial and agrees with this where the buffers belong to one evaluation.
    rows [n][8] {pre(i), post(j), matrix(j), dmatrix(j), post(k), matrix(k), dmatrix(k), dmatrix(i) or -1}; rates [n][3] {r_j, r_k, r_i};
    post_of(buffer), pre_of(buffer) -> [C, P, S]; matrix_of(slot) -> [C, S, S].  -> (first, second), [n] each, None when not asked for."""
    cw = np.asarray(category_weights, dtype=float)
    pw = np.asarray(pattern_weights, dtype=float)
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, 8)
    rates = np.asarray(rates, dtype=float).reshape(-1, 3)

    def red(v):
        return np.einsum("c,cp->p", cw, v.sum(axis=2))

    o1 = np.zeros(len(rows)) if first else None
    o2 = np.zeros(len(rows)) if second else None
    for n, (row, (rj, rk, ri)) in enumerate(zip(rows, rates)):
        pi_, pj, mj, dj, pk, mk, dk, di = (int(x) for x in row)
        q = pre_of(pi_)
        Qj, Qk = matrix_of(dj), matrix_of(dk)
        aj, ak = _mv(matrix_of(mj), post_of(pj)), _mv(matrix_of(mk), post_of(pk))
        bj, bk = _mv(Qj, aj), _mv(Qk, ak)
        D = red(aj * ak * q)
        gj, gk = red(bj * ak * q) / D, red(aj * bk * q) / D
        f = rj * gj + rk * gk
        if di >= 0:
            u = _mtv(matrix_of(di), q)
            gi = red(aj * ak * u) / D
            f = f - ri * gi
        if first:
            o1[n] = float(np.dot(pw, f))
        if not second:
            continue
        hjj = red(_mv(Qj, bj) * ak * q) / D - gj * gj
        hkk = red(aj * _mv(Qk, bk) * q) / D - gk * gk
        hjk = red(bj * bk * q) / D - gj * gk
        s = rj * rj * hjj + rk * rk * hkk + 2.0 * rj * rk * hjk
        if di >= 0:
            v = _mtv(matrix_of(di), u)
            hii = red(aj * ak * v) / D - gi * gi
            hij = red(bj * ak * u) / D - gi * gj
            hik = red(aj * bk * u) / D - gi * gk
            s = s + ri * ri * hii - 2.0 * ri * rj * hij - 2.0 * ri * rk * hik
        o2[n] = float(np.dot(pw, s))
    return o1, o2


def from_plan(plan, second=True, compact=None):
    """`node_derivatives` over what the engine library behind `plan` (a nodeheight.NodeHeightGradient after prepare()) reads back.
    compact: the tips that hold compact states (default: all of them), expanded from the workload's states."""
    b, C, S, T = plan.b, plan.C, plan.S, plan.T
    compact = set(range(T)) if compact is None else set(compact)
    q = b.getTransitionMatrix(plan.q_index).reshape(C, S, S)

    def post_of(n):
        if n in compact:
            return expand_states(plan.wl.tip_states[n], S, C)
        return b.getPartials(plan.post_index(n), -1).reshape(C, plan.P, S)

    return node_derivatives(plan.tree, post_of, lambda n: b.getPartials(plan.pre_offset + n, -1).reshape(C, plan.P, S),
                            lambda n: b.getTransitionMatrix(plan.matrix_index(n)).reshape(C, S, S), lambda n: q,
                            plan.rates, plan.wl.cat_weights, plan.wl.weights, second=second)
