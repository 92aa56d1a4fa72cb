"""Host restatements of the BASTA gradient, for the tests of beagleBastaGradient and ``BastaLikelihood.gradient``.  numpy only;
every function takes a ``dtype`` so that the same code runs in fp64 and in numpy.longdouble.

  adjoint            the reverse sweep beagleBastaGradient runs (include/beagle_mi355.h states the rule), every sum and product in the
                     device's order: in fp64 the adjoints and both gradients are the device's bit for bit
  forward            the reference's forward mode on zeroed storage, loop for loop (src/dr/evomodel/coalescent/basta/
                     GenericBastaLikelihoodDelegate.java: peelPartialsGrad :443-534, peelPopSizeSGrad :536-603, reduceWithinIntervalGrad
                     :680-753, reduceAcrossIntervalsGrad / ...GradPopSize :622-678).  O(N S^4): small cases only
  finite_difference  central differences of the likelihood restatement (basta_reference.update / accumulate), meant for longdouble

All three return the reference's intermediates: ``theta`` [S] (with respect to 1 / size) and ``migration`` [S][S] (W[a][b]: row b of
every stored matrix m += t_m * row a).  ``distances[k]`` is t of list interval k.
"""
import numpy as np

import basta_reference as br


def _cast(partials, matrices, sizes, coalescent, lengths, distances, dtype):
    dt = np.dtype(dtype)
    mats = {m: np.asarray(x).astype(dt) for m, x in matrices.items()}
    return (dt, np.asarray(partials).astype(dt), mats, np.asarray(sizes).astype(dt), np.asarray(coalescent).astype(dt),
            np.asarray(lengths).astype(dt), None if distances is None else np.asarray(distances).astype(dt))


def _interval_of(intervals, n):
    out = np.zeros(n, dtype=np.int64)
    for k in range(len(intervals) - 1):
        out[intervals[k]:intervals[k + 1]] = k
    return out


def within(partials, ops, intervals, lengths, sizes, coalescent):
    """e, f, g, h [interval number][S] as beagleBastaAccumulatePartials forms them"""
    keep = {}
    br.accumulate(partials, ops, intervals, lengths, sizes, coalescent, np.zeros(1, dtype=partials.dtype), keep)
    return keep["e"], keep["f"], keep["g"], keep["h"]


def column_products(matrix, x):
    """out_j = sum_i matrix[i][j] x_i, i in index order"""
    out = np.zeros_like(x)
    for i in range(matrix.shape[0]):
        out = out + matrix[i] * x[i]
    return out


def adjoint(ops, intervals, lengths, distances, partials, matrices, sizes, coalescent, dtype=np.float64):
    """``partials`` [buffer][S], ``matrices`` {number: S x S} and ``coalescent`` as beagleBastaUpdatePartials left them.
    -> {"adjoints": [buffer][S], "theta": [S], "migration": [S][S] (zeros without distances), "w": {operation: w}}"""
    dt, v, mats, sizes, prob, lengths, distances = _cast(partials, matrices, sizes, coalescent, lengths, distances, dtype)
    one, half, quarter = dt.type(1.0), dt.type(0.5), dt.type(0.25)
    n, s = len(ops), v.shape[1]
    e, f, g, h = within(v, ops, intervals, lengths, sizes, prob)
    interval_of = _interval_of(intervals, n)
    theta = one / sizes
    lam = np.zeros_like(v)
    w_of = {}
    for k in range(n - 1, -1, -1):
        dest, in1, m1, in2, m2, acc1, acc2, own_number = (int(x) for x in ops[k])
        iv = interval_of[k]
        number = int(ops[intervals[iv], 7])
        c = (-lengths[iv] * half) * theta
        if in2 < 0:
            lam[dest] = lam[dest] + c * (g[number] - v[dest])
            lam[in1] = column_products(mats[m1], lam[dest]) + c * (e[number] - v[in1])
            continue
        dot = dt.type(0.0)
        for i in range(s):
            dot = dot + lam[dest, i] * v[dest, i]
        with np.errstate(divide="ignore", invalid="ignore"):
            w = ((lam[dest] - dot) + one) / prob[own_number]
        w_of[k] = w
        lam[acc1] = (w * v[acc2]) * theta + c * (g[number] - v[acc1])
        lam[acc2] = (w * v[acc1]) * theta + c * (g[number] - v[acc2])
        lam[in1] = column_products(mats[m1], lam[acc1]) + c * (e[number] - v[in1])
        lam[in2] = column_products(mats[m2], lam[acc2]) + c * (e[number] - v[in2])
    # the two reductions: per interval its operations in list order, then the intervals in index order
    big_w, big_g = np.zeros((s, s), dtype=dt), np.zeros(s, dtype=dt)
    with np.errstate(invalid="ignore"):
        for iv in range(len(intervals) - 1):
            begin, end = int(intervals[iv]), int(intervals[iv + 1])
            part_w, part_g = np.zeros((s, s), dtype=dt), np.zeros(s, dtype=dt)
            if end > begin:
                number = int(ops[begin, 7])
                part_g = (-lengths[iv] * quarter) * (((e[number] * e[number] - f[number]) + g[number] * g[number]) - h[number])
                for k in range(begin, end):
                    for acc in (int(ops[k, 5]), int(ops[k, 6])) if ops[k, 3] >= 0 else (int(ops[k, 5]),):
                        if distances is not None:
                            part_w = part_w + (distances[iv] * v[acc])[:, None] * lam[acc][None, :]
                    if ops[k, 3] >= 0:
                        part_g = part_g + (w_of[k] * v[int(ops[k, 5])]) * v[int(ops[k, 6])]
            big_w = big_w + part_w
            big_g = big_g + part_g
    return {"adjoints": lam, "theta": big_g, "migration": big_w, "w": w_of}


def forward(ops, intervals, lengths, distances, partials, matrices, sizes, coalescent, dtype=np.float64):
    """The Java loops on zeroed gradient storage.  -> {"theta": [S], "migration": [S][S]}"""
    dt, v, mats, sizes, prob, lengths, distances = _cast(partials, matrices, sizes, coalescent, lengths, distances, dtype)
    n, s = len(ops), v.shape[1]
    buffers = v.shape[0]
    e, f, g, h = within(v, ops, intervals, lengths, sizes, prob)
    interval_of = _interval_of(intervals, n)
    numbers = e.shape[0]
    grad = np.zeros((s, s, buffers, s), dtype=dt)            # gradientStorage.partials[a][b]
    grad_j = np.zeros((s, s, numbers), dtype=dt)             # gradientStorage.coalescent[a][b]
    pop = np.zeros((s, buffers, s), dtype=dt)                # gradientStorage.partialsGradPopSize[a]
    pop_j = np.zeros((s, numbers), dtype=dt)
    idx = np.arange(s)

    def rows(matrix, x):                                     # sum_j matrix[i][j] x[..., j], j in index order
        out = np.zeros_like(x)
        for j in range(s):
            out = out + matrix[:, j] * x[..., j:j + 1]
        return out

    for k in range(n):
        dest, in1, m1, in2, m2, acc1, acc2, number = (int(x) for x in ops[k])
        t = distances[interval_of[k]]
        # peelPartialsGrad :476-488
        left = rows(mats[m1], grad[:, :, in1, :])
        left[:, idx, idx] += v[acc1][:, None] * t
        grad[:, :, dest, :] = left
        # peelPopSizeSGrad :553-561
        pop[:, dest, :] = rows(mats[m1], pop[:, in1, :])
        if in2 < 0:
            continue
        big_j = prob[number]
        # :498-531
        right = grad[:, :, acc2, :] + rows(mats[m2], grad[:, :, in2, :])
        right[:, idx, idx] += v[acc2][:, None] * t
        grad[:, :, acc2, :] = right
        entry = (left * v[acc2] + right * v[acc1]) / sizes
        partial_j = np.zeros((s, s), dtype=dt)
        for i in range(s):
            partial_j = partial_j + entry[:, :, i]
        grad[:, :, acc1, :] = left
        grad[:, :, dest, :] = entry / big_j - partial_j[:, :, None] * v[dest] / big_j
        grad_j[:, :, number] = partial_j
        # :572-601
        left_p = pop[:, dest, :].copy()
        right_p = rows(mats[m2], pop[:, in2, :])
        entry = (left_p * v[acc2] + right_p * v[acc1]) / sizes
        entry[idx, idx] += v[acc1] * v[acc2]
        partial_p = np.zeros(s, dtype=dt)
        for i in range(s):
            partial_p = partial_p + entry[:, i]
        pop[:, acc1, :] = left_p
        pop[:, acc2, :] = right_p
        pop[:, dest, :] = entry / big_j - partial_p[:, None] * v[dest] / big_j
        pop_j[:, number] = partial_p
    # reduceWithinIntervalGrad
    ge, gf, gg, gh = (np.zeros((s, s, numbers, s), dtype=dt) for _ in range(4))
    pe, pf, pg, ph = (np.zeros((s, numbers, s), dtype=dt) for _ in range(4))
    for iv in range(len(intervals) - 1):
        for k in range(int(intervals[iv]), int(intervals[iv + 1])):
            number = int(ops[k, 7])
            for start, end in ((int(ops[k, 1]), int(ops[k, 5])), (int(ops[k, 3]), int(ops[k, 6]))):
                if start < 0:
                    continue
                ge[:, :, number] += grad[:, :, start]; gf[:, :, number] += 2 * v[start] * grad[:, :, start]
                gg[:, :, number] += grad[:, :, end]; gh[:, :, number] += 2 * v[end] * grad[:, :, end]
                pe[:, number] += pop[:, start]; pf[:, number] += 2 * v[start] * pop[:, start]
                pg[:, number] += pop[:, end]; ph[:, number] += 2 * v[end] * pop[:, end]
    # reduceAcrossIntervalsGrad / ...GradPopSize
    out_w, out_g = np.zeros((s, s), dtype=dt), np.zeros(s, dtype=dt)
    for iv in range(len(intervals) - 1):
        if intervals[iv + 1] <= intervals[iv]:
            continue
        number = int(ops[intervals[iv], 7])
        total = np.zeros((s, s), dtype=dt)
        total_p = np.zeros(s, dtype=dt)
        for i in range(s):
            total = total + (2 * e[number, i] * ge[:, :, number, i] - gf[:, :, number, i] +
                             2 * g[number, i] * gg[:, :, number, i] - gh[:, :, number, i]) / sizes[i]
            total_p = total_p + (2 * e[number, i] * pe[:, number, i] - pf[:, number, i] +
                                 2 * g[number, i] * pg[:, number, i] - ph[:, number, i]) / sizes[i]
            total_p[i] = total_p[i] + (e[number, i] * e[number, i] - f[number, i] + g[number, i] * g[number, i] - h[number, i])
        element, element_p = -lengths[iv] * total / 4, -lengths[iv] * total_p / 4
        if prob[number] != 0.0:
            element = element + grad_j[:, :, number] / prob[number]
            element_p = element_p + pop_j[:, number] / prob[number]
        out_w += element
        out_g += element_p
    return {"theta": out_g, "migration": out_w}


def log_density(tips, ops, intervals, lengths, matrices, sizes, buffer_count, interval_count, dtype=np.longdouble):
    """basta_reference.update and accumulate on arrays of ``dtype`` as they are (no rounding through fp64)"""
    dt = np.dtype(dtype)
    partials = np.zeros((buffer_count, tips.shape[1]), dtype=dt)
    partials[:tips.shape[0]] = tips
    coalescent = np.zeros(interval_count, dtype=dt)
    br.update(partials, ops, intervals, matrices, sizes, coalescent)
    out = np.zeros(1, dtype=dt)
    br.accumulate(partials, ops, intervals, lengths, sizes, coalescent, out)
    return out[0]


def matrix_times(ops, intervals, distances):
    """{matrix number: t of the list interval whose operations use it}"""
    out = {}
    for k in range(len(intervals) - 1):
        for op in ops[intervals[k]:intervals[k + 1]]:
            for m in (int(op[2]), int(op[4])) if op[3] >= 0 else (int(op[2]),):
                assert out.setdefault(m, distances[k]) == distances[k]
    return out


def directional_difference(tips, ops, intervals, lengths, distances, matrices, sizes, buffer_count, interval_count, direction_w=None,
                           direction_theta=None, eps=1e-6, dtype=np.longdouble):
    """(L(+eps) - L(-eps)) / (2 eps) along ``direction_w`` [S][S] (every matrix m += eps t_m sum_ab D[a][b] (row b <- row a of m), that is
    eps t_m D^T M_m) and ``direction_theta`` [S] (1 / sizes += eps d)."""
    dt = np.dtype(dtype)
    eps = dt.type(eps)
    tips = np.asarray(tips).astype(dt)
    lengths = np.asarray(lengths).astype(dt)
    mats = {m: np.asarray(x).astype(dt) for m, x in matrices.items()}
    theta = dt.type(1.0) / np.asarray(sizes).astype(dt)
    times = matrix_times(ops, intervals, np.asarray(distances).astype(dt)) if direction_w is not None else {}
    value = []
    for sign in (dt.type(1.0), dt.type(-1.0)):
        moved = mats
        if direction_w is not None:
            d = np.asarray(direction_w).astype(dt)
            moved = {m: x + (sign * eps * times[m]) * (d.T @ x) if m in times else x for m, x in mats.items()}
        th = theta if direction_theta is None else theta + sign * eps * np.asarray(direction_theta).astype(dt)
        value.append(log_density(tips, ops, intervals, lengths, moved, dt.type(1.0) / th, buffer_count, interval_count, dt))
    return (value[0] - value[1]) / (2 * eps)


def finite_difference(tips, ops, intervals, lengths, distances, matrices, sizes, buffer_count, interval_count, eps=1e-6,
                      dtype=np.longdouble):
    """Every entry by central differences.  -> {"theta": [S], "migration": [S][S]}"""
    s = np.asarray(tips).shape[1]
    dt = np.dtype(dtype)
    out_w, out_g = np.zeros((s, s), dtype=dt), np.zeros(s, dtype=dt)
    args = (tips, ops, intervals, lengths, distances, matrices, sizes, buffer_count, interval_count)
    for a in range(s):
        unit = np.zeros(s)
        unit[a] = 1.0
        out_g[a] = directional_difference(*args, direction_theta=unit, eps=eps, dtype=dt)
        for b in range(s):
            unit_w = np.zeros((s, s))
            unit_w[a, b] = 1.0
            out_w[a, b] = directional_difference(*args, direction_w=unit_w, eps=eps, dtype=dt)
    return {"theta": out_g, "migration": out_w}
