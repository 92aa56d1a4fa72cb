"""Host restatement of the BASTA structured-coalescent likelihood, for the tests of beast_mcmc_amd.basta and the beagleBasta*
calls.  numpy only; every function takes a ``dtype`` so that the same code runs in fp64 and in numpy.longdouble.

What is restated (the reference's pure-Java delegate, src/dr/evomodel/coalescent/basta/):
  peel                   GenericBastaLikelihoodDelegate.peelPartials           (:813-877), for the operations of one interval at once
  reduce_within / reduce_across   reduceWithinInterval (:970-1006) / reduceAcrossIntervals (:935-968)
  update / accumulate    computeBranchIntervalOperations (:118-138) / dispatchComputeCoalescentIntervalReduction (:330-352)
  traverse               CoalescentIntervalTraversal.traverseReverseCoalescentLevelOrder (:259-480) and the CACHE_FRIENDLY buffer
                         map of BeagleBastaLikelihoodDelegate.vectorizeBranchIntervalOperations (:452-507)

Every sum runs in index order and every product is rounded before it is added (no dot products from a BLAS), so that the fp64
run is, operation for operation, what the Java code computes.  Operations of one interval are independent, which is why an
interval's operations can be taken together as long as each row's arithmetic keeps its order.
"""
import numpy as np

OP = 8


def traverse(left, right, height, tip_count, rate=1.0, sub_intervals=1):
    """-> (operations [n][8] int32, intervals, lengths, [(matrix number, scaled length)], buffer count, interval count)"""
    n_nodes = len(height)
    events = sorted(range(n_nodes), key=lambda x: (height[x], 0 if x < tip_count else 1, x))
    step = [0] * n_nodes                 # how often a node's lineage has been pushed through a matrix
    alive = [events[0]]
    ops, starts, lengths, mats = [], [0], [], []
    done = 0                             # (sub-)intervals closed so far
    last_matrix = [-1]

    def buf(x):
        return x if step[x] == 0 else (step[x] + 1) * n_nodes + x

    def use_matrix(number, length):
        if number != last_matrix[0]:
            mats.append((number, rate * length))
            last_matrix[0] = number
        return number

    def push(number, x, length):
        src = buf(x)
        step[x] += 1
        ops.append([buf(x), src, use_matrix(number, length), -1, -1, buf(x), -1, number])

    for prev, x in zip(events[:-1], events[1:]):
        span = float(height[x]) - float(height[prev])
        part = span / sub_intervals
        number = done * sub_intervals
        if x < tip_count:
            if span > 0.0:
                for _ in range(sub_intervals):
                    for y in alive:
                        push(number, y, part)
                    number += 1
                    done += 1
                    starts.append(len(ops)); lengths.append(part)
            alive.append(x)
            continue
        assert part > 0.0
        for _ in range(sub_intervals - 1):
            for y in alive:
                push(number, y, part)
            number += 1
            done += 1
            starts.append(len(ops)); lengths.append(part)
        a, b = int(left[x]), int(right[x])
        m = use_matrix(number, part)
        ops.append([x, buf(a), m, buf(b), m, n_nodes + a, n_nodes + b, number])
        alive = [y for y in alive if y != a and y != b]
        for y in alive:
            push(number, y, part)
        alive.append(x)
        done += 1
        starts.append(len(ops)); lengths.append(part)
    ops = np.asarray(ops, dtype=np.int64).reshape(-1, OP)
    first_use, used = {}, tip_count
    for row in ops:
        for c in (0, 1, 3, 5, 6):
            v = int(row[c])
            if v >= tip_count:
                if v not in first_use:
                    first_use[v] = used
                    used += 1
                row[c] = first_use[v]
    return (ops.astype(np.int32), np.asarray(starts, dtype=np.int32), np.asarray(lengths), mats, used,
            int(ops[:, 7].max()) + 1)


def matvec_rows(matrix, vectors):
    """rows r: sum_j matrix[i][j] vectors[r][j] for every i, j in index order"""
    out = np.zeros_like(vectors)
    for j in range(matrix.shape[0]):
        out += vectors[:, j:j + 1] * matrix[None, :, j]
    return out


def peel(partials, ops, matrices, sizes, coalescent):
    """The operations ``ops`` of one interval (independent of each other), in place on ``partials`` [buffer][S]."""
    for m in np.unique(ops[:, 2]):
        sel = ops[ops[:, 2] == m]
        partials_in = partials[sel[:, 1]]
        lefts = matvec_rows(matrices[m], partials_in)
        for k, op in enumerate(sel):
            dest, in2, m2, acc1, acc2, number = int(op[0]), int(op[3]), int(op[4]), int(op[5]), int(op[6]), int(op[7])
            left = lefts[k]
            if in2 < 0:
                partials[dest] = left
                continue
            right = matvec_rows(matrices[m2], partials[in2][None, :])[0]
            entry = left * right / sizes
            prob = entry.dtype.type(0.0)
            for i in range(entry.shape[0]):
                prob = prob + entry[i]
            partials[dest] = entry / prob
            partials[acc1] = left
            partials[acc2] = right
            coalescent[number] = prob


def update(partials, ops, intervals, matrices, sizes, coalescent):
    coalescent[:] = 0.0
    for k in range(len(intervals) - 1):
        if intervals[k + 1] > intervals[k]:
            peel(partials, ops[intervals[k]:intervals[k + 1]], matrices, sizes, coalescent)


def accumulate(partials, ops, intervals, lengths, sizes, coalescent, out, keep=None):
    """out[0] += the log-density; ``keep``: a dict that receives e, f, g, h ([interval number][S]) and the per-interval terms"""
    s = partials.shape[1]
    dt = partials.dtype
    n_numbers = coalescent.shape[0]
    e, f, g, h = (np.zeros((n_numbers, s), dtype=dt) for _ in range(4))
    for k in range(len(intervals) - 1):                  # reduceWithinInterval, operations in list order
        for op in ops[intervals[k]:intervals[k + 1]]:
            number = int(ops[intervals[k], 7])
            for start, end in ((op[1], op[5]), (op[3], op[6])):
                if start < 0:
                    continue
                a, b = partials[start], partials[end]
                e[number] += a; f[number] += a * a
                g[number] += b; h[number] += b * b
    terms = []
    for k in range(len(intervals) - 1):                  # reduceAcrossIntervals
        if intervals[k + 1] <= intervals[k]:
            terms.append(dt.type(0.0))
            continue
        number = int(ops[intervals[k], 7])
        total = dt.type(0.0)
        for i in range(s):
            total = total + (e[number, i] * e[number, i] - f[number, i] + g[number, i] * g[number, i] - h[number, i]) / sizes[i]
        logl = -dt.type(lengths[k]) * total / dt.type(4)
        if coalescent[number] != 0.0:
            logl = logl + np.log(coalescent[number])
        terms.append(logl)
        out[0] = out[0] + logl
    if keep is not None:
        keep.update(e=e, f=f, g=g, h=h, terms=np.asarray(terms))


def evaluate(tips, ops, intervals, lengths, matrices, sizes, buffer_count, interval_count, dtype=np.float64):
    """One evaluation from tip vectors [T][S] and matrices {number: S x S fp64 array}.
    -> (logL, partials [buffer][S], coalescent probabilities [interval_count])"""
    dt = np.dtype(dtype)
    s = tips.shape[1]
    partials = np.zeros((buffer_count, s), dtype=dt)
    partials[:tips.shape[0]] = tips
    mats = {m: np.asarray(v, dtype=np.float64).astype(dt) for m, v in matrices.items()}
    sizes = np.asarray(sizes, dtype=np.float64).astype(dt)
    coalescent = np.zeros(interval_count, dtype=dt)
    update(partials, ops, intervals, mats, sizes, coalescent)
    out = np.zeros(1, dtype=dt)
    accumulate(partials, ops, intervals, lengths, sizes, coalescent, out)
    return out[0], partials, coalescent


def transition_matrices(evec, ievc, evals, mats):
    """{number: U exp(D t) U^-1}: real spectrum (S eigenvalues), or the real block form of a complex one (2 S: real parts, then
    imaginary parts; GenericBastaLikelihoodDelegate.computeTransitionProbabilities :879-933 without its abs())."""
    s = evec.shape[0]
    out = {}
    for number, t in mats:
        iexp = np.zeros((s, s))
        i = 0
        while i < s:
            if len(evals) == s or evals[s + i] == 0.0:
                iexp[i] = ievc[i] * np.exp(t * evals[i])
            else:
                b = evals[s + i]
                ea = np.exp(t * evals[i])
                c, sn = ea * np.cos(t * b), ea * np.sin(t * b)
                iexp[i] = c * ievc[i] + sn * ievc[i + 1]
                iexp[i + 1] = c * ievc[i + 1] - sn * ievc[i]
                i += 1
            i += 1
        out[number] = evec @ iexp
    return out


def depths(ops, buffer_count):
    """Per buffer, and per operation: the number of matrix-vector products on the longest dependency path that ends there, a
    two-child operation counting as three (two products, then the elementwise product, the division and the normalising sum)."""
    d = np.zeros(buffer_count, dtype=np.int64)
    per_op = np.zeros(len(ops), dtype=np.int64)
    for k, op in enumerate(ops):
        if op[3] < 0:
            d[op[0]] = d[op[1]] + 1
        else:
            a, b = d[op[1]], d[op[3]]
            d[op[5]], d[op[6]] = a + 1, b + 1
            d[op[0]] = max(a, b) + 3
        per_op[k] = d[op[0]]
    return d, per_op


def kingman_log_density(height, tip_count, population):
    """One deme: sum_k -len_k L_k (L_k - 1) / (2 N) - (T - 1) log N over the intervals between consecutive events."""
    events = sorted(range(len(height)), key=lambda x: (height[x], 0 if x < tip_count else 1, x))
    lineages, logl = 1, 0.0
    for prev, x in zip(events[:-1], events[1:]):
        logl -= (height[x] - height[prev]) * lineages * (lineages - 1) / (2.0 * population)
        lineages += 1 if x < tip_count else -1
    return logl - (tip_count - 1) * np.log(population)
