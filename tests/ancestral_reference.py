"""Host restatement of beagleMi355SampleAncestralStates (include/beagle_mi355.h), vectorised over patterns.

It restates AncestralStateBeagleTreeLikelihood.traverseSample (src/dr/evomodel/treelikelihood/AncestralStateBeagleTreeLikelihood.java:
414-625, linear-space conditionals) and MathUtils.randomChoicePDF (src/dr/math/MathUtils.java:82-104) with the engine's stateless
random numbers, from what an engine reads back — getPartials, getTransitionMatrix, getTipStates — so that the sampler is checked
apart from the likelihood.  Every product, sum and difference is one IEEE double operation in the order the kernel forms it
(numpy does not contract to FMA), so the states must agree bit for bit.
"""
import numpy as np

GOLDEN = 0x9E3779B97F4A7C15
MIX1 = 0xBF58476D1CE4E5B9
MIX2 = 0x94D049BB133111EB
DBL_MAX = np.finfo(np.float64).max


def splitmix64(seed, ctr):
    """z = the (ctr + 1)-th SplitMix64 output from state `seed`, elementwise over ctr (uint64 arithmetic modulo 2^64)."""
    ctr = np.asarray(ctr, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = np.uint64(seed & 0xFFFFFFFFFFFFFFFF) + (ctr + np.uint64(1)) * np.uint64(GOLDEN)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(MIX1)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(MIX2)
        z = z ^ (z >> np.uint64(31))
    return z


def uniforms(seed, rows, patterns, pattern_count, kind):
    """u[row, pattern] for the counter ((row * pattern_count + p) * 2 + kind): rows x patterns (any broadcastable shapes)."""
    rows = np.asarray(rows, dtype=np.uint64)
    patterns = np.asarray(patterns, dtype=np.uint64)
    with np.errstate(over="ignore"):
        ctr = (rows * np.uint64(pattern_count) + patterns) * np.uint64(2) + np.uint64(kind)
    return (splitmix64(seed, ctr) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


UNDECIDED = 1e-8


def near_a_boundary(weights, u, use_map, tol=UNDECIDED):
    """bool, of the weights' shape: the draw would come out differently under a relative change of `tol` in the weights — some running
    sum lies within tol x total of u x total, or (use_map) the largest and the second-largest weight lie within tol x total."""
    total = np.zeros_like(weights[0])
    for w in weights:
        total = total + w
    if use_map:
        top = np.sort(np.stack(weights), axis=0)[-2:]
        return (top[1] - top[0]) <= tol * total
    near = np.zeros(total.shape, dtype=bool)
    cum = np.zeros_like(total)
    for w in weights:
        cum = cum + w
        near |= np.abs(u * total - cum) <= tol * total
    return near


def draw_choice(weights, u, use_map):
    """weights: list of n arrays (one per choice, all of one shape), u: array of that shape -> (choice int64, bad bool)."""
    total = np.zeros_like(weights[0])
    last_positive = np.zeros(total.shape, dtype=np.int64)
    best = weights[0].copy()
    choice = np.zeros(total.shape, dtype=np.int64)
    for i, w in enumerate(weights):
        total = total + w
        last_positive = np.where(w > 0.0, i, last_positive)
        if i > 0:
            better = w > best
            best = np.where(better, w, best)
            choice = np.where(better, i, choice)
    bad = ~((total > 0.0) & (total <= DBL_MAX))
    if not use_map:
        U = u * total
        choice = np.full(total.shape, -1, dtype=np.int64)
        for i, w in enumerate(weights):
            U = U - w
            choice = np.where((choice < 0) & (U < 0.0), i, choice)
        choice = np.where(choice < 0, last_positive, choice)
    return np.where(bad, 0, choice), bad


def sample(rows, partials_of, matrix_of, tip_states_of, is_compact, category_weights, frequencies, seed, use_map=False,
           patterns=None, pattern_count=None, undecided=None):
    """The draw for `rows` ([n][3] {buffer, matrix, parentRow}, root first).

    partials_of(buffer) -> [C, P, S] as getPartials(buffer, NONE) returns it; matrix_of(matrix) -> [C, S, S] (getTransitionMatrix);
    tip_states_of(buffer) -> [P] (getTipStates); is_compact(buffer) -> bool.  `patterns`: restate only these pattern indices
    (default all); `pattern_count`: the alignment's P (the random-number counter's stride; default the partials' P).
    `undecided`: a bool array [len(patterns)] that is set where some draw of the pattern lies `near_a_boundary`.
    -> (states uint8 [n, len(patterns)], categories int32 [len(patterns)], any_bad)."""
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, 3)
    root = partials_of(int(rows[0, 0]))
    C, P, S = root.shape
    pats = np.arange(P) if patterns is None else np.asarray(patterns, dtype=np.int64)
    GP = P if pattern_count is None else pattern_count
    category_weights = np.asarray(category_weights, dtype=np.float64)
    frequencies = np.asarray(frequencies, dtype=np.float64)
    any_bad = False
    if C > 1:
        wc = []
        for c in range(C):
            s = np.zeros(len(pats))
            for k in range(S):
                s = s + root[c, pats, k]
            wc.append(s * category_weights[c])
        cats, bad = draw_choice(wc, uniforms(seed, 0, pats, GP, 1), use_map)
        if undecided is not None:
            undecided |= near_a_boundary(wc, uniforms(seed, 0, pats, GP, 1), use_map)
        any_bad |= bool(bad.any())
    else:
        cats = np.zeros(len(pats), dtype=np.int64)
    states = np.zeros((len(rows), len(pats)), dtype=np.uint8)
    rp = root[cats, pats, :]
    s0, bad = draw_choice([rp[:, i] * frequencies[i] for i in range(S)], uniforms(seed, 0, pats, GP, 0), use_map)
    if undecided is not None:
        undecided |= near_a_boundary([rp[:, i] * frequencies[i] for i in range(S)], uniforms(seed, 0, pats, GP, 0), use_map)
    any_bad |= bool(bad.any())
    states[0] = s0
    for r in range(1, len(rows)):
        b, m, parent = (int(x) for x in rows[r])
        M = matrix_of(m)[cats, states[parent].astype(np.int64), :]          # [pattern, S]: M[c*][parentState][.]
        u = uniforms(seed, r, pats, GP, 0)
        if is_compact(b):
            tip = np.asarray(tip_states_of(b))[pats].astype(np.int64)
            drawn, bad = draw_choice([M[:, i] for i in range(S)], u, use_map)
            unknown = tip >= S
            if undecided is not None:
                undecided |= unknown & near_a_boundary([M[:, i] for i in range(S)], u, use_map)
            any_bad |= bool((bad & unknown).any())
            states[r] = np.where(unknown, drawn, tip)
        else:
            part = partials_of(b)[cats, pats, :]
            drawn, bad = draw_choice([part[:, i] * M[:, i] for i in range(S)], u, use_map)
            any_bad |= bool(bad.any())
            if undecided is not None:
                undecided |= near_a_boundary([part[:, i] * M[:, i] for i in range(S)], u, use_map)
            states[r] = drawn
    return states, cats.astype(np.int32), any_bad


def sample_from_engine(beagle, rows, compact, category_weights, frequencies, seed, use_map=False, patterns=None):
    """`sample` over what the engine instance behind `beagle` (a beagle.Beagle binding) reads back; `compact`: the buffers that hold
    compact tip states.  (Partials are read row by row and not kept: at 1000 taxa x 1e5 patterns they are 13 GB.)"""
    cache_m = {}

    def matrix_of(m):
        if m not in cache_m:
            cache_m[m] = beagle.getTransitionMatrix(m).reshape(beagle.categoryCount, beagle.stateCount, beagle.stateCount)
        return cache_m[m]

    return sample(rows, beagle.getPartials, matrix_of, beagle.getTipStates, lambda b: b in compact, category_weights, frequencies, seed,
                  use_map=use_map, patterns=patterns)
