"""What the CPU and the GPU tests of the complete-history simulator share: the cases (tree, model, registers, site count, seed), the
node list of a tree, the restatement of every case (computed once) and the reward / height bound."""
import functools
from types import SimpleNamespace

import numpy as np

import complete_history_reference as hr
import helpers

EPS = 2.0 ** -53
BOUND_C = 8          # test_gpu_complete_history.py's docstring derives it
OTHER_SEEDS = (41, 42)                   # the GPU tier's determinism, chunk and capacity calls on case "s4"
SHARDED_SEED, SHARDED_SITES = 31, 3001   # ... and its sharded-handle call


def tree_rows(tree, generator_of_node=None, ancestral=True):
    """-> (rows {outRow = node (or -1), qIndex, parentRow} in pre-order, the tree node of every row)."""
    order, stack = [], [tree.root]
    while stack:
        n = stack.pop()
        order.append(n)
        if n >= tree.tip_count:
            stack.append(int(tree.right[n])); stack.append(int(tree.left[n]))
    row_of = {n: r for r, n in enumerate(order)}
    rows = []
    for n in order:
        p = int(tree.parent[n])
        q = 0 if (p < 0 or generator_of_node is None) else int(generator_of_node[n])
        rows.append([n if (ancestral or n < tree.tip_count) else -1, q, -1 if p < 0 else row_of[p]])
    return np.asarray(rows, dtype=np.int32), np.asarray(order, dtype=np.int64)


def q_of(eig):
    return np.ascontiguousarray((eig.evec * eig.evals[None, :]) @ eig.ievc)


def registers(S, K, rng):
    """K registers, counts and rewards alternating: register 0 counts every jump, the other count registers are random 0 / 1
    labellings, the reward registers random positive vectors on the diagonal."""
    regs, flags = np.zeros((K, S, S)), np.zeros(K, dtype=np.int32)
    for k in range(K):
        if k % 2 == 0:
            regs[k] = 1.0 if k == 0 else (rng.random((S, S)) < 0.5).astype(np.float64)
            np.fill_diagonal(regs[k], 0.0)
        else:
            regs[k] = np.diag(rng.uniform(0.5, 2.0, size=S))
            flags[k] = hr.REWARDS
    return regs, flags


#        name       S   C  T    tree           sites K  seed  zero-rate category
CASES = {
    "s2":      (2,  1, 3,   "coalescent",  1,    1, 101, False),     # one site: one live lane
    "s4":      (4,  4, 9,   "coalescent",  1025, 3, 102, False),     # across a chunk edge of 256 and a wave edge
    "s4zero":  (4,  4, 40,  "coalescent",  300,  8, 103, True),      # a category that stops the clock; every register slot
    "s20":     (20, 4, 9,   "coalescent",  63,   3, 104, False),     # above 16 states: binary search; one lane short of a wave
    "s61":     (61, 1, 9,   "coalescent",  300,  3, 105, False),
    "s64":     (64, 4, 9,   "coalescent",  1025, 8, 106, False),     # the full LDS footprint
    "cat300":  (4,  1, 300, "caterpillar", 63,   1, 107, False),     # the longest parent chain: previous-row and read-back parents
}


@functools.lru_cache(maxsize=None)
def build(name):
    S, C, T, kind, sites, K, seed, zero = CASES[name]
    wl = helpers.random_workload(T, 2, S, C, seed=seed, tree_kind=kind, root_to_tip=2.0)      # (its tree and model only)
    rng = np.random.default_rng(seed)
    regs, flags = registers(S, K, rng)
    rows, order = tree_rows(wl.tree)
    lengths = np.array([0.0 if r == 0 else wl.tree.branch_length(int(n)) for r, n in enumerate(order)])
    heights = np.array([wl.tree.height[int(n)] for n in order], dtype=np.float64)
    rates = np.array(wl.cat_rates, dtype=np.float64)
    if zero:
        rates[0] = 0.0
    return SimpleNamespace(name=name, S=S, C=C, K=K, sites=sites, seed=seed, tree=wl.tree, rows=rows, order=order, lengths=lengths,
                           heights=heights, Q=q_of(wl.eig)[None], registers=regs, flags=flags, cat_rates=rates,
                           cat_weights=np.array(wl.cat_weights, dtype=np.float64), freqs=np.array(wl.freqs, dtype=np.float64))


def restate(c, seed=None, sites=None, site_count=None, **kw):
    return hr.simulate(c.rows, c.lengths, c.Q, c.registers, c.flags, c.cat_rates, c.cat_weights, c.freqs, c.seed if seed is None else seed,
                       c.sites if site_count is None else site_count, heights=c.heights, sites=sites, **kw)


@functools.lru_cache(maxsize=None)
def restated(name):
    """The restatement of a case, computed once and shared; nobody changes it."""
    return restate(build(name))


# the per-branch-generator case: three generators, the rows' qIndex both staying and changing between consecutive rows
@functools.lru_cache(maxsize=None)
def build_generators():
    c = build("s4")
    rng = np.random.default_rng(9)
    Qs = []
    for scale in (1.0, 0.4, 2.5):
        wl = helpers.random_workload(4, 4, 4, 1, seed=int(scale * 10) + 50)
        Qs.append(scale * q_of(wl.eig))
    pattern = np.array([0, 0, 1, 1, 1, 2, 0, 2, 2, 1, 0, 0, 2, 1, 1, 0, 2])[:len(c.rows)]
    rows = c.rows.copy()
    rows[1:, 1] = pattern[1:]
    d = SimpleNamespace(**vars(c))
    d.rows, d.Q, d.name, d.seed = rows, np.stack(Qs), "generators", 108
    return d


@functools.lru_cache(maxsize=None)
def restated_generators():
    return restate(build_generators())


def reward_bound(res, c):
    """[K, n, m]: BOUND_C * (jumps + 2) * 2^-53 * tau * max |R_kk| per history (0 for a count register: those are exact)."""
    tau = res["rate_c"][None, :] * c.lengths[:, None]
    top = np.array([np.abs(np.diag(c.registers[k])).max() if c.flags[k] & hr.REWARDS else 0.0 for k in range(c.K)])
    return BOUND_C * (res["counts"] + 2)[None] * EPS * tau[None] * top[:, None, None]


def height_bound(res, c):
    """[E]: BOUND_C * (m + 2) * 2^-53 * |h_parent - h_child| for the m-th jump of its history."""
    ro = res["event_row"]
    first = np.r_[True, (ro[1:] != ro[:-1]) | (res["event_site"][1:] != res["event_site"][:-1])] if len(ro) else np.zeros(0, dtype=bool)
    start = np.maximum.accumulate(np.where(first, np.arange(len(ro)), 0)) if len(ro) else np.zeros(0, dtype=np.int64)
    m = np.arange(len(ro)) - start + 1
    return BOUND_C * (m + 2) * EPS * np.abs(c.heights[c.rows[ro, 2]] - c.heights[ro])
