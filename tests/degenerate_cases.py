"""Degenerate and stiff inputs: case builders and a plain reference (tests/test_degenerate_host.py, tests/test_gpu_degenerate_inputs.py).

The reference is Felsenstein's pruning in np.longdouble on matrices handed in as data, without rescaling.  Every term is non-negative,
so an entry or a site sum is exactly 0 if and only if it is STRUCTURALLY zero — provided nothing underflows: the builders keep non-zero
matrix entries above 1e-3 and the trees at 12 taxa or fewer, so no live value drops below ~1e-80.  The reference decides which patterns
are dead and which partial entries are zero; the CPU oracle stays the bound on values.

Part A cases (matrices injected through setTransitionMatrix, identical on both sides):
  identity   identity on both branches of every cherry, dense elsewhere: dead <=> some cherry's two known tips differ
  block      every matrix block-diagonal over two state classes: dead <=> the known tips span both classes
  root       the block matrices, a pattern's tips all in one class, pi zero on class B: only the root sees a zero
  weight     dense matrices, one category weight exactly 0, every pattern live
Dead patterns sit at 0 and 1 (a whole lane pair), 2 (3 live), 5 (4 live), on both sides of 31/32, 63/64, 127/128 and on the last
pattern of a ragged count; pattern 1 repeats pattern 0's sub-patterns below the root's children."""
import ctypes as C

import numpy as np

import beast_mcmc_amd as bm
import helpers
from beast_mcmc_amd.inputs import synth, trees
from beast_mcmc_amd.treelikelihood import BeagleTreeLikelihood, RESCALE_DYNAMIC, RESCALE_NONE

LD = np.longdouble
NONE = bm.beagle.NONE
FIXED_DEAD = (0, 1, 2, 5, 31, 32, 63, 64, 127, 128)
KEPT_LIVE = (3, 4)


# ---- the plain reference -----------------------------------------------------------------------------------------------------------

def tip_partials(states, S, dtype=np.float64):
    """[P][S]: one-hot for a known state, all ones for a missing one (code >= S)."""
    states = np.asarray(states)
    part = np.ones((len(states), S), dtype=dtype)
    known = states < S
    part[known] = 0
    part[np.nonzero(known)[0], states[known]] = 1
    return part


def reference_prune(tree, tip_states, S, mats, cat_weights, freqs):
    """-> (site log-likelihoods [P], {node: partials [C][P][S]}), all np.longdouble; mats: {node: [C][S][S]} for every node but the root."""
    T, Cn = tree.tip_count, len(cat_weights)
    x = {t: np.broadcast_to(tip_partials(tip_states[t], S, LD), (Cn, tip_states.shape[1], S)) for t in range(T)}
    for n in tree.postorder():
        if n >= T:
            l, r = int(tree.left[n]), int(tree.right[n])
            x[n] = np.einsum("cij,cpj->cpi", mats[l].astype(LD), x[l]) * np.einsum("cij,cpj->cpi", mats[r].astype(LD), x[r])
    site = np.einsum("c,cps,s->p", np.asarray(cat_weights, dtype=LD), x[tree.root], np.asarray(freqs, dtype=LD))
    with np.errstate(divide="ignore"):
        return np.log(site), {n: x[n] for n in range(T, tree.node_count)}


# ---- part A: builders ---------------------------------------------------------------------------------------------------------------

class Case:
    def __init__(self, name, wl, mats, dead):
        self.name, self.wl, self.mats, self.dead = name, wl, mats, np.asarray(dead, dtype=bool)
        self._ref = None

    def reference(self):
        if self._ref is None:
            wl = self.wl
            self._ref = reference_prune(wl.tree, wl.tip_states, wl.state_count, self.mats, wl.cat_weights, wl.freqs)
        return self._ref


def cherries(tree):
    return [n for n in range(tree.tip_count, tree.node_count) if tree.left[n] < tree.tip_count and tree.right[n] < tree.tip_count]


def dense_matrix(rng, S, Cn):
    """Row-stochastic [C][S][S], every entry >= 0.5 / (1.5 S) (4.8e-3 at 70 states)."""
    m = rng.uniform(0.5, 1.5, size=(Cn, S, S))
    return m / m.sum(axis=2, keepdims=True)


def block_matrix(rng, S, Cn):
    """Row-stochastic and block-diagonal over the classes A = [0, S // 2) and B = [S // 2, S): exact zeros off the blocks."""
    a = S // 2
    m = np.zeros((Cn, S, S))
    m[:, :a, :a] = dense_matrix(rng, a, Cn)
    m[:, a:, a:] = dense_matrix(rng, S - a, Cn)
    return m


def dead_mask(P, rng, kind="placed"):
    if kind in ("all", "live"):
        return np.full(P, kind == "all")
    dead = np.zeros(P, dtype=bool)
    dead[[p for p in FIXED_DEAD if p < P] + [P - 1]] = True
    free = np.array([p for p in range(P) if not dead[p] and p not in KEPT_LIVE])
    extra = max(0, int(round(0.25 * P)) - int(dead.sum()))
    if extra and len(free):
        dead[rng.choice(free, size=min(extra, len(free)), replace=False)] = True
    return dead


def _base(S, Cn, T, P, seed):
    """A seeded tree, model and site model (the first, dense evaluation uses them) with tip states drawn uniformly, ~4 % missing."""
    wl = helpers.random_workload(T, max(P, 8), S, Cn, seed=seed, unknown_fraction=0.0)
    rng = np.random.default_rng(seed + 7)
    tips = rng.integers(0, S, size=(T, P)).astype(np.int32)
    tips[rng.random(tips.shape) < 0.04] = S
    weights = rng.integers(1, 9, size=P).astype(np.float64)
    return wl, rng, tips, weights


def _workload(name, wl, tips, weights, freqs=None, cat_weights=None):
    return synth.Workload(name, wl.tree, wl.eig, wl.freqs if freqs is None else freqs, wl.cat_rates,
                          wl.cat_weights if cat_weights is None else cat_weights, np.ascontiguousarray(tips), weights, wl.state_count)


def _repeat_first_pattern(tips, tree):
    """Pattern 1 = pattern 0 (with a weight of its own): two dead patterns of one lane pair in which every clade sees a repeated sub-pattern."""
    tips[:, 1] = tips[:, 0]


def identity_case(S, Cn, T, P, seed, kind="placed"):
    wl, rng, tips, weights = _base(S, Cn, T, P, seed)
    tree, ch = wl.tree, cherries(wl.tree)
    dead = dead_mask(P, rng, kind)
    for p in range(P):
        for a, b in ((int(tree.left[n]), int(tree.right[n])) for n in ch):
            if tips[a, p] < S and tips[b, p] < S:
                tips[b, p] = tips[a, p]
        if dead[p]:
            n = ch[p % len(ch)]
            a, b = int(tree.left[n]), int(tree.right[n])
            if tips[a, p] >= S:
                tips[a, p] = p % S
            tips[b, p] = (tips[a, p] + 1 + p % (S - 1)) % S
    if P > 1 and dead[0] and dead[1]:
        _repeat_first_pattern(tips, tree)
    eye = np.broadcast_to(np.eye(S), (Cn, S, S)).copy()
    under = set(int(c) for n in ch for c in (tree.left[n], tree.right[n]))
    mats = {n: (eye if n in under else dense_matrix(rng, S, Cn)) for n in range(tree.node_count) if n != tree.root}
    return Case("identity", _workload("identity-S%d" % S, wl, tips, weights), mats, dead)


def _into_class(tips, p, S, cls):
    a = S // 2
    lo, size = (0, a) if cls == 0 else (a, S - a)
    known = tips[:, p] < S
    tips[known, p] = lo + tips[known, p] % size


def block_case(S, Cn, T, P, seed, kind="placed"):
    wl, rng, tips, weights = _base(S, Cn, T, P, seed)
    dead = dead_mask(P, rng, kind)
    a = S // 2
    for p in range(P):
        cls = int(rng.integers(0, 2))
        _into_class(tips, p, S, cls)
        if dead[p]:
            k, k2 = p % T, (p + 1) % T
            if tips[k2, p] >= S:
                tips[k2, p] = 0 if cls == 0 else a
            tips[k, p] = (a + p % (S - a)) if cls == 0 else p % a
    if P > 1 and dead[0] and dead[1]:
        _repeat_first_pattern(tips, wl.tree)
    mats = {n: block_matrix(rng, S, Cn) for n in range(wl.tree.node_count) if n != wl.tree.root}
    return Case("block", _workload("block-S%d" % S, wl, tips, weights), mats, dead)


def root_case(S, Cn, T, P, seed, kind="placed"):
    """Dead at the root only: a dead pattern's tips all lie in class B, where pi is zero."""
    wl, rng, tips, weights = _base(S, Cn, T, P, seed)
    dead = dead_mask(P, rng, kind)
    for p in range(P):
        _into_class(tips, p, S, 1 if dead[p] else 0)
        if (tips[:, p] >= S).all():
            tips[0, p] = S - 1 if dead[p] else 0
    if P > 1 and dead[0] and dead[1]:
        _repeat_first_pattern(tips, wl.tree)
    pi = wl.freqs.copy()
    pi[S // 2:] = 0.0
    pi /= pi.sum()
    mats = {n: block_matrix(rng, S, Cn) for n in range(wl.tree.node_count) if n != wl.tree.root}
    return Case("root", _workload("root-S%d" % S, wl, tips, weights, freqs=pi), mats, dead)


def weight_case(S, Cn, T, P, seed, kind="placed"):
    """Every pattern live, the weight of category 1 (category 0 where there is one category ... there must be two) exactly zero."""
    assert Cn >= 2
    wl, rng, tips, weights = _base(S, Cn, T, P, seed)
    w = wl.cat_weights.copy()
    w[1] = 0.0
    w /= w.sum()
    mats = {n: dense_matrix(rng, S, Cn) for n in range(wl.tree.node_count) if n != wl.tree.root}
    return Case("weight", _workload("weight-S%d" % S, wl, tips, weights, cat_weights=w), mats, np.zeros(P, dtype=bool))


BUILDERS = {"identity": identity_case, "block": block_case, "root": root_case, "weight": weight_case}
_cases = {}


def case(name, S, Cn, T=9, P=None, kind="placed"):
    """Cached (the reference is computed once per case): P defaults to the ragged count of the layout — 131 below 16 states, 67 from there."""
    if P is None:
        P = 131 if S < 16 else 67
    key = (name, S, Cn, T, P, kind)
    if key not in _cases:
        _cases[key] = BUILDERS[name](S, Cn, T, P, seed=300 + S + Cn, kind=kind)
    return _cases[key]


# ---- part A: the injected evaluation, the same calls on the engine and on the oracle ------------------------------------------------

class Injected:
    """What one injected evaluation left behind."""


def _set_tip_partials(tl, wl):
    for t in range(wl.tip_count):
        part = np.ascontiguousarray(tip_partials(wl.tip_states[t], wl.state_count))
        tl._chk(tl.h.btlSetTipPartials(tl.ptr, t, part.ctypes.data_as(C.POINTER(C.c_double))), "setTipPartials")
    tl.makeDirty()


def inject_and_run(tl, raw, cs, mats=None):
    """Overwrite the matrices of tl's last operation list with cs.mats (mats: another set), re-issue the list, accumulate what it wrote
    and integrate at the root.  Every return code is checked (the root call's is returned: -8 would be a NaN)."""
    wl, tree = cs.wl, cs.wl.tree
    mats = cs.mats if mats is None else mats
    T = tree.tip_count
    ops = tl.last_operations().copy()
    assert len(ops) == T - 1                                   # a full evaluation
    index = {n: tl.node_matrix_index(n) for n in range(tree.node_count) if n != tree.root}
    assert set(index.values()) == set(int(m) for m in ops[:, 4]) | set(int(m) for m in ops[:, 6])
    for n, m in index.items():
        raw.setTransitionMatrix(m, mats[n], 1.0)
    out = Injected()
    out.ops = ops
    out.before = raw.walkStats() if tl.engine.prefix == "" else None
    raw.updatePartials(np.ascontiguousarray(ops, dtype=np.int32).ravel(), len(ops), NONE)
    cum = tl.cumulative_scale_index()
    out.write_mode = bool(ops[0, 1] >= 0)
    out.scaled = cum != NONE
    scale_of = {n: tl.node_scale_index(n) for n in range(T, tree.node_count)}
    if out.write_mode:
        assert sorted(scale_of.values()) == sorted(int(s) for s in ops[:, 1])
        raw.resetScaleFactors(cum)
        raw.accumulateScaleFactors(list(scale_of.values()), len(scale_of), cum)
    raw.setCategoryWeights(0, wl.cat_weights)
    raw.setStateFrequencies(0, wl.freqs)
    total = np.zeros(1)
    b, z, s = (np.array([v], dtype=np.int32) for v in (tl.root_buffer_index(), 0, cum))
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    out.rc = raw._f["CalculateRootLogLikelihoods"](raw.instance, ip(b), ip(z), ip(z), ip(s), 1, total.ctypes.data_as(C.POINTER(C.c_double)))
    out.lnl = float(total[0])
    out.site = raw.getSiteLogLikelihoods().copy()
    out.after = raw.walkStats() if tl.engine.prefix == "" else None      # (after the root call: a walk may be held back until then)
    out.partials = {n: raw.getPartials(tl.node_buffer_index(n), NONE).copy() for n in range(T, tree.node_count)}
    out.factors = {n: raw.getLogScaleFactors(scale_of[n]).copy() for n in scale_of} if out.scaled else {}
    out.cumulative = raw.getLogScaleFactors(cum).copy() if out.scaled else None
    return out


def stats_delta(res):
    return {k: res.after[k] - res.before[k] for k in res.after}


def evaluate_injected(cs, scheme, library=None, read_mode=False, as_partials=False, twice=False):
    """One evaluation through BeagleTreeLikelihood on the model's own (dense) matrices — whatever the engine derives from matrices is
    now derived from THOSE — then the injected evaluation.  read_mode (DYNAMIC): the injected evaluation in write mode leaves the factors of
    the injected matrices behind; the next evaluation after set_branch_rates reads them; its list is re-issued on the injected matrices.
    twice: the last injected evaluation is made once more (the list a second time on the same matrices: what a cached plan sees)."""
    wl = cs.wl
    tl = BeagleTreeLikelihood(wl, library=library, rescaling=scheme, delay_rescaling=False)
    raw = bm.beagle.Beagle.attach(tl)
    try:
        if as_partials:
            _set_tip_partials(tl, wl)
        first = tl.getLogLikelihood()
        assert np.isfinite(first)                               # (dense matrices: nothing is dead yet)
        res = inject_and_run(tl, raw, cs)
        assert res.write_mode == (scheme != RESCALE_NONE)
        if read_mode:
            assert scheme == RESCALE_DYNAMIC
            tl.storeState()
            tl.set_branch_rates(np.linspace(0.7, 1.4, wl.tree.node_count))
            tl.getLogLikelihood()
            res = inject_and_run(tl, raw, cs)
            assert not res.write_mode and res.scaled and (res.ops[:, 2] >= 0).all()
        if twice:
            res = inject_and_run(tl, raw, cs)
        return res
    finally:
        tl.close()


def check_against_reference(cs, res, what=""):
    """The structural half (no oracle needed): return codes, no NaN anywhere, dead patterns exactly -inf and nothing else, zero partial
    entries exactly where the reference has them, factor 0.0 where a pattern is all-zero at a node, live values within 1e-10."""
    wl = cs.wl
    ref_site, ref_nodes = cs.reference()
    dead = np.isneginf(ref_site)
    assert np.array_equal(dead, cs.dead), what
    assert res.rc == 0, (what, res.rc)
    assert not np.isnan(res.site).any(), what
    assert np.array_equal(np.isneginf(res.site), dead), (what, np.nonzero(np.isneginf(res.site) != dead)[0])
    assert np.isfinite(res.site[~dead]).all(), what
    expect_inf = bool((wl.weights[dead] > 0).any())
    assert (res.lnl == -np.inf) == expect_inf and not np.isnan(res.lnl), (what, res.lnl)
    live = ~dead
    if live.any():
        rs = ref_site[live].astype(np.float64)
        assert np.max(np.abs(res.site[live] - rs) / np.abs(rs)) <= 1e-10, what
        if not expect_inf:
            assert helpers.rel_err(res.lnl, float(np.dot(ref_site.astype(np.float64), wl.weights))) <= 1e-10, what
    for n, pg in res.partials.items():
        assert not np.isnan(pg).any(), (what, n)
        assert np.array_equal(pg == 0.0, ref_nodes[n] == 0), (what, n)
        if res.write_mode:
            all_zero = (ref_nodes[n] == 0).all(axis=(0, 2))
            assert (res.factors[n][all_zero] == 0.0).all(), (what, n)
    for n, f in res.factors.items():
        assert np.isfinite(f).all(), (what, n)
    if res.cumulative is not None:
        assert np.isfinite(res.cumulative).all(), what


def check_against_oracle(cs, res, ora, what=""):
    """Values: live site values, every node's partials (relative to the pattern's largest entry), per-node factors and the cumulative buffer."""
    dead = cs.dead
    assert np.array_equal(np.isneginf(ora.site), dead) and not np.isnan(ora.site).any(), what
    assert (res.lnl == ora.lnl) if np.isinf(ora.lnl) else helpers.rel_err(res.lnl, ora.lnl) <= 1e-10, (what, res.lnl, ora.lnl)
    live = ~dead
    if live.any():
        assert np.max(np.abs(res.site[live] - ora.site[live]) / np.abs(ora.site[live])) <= 1e-10, what
    for n, po in ora.partials.items():
        scale = np.maximum(np.abs(po).max(axis=(0, 2), keepdims=True), 1e-300)
        assert np.max(np.abs(res.partials[n] - po) / scale) <= 1e-10, (what, n)
    for n, fo in ora.factors.items():
        assert np.max(np.abs(res.factors[n] - fo)) <= 1e-12, (what, n)
    if ora.cumulative is not None:
        assert np.max(np.abs(res.cumulative - ora.cumulative)) <= 1e-9, what


# ---- part B: zero-length branches and a rate-0 category ---------------------------------------------------------------------------------

def zero_length_workload(S, Cn=4, T=9, P=130, seed=5):
    """Every cherry parent lowered onto its (contemporaneous) tips — both branches of every cherry have length zero —, category 0 at rate
    0, and the tips under each cherry equal or missing: every pattern is live and nothing hangs on the 1e-17 noise off the diagonal
    of U U^-1."""
    wl = helpers.random_workload(T, P, S, Cn, seed=seed, unknown_fraction=0.02)
    tree = wl.tree
    height = tree.height.copy()
    tips = wl.tip_states.copy()
    for n in cherries(tree):
        a, b = int(tree.left[n]), int(tree.right[n])
        height[n] = max(height[a], height[b])
        both = (tips[a] < S) & (tips[b] < S)
        tips[b, both] = tips[a, both]
    rates = wl.cat_rates.copy()
    rates[0] = 0.0
    return synth.Workload("zero-length-S%d" % S, trees.Tree(tree.left, tree.right, height, tree.root), wl.eig, wl.freqs, rates,
                          wl.cat_weights, np.ascontiguousarray(tips), wl.weights, S)


def k3st_eigen(a=0.5, b=0.3, c=0.2):
    """Kimura's three-substitution-type model with Hadamard eigenvectors: U has entries +-1 and U^-1 = U / 4, so U exp(0) U^-1 is the identity
    EXACTLY in any summation order — zero-length branches then give exact zeros through updateTransitionMatrices."""
    from beast_mcmc_amd.inputs.substmodel import EigenDecomposition
    h = np.array([[1, 1, 1, 1], [1, 1, -1, -1], [1, -1, 1, -1], [1, -1, -1, 1]], dtype=np.float64)
    evals = np.array([0.0, -2.0 * (b + c), -2.0 * (a + c), -2.0 * (a + b)])      # q_ij in {a, b, c} > 0
    evals /= 0.25 * (-(evals.sum()))                                              # one expected substitution per unit time
    return EigenDecomposition(h, h / 4.0, evals)


def k3st_dead_workload():
    """4 states, 9 taxa x 131 patterns, K3ST: every cherry parent on its tips, the simulated tips left as they are (many cherries differ).
    -> (workload, {cherry parent: its positive height before})."""
    base = helpers.random_workload(9, 131, 4, 4, seed=5, unknown_fraction=0.02)
    tree = base.tree
    height = tree.height.copy()
    restore = {}
    for n in cherries(tree):
        restore[n] = float(height[n])
        height[n] = 0.0
    wl = synth.Workload("k3st-dead", trees.Tree(tree.left, tree.right, height, tree.root), k3st_eigen(), np.full(4, 0.25), base.cat_rates,
                        base.cat_weights, base.tip_states, base.weights, 4)
    return wl, restore


# ---- part C: stiff regimes -----------------------------------------------------------------------------------------------------------

STIFF_REGIMES = [(80.0, 0.05), (80.0, 0.7), (1.0, 0.02), (2e-6, 0.05), (2e-6, 0.7)]


def stiff_workload(S, factor, alpha):
    """random_workload(9, 130, S, 4, seed=5, unknown_fraction=0.02), simulated BEFORE the heights are multiplied by `factor` (at a
    root-to-tip distance of 1e-6 the simulator cannot produce 130 distinct patterns), rates from GammaSiteRateModel(alpha, 4)."""
    from beast_mcmc_amd.inputs.siterates import GammaSiteRateModel
    wl = helpers.random_workload(9, 130, S, 4, seed=5, unknown_fraction=0.02)
    tree = wl.tree
    rates, props = GammaSiteRateModel(alpha=alpha, gamma_categories=4).category_rates_and_proportions()
    return synth.Workload("stiff-S%d" % S, trees.Tree(tree.left, tree.right, tree.height * factor, tree.root), wl.eig, wl.freqs, rates, props,
                          wl.tip_states, wl.weights, S)


def site_values(wl, library=None, scheme=RESCALE_NONE, precise=False):
    """(lnL, site log-likelihoods) of one evaluation; precise: the oracle's long-double mode, switched off again whatever happens."""
    if precise:
        library.lib.oracle_set_precise(1)
    try:
        tl = BeagleTreeLikelihood(wl, library=library, rescaling=scheme, delay_rescaling=False)
        lnl = tl.getLogLikelihood()
        site = tl.getSiteLogLikelihoods().copy()
        tl.close()
    finally:
        if precise:
            library.lib.oracle_set_precise(0)
    return lnl, site
