"""Rate-category counts above the ones the rest of the suite uses: shapes, builders, the recorded evaluation and its checkers
(tests/test_category_counts_host.py, tests/test_gpu_category_counts.py).  Plain Python: no library is loaded at import.

The engine branches on the category count C where the 4-state walk's templates end (4, 8, 16), where the hold slots drop from three to
two (above 8), where every walk ends (above 16: engine_create.cpp in->walk / in->walkT) and where k_transition4Fused stops staging the
rates in LDS (above 16).  9 is the first count on the 16-wide templates, 16 the last on the walks, 17 the first off them, 32 twice the
limit.  16 appears only where the 16 / 17 pair is contrasted.

The checkers take two recorded evaluations (engine and oracle, or oracle and a perturbed oracle) and nothing else, so the CPU tier runs
them on the oracle against an oracle whose category weights are rolled by one position: each of them must then fail."""
import numpy as np

COUNTS = (9, 17, 32)
CONTRAST = (16, 17)                                      # the last count on the walks and the first off them
# (S, T, P): the smallest that still cross a 128-pattern group, a 32-pattern tile and a ragged tail
SHAPES = [(4, 10, 130), (4, 12, 257), (7, 8, 67), (20, 8, 33), (20, 10, 130), (61, 6, 37), (64, 5, 65), (80, 5, 23)]
REL_TOL = 1e-10                                          # the project's bound on the engine
ORACLE_TOL = 1e-12                                       # the oracle against the long-double pruning reference (test_degenerate_host.py)
STEPS = ("first", "move 0", "restore 0", "move 1", "restore 1", "model")

_workloads = {}


def counts_for(S):
    """The category counts of the likelihood cases: 9, 17, 32, and 16 as well at 4 states."""
    return (9, 16, 17, 32) if S == 4 else COUNTS


def likelihood_cases():
    return [(S, T, P, C) for (S, T, P) in SHAPES for C in counts_for(S)]


def case_id(case):
    return "S%d-T%d-P%d-C%d" % tuple(case)


def workload(S, T, P, C):
    """helpers.random_workload (5 % unknown tip states), seeded by the shape; cached and never modified."""
    import helpers
    key = (S, T, P, C)
    if key not in _workloads:
        _workloads[key] = helpers.random_workload(T, P, S, C, seed=4000 + 131 * S + 17 * C + T + P)
    return _workloads[key]


def second_model(wl):
    """Another substitution model and another site model with the same category count: (eig, freqs, rates, weights)."""
    from beast_mcmc_amd.inputs import substmodel
    from beast_mcmc_amd.inputs.siterates import GammaSiteRateModel
    S, C = wl.state_count, wl.category_count
    rng = np.random.default_rng(900 + S + C)
    if S == 4:
        pi = rng.dirichlet(np.full(4, 10.0))
        eig = substmodel.gtr(rng.gamma(2.0, 1.0, size=6) + 0.1, pi)
    else:
        eig, pi = substmodel.random_reversible(S, rng)
    rates, weights = GammaSiteRateModel(alpha=1.3, gamma_categories=C).category_rates_and_proportions()
    return eig, np.asarray(pi, dtype=np.float64), np.asarray(rates, dtype=np.float64), np.asarray(weights, dtype=np.float64)


def uneven_weights(C, seed=1):
    """Category weights that differ from one category to the next (a gamma model's are all 1 / C, which a rolled copy equals)."""
    w = np.random.default_rng(seed).uniform(0.5, 1.5, size=C)
    return w / w.sum()


def transition_rates(C, which=0):
    """Strictly increasing, strictly positive rates with mean 1 under equal weights; `which` picks one of several distinct sets."""
    r = np.linspace(0.05, 2.0, C) ** (1.0 + 0.5 * which)
    return r / r.mean()


# ---- the recorded evaluation: the same calls on the engine and on the oracle --------------------------------------------------------

class Snapshot:
    """What one evaluation left behind: lnL, site values, every internal node's partials, every scale buffer, the branch matrices."""


def snapshot(tl, raw, label, matrices=False):
    import beast_mcmc_amd as bm
    NONE = bm.beagle.NONE
    tree = tl.tree
    T = tree.tip_count
    s = Snapshot()
    s.label = label
    s.lnl = tl.getLogLikelihood()
    s.site = tl.getSiteLogLikelihoods().copy()
    s.partials = {n: raw.getPartials(tl.node_buffer_index(n), NONE).copy() for n in range(T, tree.node_count)}
    cum = tl.cumulative_scale_index()
    s.scaled = cum != NONE
    s.factors = {n: raw.getLogScaleFactors(tl.node_scale_index(n)).copy() for n in range(T, tree.node_count)} if s.scaled else {}
    s.cumulative = raw.getLogScaleFactors(cum).copy() if s.scaled else None
    s.mats = ({n: raw.getTransitionMatrix(tl.node_matrix_index(n)).copy() for n in range(tree.node_count) if n != tree.root}
              if matrices else None)
    return s


def run_sequence(wl, scheme, library=None, matrices=False, roll_weights=False, stats=None):
    """A full evaluation, two branch moves (helpers.proposed_height) each followed by a restore, a model move: a Snapshot after each.
    roll_weights: every site model is installed with its category weights rolled by one position (the perturbation of the CPU tier).
    stats: a dict that receives the engine's walk counters (walkStats, walkLaunchInfo) of the whole sequence."""
    import beast_mcmc_amd as bm
    import helpers
    from beast_mcmc_amd.treelikelihood import BeagleTreeLikelihood
    tl = BeagleTreeLikelihood(wl, library=library, rescaling=scheme, delay_rescaling=False)
    raw = bm.beagle.Beagle.attach(tl)
    roll = (lambda w: np.roll(w, 1)) if roll_weights else (lambda w: w)
    out = []
    try:
        if roll_weights:
            tl.set_site_model(wl.cat_rates, roll(np.asarray(wl.cat_weights)))
        out.append(snapshot(tl, raw, STEPS[0], matrices))
        rng = np.random.default_rng(77)
        tree = wl.tree
        for move in range(2):
            node = int(rng.integers(tree.tip_count, tree.node_count))
            tl.storeState()
            tl.set_node_height(node, helpers.proposed_height(tree, node, rng))
            out.append(snapshot(tl, raw, "move %d" % move, matrices))
            tl.restoreState()
            tl.restore_node_height(node, float(tree.height[node]))
            out.append(snapshot(tl, raw, "restore %d" % move, matrices))
        eig, freqs, rates, weights = second_model(wl)
        tl.storeState()
        tl.set_substitution_model(eig, freqs)
        tl.set_site_model(rates, roll(uneven_weights(len(rates))))
        out.append(snapshot(tl, raw, "model", matrices))
        if stats is not None:
            stats.update(raw.walkStats())
            stats.update(raw.walkLaunchInfo())
    finally:
        tl.close()
    assert [s.label for s in out] == list(STEPS)
    return out


def _rel(a, b):
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300)))


def check_sequences(got, want, what="", tol=REL_TOL, worst=None):
    """Every step of `got` against `want` (the oracle on the same calls): lnL, every site value, every internal node's partials (per pattern,
    relative to the pattern's largest entry, as test_gpu_parity.test_engine_matches_oracle does) and every scale buffer.
    worst: a dict that collects the largest deviation seen per quantity."""
    assert len(got) == len(want) == len(STEPS)
    worst = {} if worst is None else worst

    def note(key, v):
        worst[key] = max(worst.get(key, 0.0), float(v))

    for a, b in zip(got, want):
        tag = "%s, %s" % (what, b.label)
        assert np.isfinite(b.lnl) and np.isfinite(b.site).all(), tag
        note("lnL", abs(a.lnl - b.lnl) / max(abs(b.lnl), 1e-300))
        note("site", _rel(a.site, b.site))
        assert abs(a.lnl - b.lnl) / max(abs(b.lnl), 1e-300) <= tol, ("lnL", tag, a.lnl, b.lnl)
        assert _rel(a.site, b.site) <= tol, ("site values", tag, _rel(a.site, b.site))
        assert a.scaled == b.scaled and set(a.partials) == set(b.partials), tag
        for n, po in b.partials.items():
            scale = np.maximum(np.abs(po).max(axis=(0, 2), keepdims=True), 1e-300)
            err = float(np.max(np.abs(a.partials[n] - po) / scale))
            note("partials", err)
            assert err <= tol, ("partials", tag, n, err)
        for n, fo in b.factors.items():
            err = float(np.max(np.abs(a.factors[n] - fo)))
            note("factors", err)
            assert err <= tol, ("scale factors", tag, n, err)      # (absolute on a logarithm = relative on the factor, a partial's largest entry)
        if b.cumulative is not None:
            err = float(np.max(np.abs(a.cumulative - b.cumulative)))
            note("cumulative", err)
            assert err <= tol, ("cumulative buffer", tag, err)     # (a scale buffer like the others: the same bound)
    # the restores bring back the first evaluation (same buffers as before the move, or the same arithmetic again)
    for k in (2, 4):
        assert abs(got[k].lnl - got[0].lnl) / abs(got[0].lnl) <= 1e-12, ("restored lnL", what, STEPS[k])
    return worst


def check_against_prune(wl, steps, what="", tol=REL_TOL, worst=None):
    """Every step's site values against degenerate_cases.reference_prune in np.longdouble over the matrices the SAME instance read back
    (getTransitionMatrix), with the weights and frequencies the caller believes it installed (wl's, second_model's)."""
    import degenerate_cases as dc
    eig, freqs, rates, _ = second_model(wl)
    worst = {} if worst is None else worst
    for s in steps:
        assert s.mats is not None
        w, f = (uneven_weights(len(rates)), freqs) if s.label == "model" else (wl.cat_weights, wl.freqs)
        ref_site, _ = dc.reference_prune(wl.tree, wl.tip_states, wl.state_count, s.mats, w, f)
        rs = ref_site.astype(np.float64)
        assert np.isfinite(rs).all(), (what, s.label)
        if not s.label.startswith("restore"):
            # (a restore evaluates nothing — the host driver flips its indices back and returns the stored lnL —, so the site values an
            # instance holds after it are still the rejected move's: there the reference checks the restored matrices through lnL alone)
            err = _rel(s.site, rs)
            worst["prune"] = max(worst.get("prune", 0.0), err)
            assert err <= tol, (what, s.label, err)
        total = float(np.dot(ref_site, wl.weights.astype(np.longdouble)))
        assert abs(s.lnl - total) / abs(total) <= tol, (what, s.label)
    return worst


# ---- transition matrices ------------------------------------------------------------------------------------------------------------

def matrix_cases():
    """(S, C, complex): real eigen systems at 4, 7, 20, 61 and 100 states, complex ones (test_oracle_golden._cyclic_model) at 4 and 7;
    C = 17 and 32, and 9 and 16 as well at 4 states."""
    out = []
    for S in (4, 7, 20, 61, 100):
        for C in ((9, 16, 17, 32) if S == 4 else (17, 32)):
            out.append((S, C, False))
            if S in (4, 7):
                out.append((S, C, True))
    return out


MATRIX_LENGTHS = np.array([0.0, 1e-3, 0.07, 0.3, 1.1, 2.5])
MATRIX_TOL = 1e-12                                        # absolute (test_gpu_parity.test_complex_eigen_instance_against_oracle)


def matrix_models(S, complex_eigen):
    """Two models -> [(Q normalised to one substitution per unit time, eigen system)]."""
    from beast_mcmc_amd.inputs import substmodel
    out = []
    for k in range(2):
        if complex_eigen:
            from test_oracle_golden import _cyclic_model
            qn, _, eig = _cyclic_model(S, 3 + S + 10 * k)
        else:
            rng = np.random.default_rng(50 + S + k)
            if S == 4:
                eig = substmodel.gtr(rng.gamma(2.0, 1.0, size=6) + 0.1, rng.dirichlet(np.full(4, 10.0)))
            else:
                eig, _ = substmodel.random_reversible(S, rng)
            qn = (eig.evec * eig.evals[None, :S]) @ eig.ievc
        out.append((qn, eig))
    return out


def matrix_instance(S, C, complex_eigen, library=None):
    import beast_mcmc_amd as bm
    flags = bm.beagle.FLAG_EIGEN_COMPLEX if complex_eigen else 0
    return bm.beagle.Beagle(3, 5, 3, S, 10, 2, 2 * len(MATRIX_LENGTHS) + 2, C, 0, requirementFlags=flags, library=library)


def run_matrices(S, C, complex_eigen, library=None, roll_rates=False):
    """-> (models, rate sets, {"single": [branch][C][S][S], "alone": the same from calls that name one branch each,
    "multi": [branch][C][S][S] with model and rate set alternating by branch, "multi_alone": ...}).
    roll_rates: the rate sets are installed rolled by one position (the perturbation of the CPU tier: matrices do not read weights)."""
    models = matrix_models(S, complex_eigen)
    rates = [transition_rates(C, 0), transition_rates(C, 1)]
    b = matrix_instance(S, C, complex_eigen, library)
    n = len(MATRIX_LENGTHS)
    try:
        for k, (_, eig) in enumerate(models):
            b.setEigenDecomposition(k, eig.evec, eig.ievc, eig.evals)
        installed = [np.roll(r, 1) for r in rates] if roll_rates else rates
        b.setCategoryRates(installed[0])
        b.setCategoryRatesWithIndex(1, installed[1])
        out = {}
        idx = np.arange(n)
        b.updateTransitionMatrices(0, idx, None, None, MATRIX_LENGTHS, n)
        out["single"] = np.stack([b.getTransitionMatrix(int(i)) for i in idx])
        alone = []
        for i in idx:
            b.updateTransitionMatrices(0, [n + int(i)], None, None, [MATRIX_LENGTHS[i]], 1)
            alone.append(b.getTransitionMatrix(n + int(i)))
        out["alone"] = np.stack(alone)
        which = idx % 2                                         # branch i: model i % 2 with rate set (i // 2) % 2
        rset = (idx // 2) % 2
        b.updateTransitionMatricesWithMultipleModels(which, rset, idx, None, None, MATRIX_LENGTHS, n)
        out["multi"] = np.stack([b.getTransitionMatrix(int(i)) for i in idx])
        alone = []
        for i in idx:
            b.updateTransitionMatricesWithMultipleModels([which[i]], [rset[i]], [n + int(i)], None, None, [MATRIX_LENGTHS[i]], 1)
            alone.append(b.getTransitionMatrix(n + int(i)))
        out["multi_alone"] = np.stack(alone)
        out["which"], out["rset"] = which, rset
    finally:
        b.finalize()
    return models, rates, out


def check_matrices(models, rates, out, what="", worst=None):
    """Every category's matrix against scipy.linalg.expm(Q t r_c) at 1e-12 absolute; bit for bit against the one-branch calls."""
    import scipy.linalg
    worst = {} if worst is None else worst
    err = 0.0
    for i, t in enumerate(MATRIX_LENGTHS):
        for c in range(len(rates[0])):
            err = max(err, float(np.max(np.abs(out["single"][i][c] - scipy.linalg.expm(models[0][0] * (t * rates[0][c]))))))
            q, r = models[out["which"][i]][0], rates[out["rset"][i]]
            err = max(err, float(np.max(np.abs(out["multi"][i][c] - scipy.linalg.expm(q * (t * r[c]))))))
    worst["matrices"] = max(worst.get("matrices", 0.0), err)
    assert err <= MATRIX_TOL, (what, err)
    assert np.array_equal(out["single"], out["alone"]), what
    assert np.array_equal(out["multi"], out["multi_alone"]), what
    return worst


# ---- gradients ----------------------------------------------------------------------------------------------------------------------

GRADIENT_CASES = ([(S, T, P, C) for (S, T, P) in ((4, 10, 130), (4, 12, 257)) for C in (9, 16, 17, 32)] +
                  [(20, 8, 33, 17), (61, 6, 37, 17), (7, 8, 67, 17)])
NODE_HEIGHT_CASES = [(S, T, P, C) for (S, T, P) in ((4, 10, 130), (20, 8, 33)) for C in (17, 32)]


def gradient_workload(S, T, P, C):
    """The likelihood workload of the shape with category weights that are not all equal (a rolled copy then differs)."""
    from beast_mcmc_amd.inputs import synth
    wl = workload(S, T, P, C)
    return synth.Workload(wl.name + "-w", wl.tree, wl.eig, wl.freqs, wl.cat_rates, uneven_weights(C, seed=3), wl.tip_states, wl.weights, S)


def rolled(wl):
    """wl with its category weights rolled by one position."""
    from beast_mcmc_amd.inputs import synth
    return synth.Workload(wl.name + "-rolled", wl.tree, wl.eig, wl.freqs, wl.cat_rates, np.roll(wl.cat_weights, 1), wl.tip_states,
                          wl.weights, wl.state_count)


class GradientRecord:
    """lnL, first and second derivatives, per-pattern derivatives, cross products and every pre-order partial of one BranchGradient."""


def record_gradient(g, stats_after=None):
    """Three evaluations (the first, the one a held list answers, the one that asks for everything).  stats_after: a list that receives
    gradientStats() after each evaluation and after the read of the pre-order partials in between (engine only)."""
    r = GradientRecord()
    note = (lambda: stats_after.append(g.b.gradientStats())) if stats_after is not None else (lambda: None)
    r.before = g.log_likelihood()
    r.first = g.gradient(); note()
    r.second = g.gradient(); note()
    root = g.wl.tree.root
    r.pre_held = {n: g.pre_partials(n).copy() for n in range(g.N) if n != root}; note()
    r.full = g.gradient(second=True, per_pattern=True); note()
    r.cross = g.cross_products().copy()
    r.pre = {n: g.pre_partials(n).copy() for n in range(g.N) if n != root}
    r.after = g.log_likelihood()
    r.branch_lengths = g.branch_lengths.copy()
    return r


def close(a, b, what, tol=REL_TOL, worst=None, key=None):
    """The `close` of tests/test_gpu_gradients.py."""
    a, b = np.asarray(a, dtype=float).ravel(), np.asarray(b, dtype=float).ravel()
    scale = max(1.0, float(np.max(np.abs(b))))
    err = float(np.max(np.abs(a - b))) / scale
    if worst is not None:
        worst[key or what] = max(worst.get(key or what, 0.0), err)
    assert err <= tol, (what, err)


def check_node_heights(got, want, tip_count, what="", worst=None):
    """(lnL, first, second) of beagleMi355NodeHeightDerivatives against the restatement's, under `close`."""
    (lnl, first, second), (lo, fo, so) = got, want
    assert np.shape(first) == np.shape(second) == (tip_count - 1,), what
    close(lnl, lo, what + " lnL", worst=worst, key="lnL")
    close(first, fo, what + " first", worst=worst, key="first")
    close(second, so, what + " second", worst=worst, key="second")


def check_gradients(wl, got, want, what="", worst=None, rescale=False):
    C, P, S = wl.category_count, wl.pattern_count, wl.state_count
    for name in ("first", "second"):
        a, b = getattr(got, name), getattr(want, name)
        close(a[0], b[0], "%s lnL (%s evaluation)" % (what, name), worst=worst, key="lnL")
        close(a[1], b[1], "%s gradient (%s evaluation)" % (what, name), worst=worst, key="gradient")
    (lg, gg, hg, pg), (lo, go, ho, po) = got.full, want.full
    close(lg, lo, what + " lnL", worst=worst, key="lnL")
    close(gg, go, what + " gradient", worst=worst, key="gradient")
    close(hg, ho, what + " second derivatives", worst=worst, key="second")
    close(pg, po, what + " per-pattern derivatives", worst=worst, key="per-pattern")
    close(got.cross, want.cross, what + " cross products", worst=worst, key="cross")
    for pre_g, pre_o in ((got.pre_held, want.pre_held), (got.pre, want.pre)):
        for n, b in pre_o.items():
            a, b = pre_g[n].reshape(C, P, S), b.reshape(C, P, S)
            ref = np.maximum(np.max(np.abs(b), axis=(0, 2), keepdims=True), 1e-300)
            err = float(np.max(np.abs(a - b) / ref))
            if worst is not None:
                worst["pre-order"] = max(worst.get("pre-order", 0.0), err)
            assert err <= REL_TOL, (what, n, err)
    # the cross products' exact direction (scaling Q scales every branch): sum_ij Q_ij dlnL/dQ_ij = sum_n t_n dlnL/dt_n
    q = (wl.eig.evec * wl.eig.evals[None, :]) @ wl.eig.ievc
    lhs, rhs = float(np.sum(q * got.cross)), float(np.dot(got.branch_lengths, gg))
    assert abs(lhs - rhs) / max(abs(rhs), 1e-300) <= 1e-9, (what, lhs, rhs)
    # the likelihood path is undisturbed: the evaluation after the three gradients gives the bits of the one right before the last of them
    # (lg) and, without rescaling, the bits of the evaluation made before the first; with rescaling an instance's FIRST evaluation runs
    # another plan than its later ones and agrees with them to rounding only
    assert got.after == lg, ("lnL after the gradient", what, got.after, lg)
    if rescale:
        assert abs(got.before - got.after) <= 1e-12 * abs(lg), ("lnL before and after", what, got.before, got.after)
    else:
        assert got.before == got.after, ("lnL before and after", what, got.before, got.after)


# ---- one-call entry points -------------------------------------------------------------------------------------------------------------

SAMPLER_SHAPES = [(4, 10, 130), (20, 8, 33), (61, 6, 37)]          # sampleAncestralStates
JUMP_SHAPES = [(4, 10, 130), (20, 8, 33)]                          # sampleMarkovJumps, integrated and uniformized
SIMULATE_SHAPES = [(4, 10), (61, 6)]                               # simulateSequences: (S, T), 5 and 259 sites
SIMULATE_SITES = (5, 259)
HISTORY_SHAPES = [(4, 10), (20, 8)]                                # simulateCompleteHistories: (S, T), 130 sites
HISTORY_SITES = 130
DIFFERENTIAL_STATES = (4, 20, 61)                                  # updateDifferentialMatrices
EMISSION_SHAPES = [(4, 10, 130), (20, 10, 130)]                    # setTipEmission
_histories = {}


def history_case(S, T, C):
    """A case of tests/complete_history_cases.py (its builder's layout: pre-order rows, three registers — all jumps, a reward, a random
    labelling) at C categories and HISTORY_SITES sites."""
    from types import SimpleNamespace
    import complete_history_cases as hc
    import helpers
    key = (S, T, C)
    if key not in _histories:
        seed = 700 + S + C
        wl = helpers.random_workload(T, 2, S, C, seed=seed, root_to_tip=2.0)      # (its tree and model only)
        rng = np.random.default_rng(seed)
        regs, flags = hc.registers(S, 3, rng)
        rows, order = hc.tree_rows(wl.tree)
        lengths = np.array([0.0 if r == 0 else wl.tree.branch_length(int(n)) for r, n in enumerate(order)])
        heights = np.array([wl.tree.height[int(n)] for n in order], dtype=np.float64)
        c = SimpleNamespace(name="S%d-C%d" % (S, C), S=S, C=C, K=3, sites=HISTORY_SITES, seed=seed, tree=wl.tree, rows=rows, order=order,
                            lengths=lengths, heights=heights, Q=hc.q_of(wl.eig)[None], registers=regs, flags=flags,
                            cat_rates=np.array(wl.cat_rates, dtype=np.float64), cat_weights=uneven_weights(C, seed=5),
                            freqs=np.array(wl.freqs, dtype=np.float64))
        _histories[key] = (c, hc.restate(c))
    return _histories[key]
