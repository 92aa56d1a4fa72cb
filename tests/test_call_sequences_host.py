"""The call-sequence generator (tests/call_sequences.py) on the CPU tier: its records are reproducible and survive JSON, every sequence
is a valid one for the oracle (return code 0 at every call, finite values at every read), every action and motif is really there, and
the inputs are well conditioned — measured, not assumed: each sequence also runs on the oracle's long-double mode
(``oracle_set_precise``), and the largest difference between the two runs over all reads, normalised as the GPU comparison normalises
them (``call_sequences.deviation``), must stay at or below 1e-11: a tenth of the 1e-10 the engine is held to, so that bound has a
decade of margin that belongs to the inputs and not to the engine.

Measured maxima of |oracle - precise oracle| over a shape's seeds (the conditioning test prints them):

    (S, C, T, P)        largest deviation
    (4, 4, 12, 130)     8.4e-15
    (4, 3, 9, 257)      1.1e-14
    (20, 2, 8, 33)      1.2e-14
    (61, 1, 6, 37)      1.1e-14
    (7, 2, 8, 67)       5.4e-15
    (80, 1, 6, 23)      2.2e-14

The same holds for the generator's second profile, "extensions" (the one-call extension entry points and motifs (j)-(m), on the five
shapes of at most 64 states; 4 seeds for a 4-state shape, 2 for the others), whose oracle side is made of the numpy restatements
over the oracle's reads.  Its numeric reads — node-height derivatives, Markov-jump values and the rest — are held to the same 1e-11;
the states and categories of its draws must equal the long-double run's on every decided pattern, a pattern being undecided when some
draw on it lies within 1e-8 x total of a boundary (two decades above the 1e-10 the engine's partials are held to), and at most 1 % of
a sequence's (sampler call, pattern) pairs may be undecided.  Measured: no pair of any sequence is undecided (150 .. 2574 pairs a
sequence), and

    (S, C, T, P)        largest deviation, extensions
    (4, 4, 12, 130)     9.0e-15
    (4, 3, 9, 257)      1.2e-14
    (20, 2, 8, 33)      1.4e-14
    (61, 1, 6, 37)      1.8e-13
    (7, 2, 8, 67)       3.9e-15

And for the third profile, "queries" (updateTransitionMatricesFromGenerators, updateTransitionMatricesWithEpochs, nodePosteriors,
nodePatternLikelihoods, placementScores and motifs (n)-(r), on the same shapes and seeds): posteriors, log pattern values, node terms,
log tables and scores within 1e-11 of the long-double run, MAP states equal to its on every decided pattern (undecided: the two largest
posteriors within 1e-8), at most 1 % of the (sampler or MAP call, pattern) pairs undecided.  No input had to be drawn differently and no
seed replaced: the generator's branch lengths (0.01 .. 1), the code table's real-valued row (0.05 .. 1) and the log weights (-3 .. 0)
keep every log value a few units from 0.  Measured: no pair undecided (0 .. 514 pairs a sequence), and

    (S, C, T, P)        largest deviation, queries
    (4, 4, 12, 130)     9.3e-15
    (4, 3, 9, 257)      1.5e-14
    (20, 2, 8, 33)      1.5e-14
    (61, 1, 6, 37)      2.0e-14
    (7, 2, 8, 67)       1.1e-14

The sequences of the first two profiles are pinned record for record: tests/golden/call_sequence_digests.json holds the sha256 of each
base sequence's dumped file, written before the generator learned the second profile, and
tests/golden/call_sequence_digests_extensions.json those of the extension profile, written before it learned the third.
"""
import collections
import hashlib
import json
import os

import numpy as np
import pytest

import beast_mcmc_amd as bm
import call_sequences as cs

# the smallest shapes that cross a 128-pattern group (4 states), a 32-pattern tile (20, 61 states), a 4 x 4 matrix block edge
# (7 states) and the 64-state limit of the walks (80 states: the level kernels)
SHAPES = [(4, 4, 12, 130), (4, 3, 9, 257), (20, 2, 8, 33), (61, 1, 6, 37), (7, 2, 8, 67), (80, 1, 6, 23)]
SEEDS = {shape: list(range(1, 9 if shape[0] == 4 else 5)) for shape in SHAPES}
CASES = [(shape, seed) for shape in SHAPES for seed in SEEDS[shape]]
CONDITIONING_BOUND = 1e-11
# profile "extensions": the shapes with at most 64 states (several of the calls answer NO_IMPLEMENTATION above), 4 seeds for a 4-state
# shape and 2 for the others.  No seed had to be replaced: every one of them keeps the cap on undecided patterns.
SHAPES_EXT = [s for s in SHAPES if s[0] <= cs.EXT_MAX_STATES]
SEEDS_EXT = {shape: list(range(1, 5 if shape[0] == 4 else 3)) for shape in SHAPES_EXT}
CASES_EXT = [(shape, seed) for shape in SHAPES_EXT for seed in SEEDS_EXT[shape]]
# profile "queries": the same shapes and seeds as "extensions".  No seed had to be replaced here either.
CASES_Q = list(CASES_EXT)
PROFILE_CASES = [c + ("base",) for c in CASES] + [c + ("extensions",) for c in CASES_EXT] + [c + ("queries",) for c in CASES_Q]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DIGESTS = os.path.join(GOLDEN, "call_sequence_digests.json")
DIGESTS_EXT = os.path.join(GOLDEN, "call_sequence_digests_extensions.json")


def seeds_of(shape, profile="base"):
    return SEEDS[shape] if profile == "base" else SEEDS_EXT[shape]


def length_for(seed):
    return 100 + 3 * (seed % 5)                                # 100 .. 112 calls behind the set-up, and what coverage still asks for


_records = {}


def records(shape, seed, profile="base"):
    if (shape, seed, profile) not in _records:
        _records[(shape, seed, profile)] = cs.generate(shape, seed, length_for(seed), profile)
    return _records[(shape, seed, profile)]


def case_id(c):
    return "S%d-C%d-T%d-P%d-seed%d" % (c[0] + (c[1],)) + ("-" + c[2] if len(c) > 2 and c[2] != "base" else "")


def run_on_oracle(shape, recs, oracle_lib, precise=False):
    """-> [(return code, reads, undecided patterns or None)] per record"""
    if precise:
        oracle_lib.lib.oracle_set_precise(1)
    try:
        b = cs.create(shape, bm.beagle.Beagle, library=oracle_lib)
        try:
            out = []
            for r in recs:
                info = {}
                out.append(cs.execute(b, r, "oracle", info) + (info.get("undecided"),))
            return out
        finally:
            b.finalize()
    finally:
        if precise:
            oracle_lib.lib.oracle_set_precise(0)


def test_the_base_sequences_are_record_for_record_what_they_were(tmp_path):
    """The sha256 of every base sequence's dumped file, as written before the generator learned a second profile: their conditioning
    table above and every GPU run so far stay valid."""
    with open(DIGESTS) as f:
        want = json.load(f)
    assert sorted(want) == sorted(case_id(c) for c in CASES)
    path = str(tmp_path / "sequence.json")
    for shape, seed in CASES:
        cs.dump(path, shape, seed, records(shape, seed))
        with open(path, "rb") as f:
            assert hashlib.sha256(f.read()).hexdigest() == want[case_id((shape, seed))], (shape, seed)


def test_the_extension_sequences_are_record_for_record_what_they_were(tmp_path):
    """The same for the extension profile: the sha256 of every one of its sequences' dumped files, written before the generator
    learned the third profile, "queries"."""
    with open(DIGESTS_EXT) as f:
        want = json.load(f)
    assert sorted(want) == sorted(case_id(c + ("extensions",)) for c in CASES_EXT)
    path = str(tmp_path / "sequence.json")
    for shape, seed in CASES_EXT:
        cs.dump(path, shape, seed, records(shape, seed, "extensions"), "extensions")
        with open(path, "rb") as f:
            assert hashlib.sha256(f.read()).hexdigest() == want[case_id((shape, seed, "extensions"))], (shape, seed)


@pytest.mark.parametrize("case", PROFILE_CASES[::5], ids=case_id)
def test_same_seed_same_records_and_json_round_trip(case, tmp_path):
    shape, seed, profile = case
    a = records(shape, seed, profile)
    assert cs.generate(shape, seed, length_for(seed), profile) == a
    assert cs.generate(shape, seed + 100, length_for(seed), profile) != a
    path = str(tmp_path / "sequence.json")
    cs.dump(path, shape, seed, a, profile)
    assert cs.load(path) == (shape, seed, a)
    assert cs.load(path, with_profile=True) == (shape, seed, a, profile)


def prelude_length(shape, seed, profile="base"):
    g = cs.Generator(shape, seed, length_for(seed), profile)
    g.prelude()
    return g.prelude_end


@pytest.mark.parametrize("shape", SHAPES + [s + ("extensions",) for s in SHAPES_EXT] + [s + ("queries",) for s in SHAPES_EXT],
                         ids=lambda s: "S%d-C%d-T%d-P%d" % s[:4] + "".join("-" + x for x in s[4:]))
def test_every_action_and_motif_is_there(shape):
    """Coverage is a condition: over a shape's seeds every action at least 3 times (counted behind the set-up calls), every motif in
    every sequence; a 4-state shape's seeds together hold every variant of the motifs that have variants.  Query profile: every
    sequence also holds an epoch entry with a single segment, a placement candidate above the root and one whose child is a tip."""
    shape, profile = shape[:4], shape[4] if len(shape) > 4 else "base"
    count, variants = collections.Counter(), set()
    for seed in seeds_of(shape, profile):
        recs = records(shape, seed, profile)
        tail = recs[prelude_length(shape, seed, profile):]
        count.update(r["action"] for r in tail)
        assert set(r["motif"] for r in tail if r["motif"]) == set(cs.motifs_for(profile)), seed
        variants |= set((r["motif"], r["variant"]) for r in tail if r["variant"])
        assert all(r["action"] in cs.actions_for(shape[0], profile) for r in recs)
        if profile == "queries":
            epochs = [r["a"][0] for r in recs if r["m"] == "updateTransitionMatricesWithEpochs"]
            assert any(b - a == 1 for off in epochs for a, b in zip(off, off[1:])), seed
            for r in recs:
                if r["m"] == "placementScores":
                    assert 2 <= len(r["a"][0]) <= 6 and len(r["a"][3]) == shape[0] + 1
                    assert any(c[1] == cs.NONE and c[2] == cs.NONE for c in r["a"][0]) and any(c[3] < shape[2] for c in r["a"][0]), seed
    short = {a: count[a] for a in cs.actions_for(shape[0], profile) if count[a] < 3}
    assert not short, short
    if shape[0] == 4:
        want = cs.variants_for(4, profile)
        assert set(v for v in variants if v[0] in set(m for m, _ in want)) == want


def test_the_open_cases_of_the_contract_are_never_emitted():
    for shape, seed, profile in PROFILE_CASES:
        calls = len(records(shape, seed, profile)) - prelude_length(shape, seed, profile)
        assert 80 <= calls <= (120 if profile == "base" else 260), (shape, seed, profile, calls)   # (13 motifs instead of 9, and 60 drawn calls at the least)
        for r in records(shape, seed, profile):
            m, a = r["m"], r["a"]
            if m in ("updatePartials", "updatePrePartials"):
                for k in range(a[1]):
                    op = a[0][7 * k:7 * k + 7]
                    assert op[0] not in (op[3], op[5])
            elif m in ("convolveTransitionMatrices", "addTransitionMatrices"):
                assert all(r_ not in (f, s) for f, s, r_ in zip(*a[:3]))
            elif m == "transposeTransitionMatrices":
                assert all(i != o for i, o in zip(a[0], a[1]))
            elif m == "calculateRootLogLikelihoods":
                assert a[4] == 1
            elif m in ("updateTransitionMatricesFromGenerators", "updateTransitionMatricesWithEpochs"):
                slots = a[3] if m.endswith("Generators") else a[4]
                assert len(set(slots)) == len(slots) == a[-1]                  # (no slot twice in one call)
            elif m.startswith("updateTransitionMatrices"):
                assert a[-4] is None and a[-3] is None


_worst = collections.defaultdict(float)


@pytest.mark.parametrize("case", PROFILE_CASES, ids=case_id)
def test_sequence_is_valid_and_well_conditioned_on_the_oracle(case, oracle_lib):
    """Every numeric read within CONDITIONING_BOUND of the long-double run; the states and categories of every draw equal to the
    long-double run's on every decided pattern, and undecided patterns (some draw within 1e-8 x total of a boundary: two decades
    above the 1e-10 partials are held to) at most 1 % of the sequence's (sampler call, pattern) pairs."""
    shape, seed, profile = case
    recs = records(shape, seed, profile)
    plain = run_on_oracle(shape, recs, oracle_lib)
    precise = run_on_oracle(shape, recs, oracle_lib, precise=True)
    worst, reads, pairs, undecided = 0.0, 0, 0, 0
    for step, (rec, (rc, got, und), (rc_p, want, _)) in enumerate(zip(recs, plain, precise)):
        assert rc == 0 and rc_p == 0, (step, cs.describe(rec), rc, rc_p)
        assert len(got) == len(want)
        if und is not None:
            pairs += und.size
            undecided += int(und.sum())
        for (kind, g), (_, w) in zip(got, want):
            assert np.isfinite(g).all() and np.isfinite(w).all(), (step, cs.describe(rec))
            d = cs.deviation(kind, g, w, undecided=und)
            assert d <= CONDITIONING_BOUND, (step, cs.describe(rec), kind, d)
            worst = max(worst, d)
            reads += 1
    assert reads >= 30
    assert undecided <= cs.UNDECIDED_CAP * pairs, (undecided, pairs)
    _worst[(shape, profile)] = max(_worst[(shape, profile)], worst)
    print("shape %s seed %d %s: %d reads, |oracle - precise| at most %.2e (so far over the shape's seeds: %.2e); %d of %d (sampler call, "
          "pattern) pairs undecided" % (shape, seed, profile, reads, worst, _worst[(shape, profile)], undecided, pairs))


def test_deviation_of_the_new_kinds_sees_what_it_should():
    """An eigen system is compared through what it reconstructs (a column's sign and scale are free, the values are not); states and
    categories on the decided patterns only; "exact" is the side's own count."""
    rng = np.random.default_rng(5)
    u, ui, lam, _, q = cs.reversible_model(rng, 7)
    flip = np.array([1.0, -1.0, 2.0, 1.0, -0.5, 1.0, 1.0])
    same = cs.packed_eigen(u * flip[None, :], ui / flip[:, None], lam)
    assert cs.deviation("eigen", same, cs.packed_eigen(u, ui, lam)) <= 1e-14
    off = lam.copy()
    off[3] *= 1.0 + 1e-8
    assert cs.deviation("eigen", cs.packed_eigen(u, ui, off), cs.packed_eigen(u, ui, lam)) > 1e-10
    assert cs.deviation("eigen", cs.packed_eigen(u, ui * (1.0 + 1e-8), lam), cs.packed_eigen(u, ui, lam)) > 1e-10
    a = rng.integers(0, 4, size=(5, 9)).astype(np.uint8)
    b = a.copy()
    b[2, 4] ^= 1
    und = np.zeros(9, dtype=bool)
    assert cs.deviation("states", a, a.copy(), undecided=und) == 0.0
    assert cs.deviation("states", b, a, undecided=und) == 1.0 and cs.deviation("states", b, a) == 1.0
    und[4] = True
    assert cs.deviation("states", b, a, undecided=und) == 0.0
    assert cs.deviation("cats", b[2], a[2], undecided=und) == 0.0 and cs.deviation("cats", b[2], a[2]) == 1.0
    assert cs.deviation("exact", np.array([0.0]), np.array([0.0])) == 0.0
    assert cs.deviation("exact", np.array([3.0]), np.array([0.0])) > 1.0 and cs.deviation("exact", np.array([3.0]), np.array([3.0])) > 1.0
    assert cs.deviation("jumps", np.array([2.0, 1e-9]), np.array([2.0, 0.0])) == pytest.approx(5e-10)
    # the query profile's kinds: posteriors (and category posteriors, MAP probabilities, totals over the sum of the pattern weights)
    # by their absolute difference; a log value against max(1, |value|); MAP states on the decided patterns only
    post = rng.dirichlet(np.full(4, 2.0), size=(3, 9))
    off = post.copy()
    off[1, 4, 2] += 1e-8
    assert cs.deviation("posterior", post, post.copy()) == 0.0
    assert cs.deviation("posterior", off, post) == pytest.approx(1e-8) and cs.deviation("posterior", off, post) > cs.BOUND
    logs = np.array([[-0.02, -5.0], [-700.0, -1e-12]])
    assert cs.deviation("logval", logs, logs.copy()) == 0.0
    assert cs.deviation("logval", logs + np.array([[1e-8, 0.0], [0.0, 0.0]]), logs) == pytest.approx(1e-8)     # (a value near 0: absolute)
    assert cs.deviation("logval", logs * np.array([[1.0, 1.0], [1.0 + 1e-8, 1.0]]), logs) == pytest.approx(1e-8, rel=1e-3)
    assert cs.deviation("logval", logs * np.array([[1.0, 1.0], [1.0 + 1e-12, 1.0]]), logs) < cs.BOUND
    assert cs.deviation("logval", np.array([-np.inf]), np.array([-np.inf])) != cs.deviation("logval", np.array([-np.inf]), np.array([-np.inf]))
    assert cs.deviation("sum", np.array([-1234.5 * (1.0 + 1e-8)]), np.array([-1234.5])) == pytest.approx(1e-8, rel=1e-3)
    ms = np.argmax(post, axis=2).astype(np.uint8)
    other = ms.copy()
    other[0, 7] = (other[0, 7] + 1) % 4
    und = np.zeros(9, dtype=bool)
    assert cs.deviation("states", other, ms, undecided=und) == 1.0
    und[7] = True
    assert cs.deviation("states", other, ms, undecided=und) == 0.0


def test_a_draw_next_to_a_boundary_is_reported_undecided():
    """The margin output of the two sampler restatements: 1e-8 x total around every running sum, and around a tie under MAP."""
    import ancestral_reference as ar
    import simulate_reference as sr
    w = [np.array([0.25, 0.25, 0.25]), np.array([0.25, 0.25, 0.2500000001]), np.array([0.5, 0.5, 0.5])]
    u = np.array([0.25 + 5e-9, 0.25 + 5e-8, 0.6])
    assert ar.near_a_boundary(w, u, False).tolist() == [True, False, False]
    assert ar.near_a_boundary(w, u, True).tolist() == [False, False, False]
    assert ar.near_a_boundary([w[0], w[1]], u, True).tolist() == [True, True, True]
    cum, last, bad = sr.cumulative(np.array([[0.1, 0.2, 0.7]] * 3))
    und = np.zeros(3, dtype=bool)
    sr.draw(cum, last, bad, np.array([0.3 - 5e-9, 0.3 + 5e-8, 0.999]), und)
    assert und.tolist() == [True, False, False]


def worst_over(shape, recs, other, pairs, oracle_lib):
    """both record lists on the oracle -> the largest deviation over the reads of the record pairs (index in recs, index in other)"""
    a, b = run_on_oracle(shape, recs, oracle_lib), run_on_oracle(shape, other, oracle_lib)
    worst = 0.0
    for i, j in pairs:
        assert a[i][0] == 0 and b[j][0] == 0 and len(a[i][1]) == len(b[j][1])
        for (kind, g), (_, w) in zip(a[i][1], b[j][1]):
            if kind not in ("states", "cats", "exact"):
                worst = max(worst, cs.deviation(kind, g, w))
    return worst


@pytest.mark.parametrize("case", [c for c in CASES_EXT if c[0][0] == 4], ids=case_id)
def test_motifs_k_and_m_would_show_the_wrong_decision(case, oracle_lib):
    """The two motifs whose point is an upload or a list that must NOT be skipped or run late, played wrongly on the oracle: (k,
    variant "reupload") without the setEigenDecomposition behind setReversibleModels — what a stale upload shadow would do — and (m)
    with the pre-order list run only after the branch's matrix was overwritten and put back — what a list left held would do.  The
    motif's own reads must then differ from the right order's by far more than the bound the engine is held to."""
    shape, seed = case
    recs = records(shape, seed, "extensions")
    k = [i for i, r in enumerate(recs) if r["motif"] == "k"]
    if recs[k[0]]["variant"] == "reupload":
        drop = [i for i in k if recs[i]["m"] == "setEigenDecomposition"]
        assert len(drop) == 1 and recs[drop[0] - 1]["m"] == "setReversibleModels"
        other = recs[:drop[0]] + recs[drop[0] + 1:]
        assert worst_over(shape, recs, other, [(i, i - 1) for i in k if i > drop[0]], oracle_lib) > 1e4 * cs.BOUND
    m = [i for i, r in enumerate(recs) if r["motif"] == "m"]
    assert [recs[i]["m"] for i in m[-4:]] == ["updatePrePartials", "updateDifferentialMatrices", "updateTransitionMatrices", "getPartials"]
    other = list(recs)
    other[m[-4]:m[-1]] = [recs[m[-3]], recs[m[-2]], recs[m[-4]]]
    assert worst_over(shape, recs, other, [(m[-1], m[-1])], oracle_lib) > 1e4 * cs.BOUND


@pytest.mark.parametrize("case", [c for c in CASES_Q if c[0][0] == 4], ids=case_id)
def test_motifs_n_p_and_r_would_show_the_wrong_decision(case, oracle_lib):
    """The same for the query profile's motifs, whichever of them the seed holds in the variant that matters: (p) without "_spare"
    with the pre-order list run only after the branch's matrix was rewritten — what a list left held would do; (r, variant
    "reupload") without the setEigenDecomposition behind setReversibleModels; (n, variant "set_pre") with the posteriors taken
    before the setPartials into the pre-order buffer — what a call that did not see the write would return."""
    shape, seed = case
    recs = records(shape, seed, "queries")
    played = 0
    p = [i for i, r in enumerate(recs) if r["motif"] == "p"]
    if not recs[p[0]]["variant"].endswith("_spare"):
        assert [recs[i]["m"] for i in p[-5:-3]] + [recs[i]["m"] for i in p[-3:]] == \
            ["updatePrePartials", recs[p[-4]]["m"], "calculateEdgeDifferentials", "getPartials", "updateTransitionMatrices"]
        assert recs[p[-4]]["m"] in ("updateTransitionMatricesFromGenerators", "updateTransitionMatricesWithEpochs")
        other = list(recs)
        other[p[-5]], other[p[-4]] = recs[p[-4]], recs[p[-5]]
        assert worst_over(shape, recs, other, [(p[-3], p[-3]), (p[-2], p[-2])], oracle_lib) > 1e4 * cs.BOUND
        played += 1
    r = [i for i, x in enumerate(recs) if x["motif"] == "r"]
    if recs[r[0]]["variant"] == "reupload":
        drop = [i for i in r if recs[i]["m"] == "setEigenDecomposition"]
        assert len(drop) == 1 and recs[drop[0] - 1]["m"] == "setReversibleModels"
        other = recs[:drop[0]] + recs[drop[0] + 1:]
        assert worst_over(shape, recs, other, [(i, i - 1) for i in r if i > drop[0]], oracle_lib) > 1e4 * cs.BOUND
        played += 1
    n = [i for i, x in enumerate(recs) if x["motif"] == "n"]
    if recs[n[0]]["variant"] == "set_pre":
        assert [recs[i]["m"] for i in n[-4:]] == ["updatePrePartials", "setPartials", "nodePosteriors", "calculateEdgeDifferentials"]
        other = list(recs)
        other[n[-3]], other[n[-2]] = recs[n[-2]], recs[n[-3]]
        assert worst_over(shape, recs, other, [(n[-2], n[-3])], oracle_lib) > 1e4 * cs.BOUND
        played += 1
    assert played, "each of the seeds 1 .. 4 holds one of the three at the least"
