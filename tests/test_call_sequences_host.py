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
"""
import collections

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


def length_for(seed):
    return 100 + 3 * (seed % 5)                                # 100 .. 112 calls behind the set-up, and what coverage still asks for


_records = {}


def records(shape, seed):
    if (shape, seed) not in _records:
        _records[(shape, seed)] = cs.generate(shape, seed, length_for(seed))
    return _records[(shape, seed)]


def case_id(c):
    return "S%d-C%d-T%d-P%d-seed%d" % (c[0] + (c[1],))


def run_on_oracle(shape, recs, oracle_lib, precise=False):
    """-> [(return code, reads)] per record"""
    if precise:
        oracle_lib.lib.oracle_set_precise(1)
    try:
        b = cs.create(shape, bm.beagle.Beagle, library=oracle_lib)
        try:
            return [cs.execute(b, r, "oracle") for r in recs]
        finally:
            b.finalize()
    finally:
        if precise:
            oracle_lib.lib.oracle_set_precise(0)


@pytest.mark.parametrize("case", CASES[::5], ids=case_id)
def test_same_seed_same_records_and_json_round_trip(case, tmp_path):
    shape, seed = case
    a = records(shape, seed)
    assert cs.generate(shape, seed, length_for(seed)) == a
    assert cs.generate(shape, seed + 100, length_for(seed)) != a
    path = str(tmp_path / "sequence.json")
    cs.dump(path, shape, seed, a)
    assert cs.load(path) == (shape, seed, a)


def prelude_length(shape, seed):
    g = cs.Generator(shape, seed, length_for(seed))
    g.prelude()
    return g.prelude_end


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "S%d-C%d-T%d-P%d" % s)
def test_every_action_and_motif_is_there(shape):
    """Coverage is a condition: over a shape's seeds every action at least 3 times (counted behind the set-up calls), every motif in
    every sequence; a 4-state shape's seeds together hold every variant of motifs (d) and (f)."""
    count, variants = collections.Counter(), set()
    for seed in SEEDS[shape]:
        recs = records(shape, seed)
        tail = recs[prelude_length(shape, seed):]
        count.update(r["action"] for r in tail)
        assert set(r["motif"] for r in tail if r["motif"]) == set(cs.MOTIFS), seed
        variants |= set((r["motif"], r["variant"]) for r in tail if r["variant"])
        assert all(r["action"] in cs.ACTIONS for r in recs)
    short = {a: count[a] for a in cs.actions_for(shape[0]) if count[a] < 3}
    assert not short, short
    if shape[0] == 4:
        assert variants == set(("d", v) for v in cs.D_VARIANTS) | set(("f", v) for v in cs.F_VARIANTS)


def test_the_open_cases_of_the_contract_are_never_emitted():
    for shape, seed in CASES:
        assert 80 <= len(records(shape, seed)) - prelude_length(shape, seed) <= 120, (shape, seed)
        for r in records(shape, seed):
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
            elif m.startswith("updateTransitionMatrices"):
                assert a[-4] is None and a[-3] is None


_worst = collections.defaultdict(float)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_sequence_is_valid_and_well_conditioned_on_the_oracle(case, oracle_lib):
    shape, seed = case
    recs = records(shape, seed)
    plain = run_on_oracle(shape, recs, oracle_lib)
    precise = run_on_oracle(shape, recs, oracle_lib, precise=True)
    worst, reads = 0.0, 0
    for step, (rec, (rc, got), (rc_p, want)) in enumerate(zip(recs, plain, precise)):
        assert rc == 0 and rc_p == 0, (step, cs.describe(rec), rc, rc_p)
        for (kind, g), (_, w) in zip(got, want):
            assert np.isfinite(g).all() and np.isfinite(w).all(), (step, cs.describe(rec))
            d = cs.deviation(kind, g, w)
            assert d <= CONDITIONING_BOUND, (step, cs.describe(rec), kind, d)
            worst = max(worst, d)
            reads += 1
    assert reads >= 30
    _worst[shape] = max(_worst[shape], worst)
    print("shape %s seed %d: %d reads, |oracle - precise| at most %.2e (so far over the shape's seeds: %.2e)"
          % (shape, seed, reads, worst, _worst[shape]))
