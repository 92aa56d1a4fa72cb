"""CPU tier of beagleBastaSampleStates: the host restatement of the draw (tests/basta_states_reference.py) on the vectors of the host
restatement of the likelihood (tests/basta_reference.py), for a 5-tip and a 51-tip tree sampled through time."""
import re

import numpy as np
import pytest

import ancestral_reference as ar
import basta_reference as ref
import basta_states_cases as cases
import basta_states_reference as sr
import beast_mcmc_amd as bm
import helpers

_made = {}


def fixture(state_count, tip_count, **kw):
    """(inputs, vectors [buffer][S]) — evaluated once per distinct case and left unchanged"""
    key = (state_count, tip_count, tuple(sorted(kw.items())))
    if key not in _made:
        x = cases.Inputs(state_count, tip_count, seed=state_count + tip_count, **kw)
        tr = x.traversal
        _, vectors, _ = ref.evaluate(x.tips, tr.operations, tr.intervals, tr.lengths, x.matrices, x.sizes, tr.buffer_count, tr.interval_count)
        vectors.setflags(write=False)
        _made[key] = (x, vectors)
    return _made[key]


def draw(x, vectors, replicates, seed, **kw):
    tr = x.traversal
    return sr.sample(tr.operations, tr.intervals, vectors, lambda m: x.matrices[m], x.frequencies, replicates, seed, **kw)


def test_the_header_declares_and_the_veneer_binds_the_call():
    hdr = open(helpers.ROOT + "/include/beagle_mi355.h").read()
    assert re.search(r"\bint\s+beagleBastaSampleStates\s*\(", hdr)
    assert re.search(r"#define\s+BEAGLE_MI355_BASTA_STATES_AS_WRITTEN\s+2\b", hdr)
    assert "beagleBastaSampleStates" in bm.beagle.ABI_SYMBOLS and "beagleBastaStatesStats" in bm.beagle.ABI_SYMBOLS
    assert hasattr(bm.beagle.Beagle, "sampleBastaStates") and hasattr(bm.basta.BastaLikelihood, "sample_states")
    assert bm.beagle.Beagle.BASTA_STATES_AS_WRITTEN == sr.AS_WRITTEN


def test_the_random_numbers_are_the_samplers_stream():
    for seed, r, b in ((0, 0, 0), (12345, 7, 99), (2 ** 64 - 1, 3, 2 ** 31)):
        stream = int(ar.splitmix64(seed, r))
        want = float(int(ar.splitmix64(stream, b)) >> 11) * 2.0 ** -53
        assert sr.uniforms(seed, np.array([r], dtype=np.uint64), b)[0] == want


@pytest.mark.parametrize("state_count,tip_count,tips", [(3, 5, "ambiguous"), (7, 51, "ambiguous"), (4, 51, "one-hot")])
def test_default_weights_are_the_exact_conditional(state_count, tip_count, tips):
    """For every operation and every dest state s the default weights add up, in index order, to left_s / right_s as the likelihood
    restatement formed them (stored in dest of a one-input operation, in acc1 / acc2 of a coalescence): within S 2^-52 relative."""
    x, vectors = fixture(state_count, tip_count, tips=tips)
    s_all = np.arange(state_count)
    worst = 0.0
    for op in x.traversal.operations:
        for inp, m, stored in ((op[1], op[2], op[5] if op[3] >= 0 else op[0]), (op[3], op[4], op[6])):
            if inp < 0:
                continue
            w = sr.weights(x.matrices[int(m)], s_all, vectors[inp], False)
            total = np.zeros(state_count)
            for j in range(state_count):
                total = total + w[:, j]
            want = vectors[stored]
            assert np.all(np.abs(total - want) <= state_count * 2.0 ** -52 * want)
            worst = max(worst, float(np.max(np.abs(total - want) / np.where(want > 0, want, 1.0))))
    print("S=%d T=%d: worst relative difference %.3e" % (state_count, tip_count, worst))


@pytest.mark.parametrize("state_count,tip_count", [(3, 5), (4, 51)])
def test_fixed_tips_give_their_deme_for_every_seed(state_count, tip_count):
    x, vectors = fixture(state_count, tip_count, tips="one-hot")
    for seed in (0, 1, 977):
        for kw in ({}, {"as_written": True}, {"use_map": True}):
            states, _, _, bad = draw(x, vectors, 4, seed, **kw)
            assert not bad
            assert np.array_equal(states[:, :tip_count], np.broadcast_to(x.demes.astype(np.uint8), (4, tip_count)))


def test_every_vector_of_the_list_gets_a_state_and_no_other():
    x, vectors = fixture(4, 51, tips="ambiguous")
    ops = x.traversal.operations
    states, _, _, _ = draw(x, vectors, 3, 5)
    touched = np.zeros(vectors.shape[0], dtype=bool)
    touched[ops[:, 0]] = True
    touched[ops[:, 1]] = True
    two = ops[:, 3] >= 0
    for col in (3, 5, 6):
        touched[ops[two, col]] = True
    assert np.all(states[:, touched] < 4) and np.all(states[:, ~touched] == 255)
    assert np.array_equal(states[:, ops[two, 5]], states[:, ops[two, 1]]) and np.array_equal(states[:, ops[two, 6]], states[:, ops[two, 3]])


@pytest.mark.parametrize("tip_count", [5, 51])
def test_the_orientation_flag_matters_only_for_an_asymmetric_q(tip_count):
    x, vectors = fixture(4, tip_count, tips="ambiguous", symmetric=True)
    assert all(np.array_equal(m, m.T) for m in x.matrices.values())
    assert np.array_equal(draw(x, vectors, 64, 3)[0], draw(x, vectors, 64, 3, as_written=True)[0])
    y, vectors_y = fixture(4, tip_count, tips="ambiguous")
    assert not np.array_equal(draw(y, vectors_y, 64, 3)[0], draw(y, vectors_y, 64, 3, as_written=True)[0])


@pytest.mark.parametrize("tip_count", [5, 51])
def test_map_does_not_depend_on_the_seed_or_the_replicate(tip_count):
    x, vectors = fixture(4, tip_count, tips="ambiguous")
    a = draw(x, vectors, 3, 1, use_map=True)[0]
    b = draw(x, vectors, 3, 2, use_map=True)[0]
    assert np.array_equal(a, b) and np.array_equal(a[0], a[1]) and np.array_equal(a[0], a[2])
    assert not np.array_equal(draw(x, vectors, 3, 1)[0], draw(x, vectors, 3, 2)[0])


def test_replicates_do_not_depend_on_how_the_call_is_cut():
    x, vectors = fixture(4, 51, tips="ambiguous")
    whole = draw(x, vectors, 130, 9)[0]
    assert np.array_equal(whole[64:], draw(x, vectors, 66, 9, first_replicate=64)[0])


def test_root_state_frequencies():
    """5 tips, 2 demes, 65 536 replicates: each root state's frequency within 5 binomial standard deviations of p_i f_i / sum."""
    x, vectors = fixture(2, 5, tips="ambiguous")
    replicates = 65536
    states, _, _, bad = draw(x, vectors, replicates, 20260101)
    assert not bad
    root = int(x.traversal.operations[-1, 0])
    w = vectors[root] * x.frequencies
    p = w / w.sum()
    got = np.bincount(states[:, root], minlength=2) / replicates
    sd = np.sqrt(p * (1.0 - p) / replicates)
    print("root state frequencies %s, expected %s, deviations in sd %s" % (got, p, (got - p) / sd))
    assert np.all(np.abs(got - p) <= 5.0 * sd)


@pytest.mark.parametrize("state_count,tip_count", [(3, 5), (4, 51)])
def test_count_arrays_are_the_counts_of_the_states(state_count, tip_count):
    x, vectors = fixture(state_count, tip_count, tips="ambiguous")
    tr = x.traversal
    states, occupancy, changes, _ = draw(x, vectors, 37, 4)
    want_occupancy, want_changes = sr.counts_from_states(tr.operations, tr.intervals, states, state_count)
    assert np.array_equal(occupancy, want_occupancy) and np.array_equal(changes, want_changes)
    inputs = (tr.operations[:, 1] >= 0).sum() + (tr.operations[:, 3] >= 0).sum()
    assert occupancy.sum() == changes.sum() == 37 * inputs
    assert np.array_equal(occupancy.sum(axis=0), changes.sum(axis=0))


def test_a_zero_vector_is_flagged_and_gets_state_zero():
    x, vectors = fixture(3, 5, tips="ambiguous")
    broken = vectors.copy()
    broken[1] = 0.0
    good = draw(x, vectors, 5, 8)[0]
    states, _, _, bad = draw(x, broken, 5, 8)
    assert bad and np.all(states[:, 1] == 0)
    others = np.arange(vectors.shape[0]) != 1
    acc = [int(op[5 if op[1] == 1 else 6]) for op in x.traversal.operations if op[3] >= 0 and 1 in (op[1], op[3])]
    others[acc] = False
    assert np.array_equal(states[:, others], good[:, others])


def test_launch_depth_of_a_ladder_and_of_a_list_without_a_coalescence_at_the_top():
    ladder = cases.Inputs(2, 12, kind="ladder")
    assert sr.coalescence_depth(ladder.traversal.operations) == 11
    assert sr.coalescence_depth([[2, 0, 0, -1, -1, 2, -1, 0], [3, 2, 1, 1, 1, 4, 5, 1]]) == 1
    assert sr.coalescence_depth([[3, 0, 0, 1, 0, 4, 5, 0], [6, 3, 1, -1, -1, 6, -1, 1]]) == 2
