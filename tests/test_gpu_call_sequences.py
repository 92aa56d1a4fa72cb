"""Seeded random call sequences (tests/call_sequences.py) on the engine and the CPU oracle in lockstep.

Almost every call into the engine is deferred or cached somewhere (uploads that ride in the next launch, a one-launch walk held back
until the next call, a pre-order list held back until something reads or writes its buffers, plans replayed from a cache, virtual
buffers, site values fetched ahead); every such mechanism has a scripted test that walks the order its author thought of.  Here the
orders are generated: per (shape, seed) three instances execute the same records call by call —

  * the engine on its defaults,
  * a twin created under BEAGLE_MI355_COPY_ENGINE_UPLOADS=1 and BEAGLE_MI355_NO_PLAN_CACHE=1, the two switches whose row in
    tests/test_gpu_switches.py SWITCHES promises the same bits,
  * the CPU oracle —

and AT EVERY CALL the three return codes are equal, every read of the default engine equals the twin's bit for bit, and is within the
project's bounds of the oracle's (call_sequences.deviation: 1e-10 relative for sums, site values and log scale factors; node partials
and pre-order partials within 1e-10 of each pattern's largest entry as test_gpu_parity.test_engine_matches_oracle normalises them, a
transition matrix likewise against its largest entry; derivative outputs as test_gpu_gradients.test_gradient_matches_oracle's
``close``).  tests/test_call_sequences_host.py measures that the oracle itself is within 1e-11 of its long-double mode on every read of
every sequence used here.

A mismatch names shape, seed, step and call, leaves the records in the test's tmp_path and gives the replay line.

Route evidence (counters read at the end of each sequence, summed over a shape's seeds): on 4 states a root call answered inside the
walk's launch, site values found prefetched, ticket walks, slice accumulations, pre-order lists answered held (fused or walked) and a
held list forced to run by a later call; on 20 and 61 states the pattern walks.  NOT reached at these sizes: the class tables of
repeated sub-patterns (repeatStats; the engine leaves them off below 64 KiB partials buffers) — tests/test_gpu_repeats.py holds them
under BEAGLE_MI355_REPEATS_ANY_SIZE=1.

One more parametrisation runs shape (4, 4, 12, 130) on the pattern-sharded handle (three shards on one GPU, as
tests/test_gpu_sharded_instance.py creates it) against the oracle only; a read the handle answers with NO_IMPLEMENTATION is dropped.

The generator's second profile, "extensions", puts the one-call entry points into the generated orders — sampleAncestralStates,
sampleMarkovJumps, simulateSequences, nodeHeightDerivatives, updateDifferentialMatrices, setReversibleModels, getEigenDecomposition
— with motifs (j)-(m) around the decisions each of them makes about the deferred state (tests/call_sequences.py).  The same three
instances, the same three conditions at every call, on the five shapes of at most 64 states, and two seeds on the sharded handle
(NO_IMPLEMENTATION tolerated on calls that return values and change nothing).  What is compared: node-height derivatives and
Markov-jump values as derivative outputs are (the jump values restated on the oracle's side for the DEVICE's states and categories);
an eigen system through U diag(lambda) U^-1 against the oracle side's Q, relative to max |Q|, and U U^-1 against I; the states and
categories of every draw twice — byte for byte against the restatement over what the same instance reads back right after the call
(read "exact"), and against the restatement over the oracle's reads on every decided pattern, with at most 1 % of a sequence's
(sampler call, pattern) pairs undecided.  Route evidence over a 4-state shape's seeds: a held pre-order list both run late and
answered while held, models decomposed on the device, a folded tip demoted by a sampler, one-launch walks.

The third profile, "queries", does the same for the five entry points merged since — updateTransitionMatricesFromGenerators,
updateTransitionMatricesWithEpochs, nodePosteriors, nodePatternLikelihoods, placementScores — with motifs (n)-(r): the same shapes
and seeds, the same three instances and conditions, two seeds on the sharded handle (where placementScores answers NO_IMPLEMENTATION
before it changes anything and is left out; the four others run).  What is compared: the matrices the two matrix calls wrote through
every later read; posteriors, category posteriors, MAP probabilities and state totals (over the sum of the pattern weights) by their
absolute difference; MAP states on every decided pattern; log pattern values, node terms, log tables and scores against max(1,
|value|), the node-pattern sum as a log-likelihood; and the device's posteriors byte for byte against
node_posteriors_reference.posteriors over what the same instance reads back (read "exact").  Route evidence over a 4-state shape's
seeds: a held list both run late and answered while held, buffers materialised by each of nodePosteriors, placementScores and
nodePatternLikelihoods, generator and epoch calls, a demoted folded tip, models decomposed on the device — every one of these counters
is reached at these sizes.

Every sequence prints its wall time.  Measured on an MI355X, in one run, per sequence (200 .. 226 calls, three instances): extensions
0.06 .. 0.16 s (0.35 s for the first of the process), queries 0.04 .. 0.17 s — the 61-state shape is the slowest of both, 0.16 / 0.17 s.
"""
import collections
import os
import time

import numpy as np
import pytest

import beast_mcmc_amd as bm
import call_sequences as cs
from test_call_sequences_host import CASES, CASES_EXT, CASES_Q, SEEDS, SEEDS_EXT, SHAPES, SHAPES_EXT, case_id, records

pytestmark = pytest.mark.gpu

TWIN_ENV = {"BEAGLE_MI355_COPY_ENGINE_UPLOADS": "1", "BEAGLE_MI355_NO_PLAN_CACHE": "1"}
READ_ONLY = ("getTransitionMatrix", "getLogScaleFactors", "getSiteLogLikelihoods", "getPartials", "getPartialsBatch",
             "calculateEdgeDifferentials", "calculateCrossProductDifferentials")
RETURNS_VALUES = ("sampleAncestralStates", "sampleMarkovJumps", "simulateSequences", "nodeHeightDerivatives", "getEigenDecomposition",
                  "nodePosteriors", "nodePatternLikelihoods", "placementScores")
NO_IMPLEMENTATION = -7


def created_under(env, make):
    """make() with the BEAGLE_MI355_* switches `env` in force (the engine reads them when an instance is created)"""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return make()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def fail(what, shape, seed, step, recs, tmp_path, profile="base"):
    path = str(tmp_path / ("sequence_S%d_C%d_T%d_P%d_seed%d.json" % (shape + (seed,))))
    cs.dump(path, shape, seed, recs, profile)
    raise AssertionError("shape %s seed %d step %d %s: %s\nreplay: python tests/call_sequences.py --replay %s --upto %d"
                         % (shape, seed, step, cs.describe(recs[step]), what, path, step))


def counters(b, queries=False):
    """`queries`: what the stats getters of the query profile's five calls report as well (not on the sharded handle)"""
    info, grad = b.walkLaunchInfo(), b.gradientStats()
    out = {"rootFusedCount": b.rootFusedCount(), "sitePrefetchCount": b.sitePrefetchCount(), "ticket_walks": info["ticket_walks"],
           "slice_accumulations": info["slice_accumulations"], "held_answered": grad["fused"] + grad["walked"], "late": grad["late"],
           "walks": b.walkStats()["walks"], "eigen_calls": b.eigenStats()["calls"], "demotions": b.tipEmissionStats()["demotions"]}
    if queries:
        out.update({"generator_calls": b.generatorStats()["calls"], "epoch_calls": b.epochStats()["calls"],
                    "posteriors_materialised": b.nodePosteriorStats()["materialised"], "placement_materialised": b.placementStats()["materialised"],
                    "nodepattern_materialised": b.nodePatternStats()["materialised"]})
    return out


def lockstep(shape, seed, oracle_lib, tmp_path, sharded=False, profile="base"):
    """-> the default engine's counters at the end of the sequence"""
    recs = records(shape, seed, profile)
    instances = []
    started = time.perf_counter()
    try:
        if sharded:
            g = len(bm.beagle.engine().resource_list()) - 2
            eng = created_under({"BEAGLE_MI355_SHARDS": "3"}, lambda: cs.create(shape, bm.beagle.Beagle, resourceList=(g + 1,)))
            instances.append(eng)
            twin = None
        else:
            eng = cs.create(shape, bm.beagle.Beagle)
            instances.append(eng)
            twin = created_under(TWIN_ENV, lambda: cs.create(shape, bm.beagle.Beagle))
            instances.append(twin)
        ora = cs.create(shape, bm.beagle.Beagle, library=oracle_lib)
        instances.append(ora)
        worst = collections.defaultdict(float)
        pairs = undecided = 0
        for step, rec in enumerate(recs):
            rc_e, got = cs.execute(eng, rec, "engine")
            if sharded and rc_e == NO_IMPLEMENTATION:
                # (only a call that returns values and changes nothing can be left out without the two sides parting)
                assert rec["m"] in READ_ONLY + RETURNS_VALUES, (step, cs.describe(rec))
                continue
            info = {"device": got}
            rc_o, want = cs.execute(ora, rec, "oracle", info)
            if "undecided" in info:
                pairs += info["undecided"].size
                undecided += int(info["undecided"].sum())
            if twin is not None:
                rc_t, same = cs.execute(twin, rec, "engine")
                if not (rc_e == rc_t == rc_o):
                    fail("return codes engine %d, twin %d, oracle %d" % (rc_e, rc_t, rc_o), shape, seed, step, recs, tmp_path, profile)
                for k, ((kind, a), (_, b)) in enumerate(zip(got, same)):
                    if not np.array_equal(a, b):
                        fail("read %d (%s): the default engine and its twin (%s) differ, by at most %.3e"
                             % (k, kind, " ".join(sorted(TWIN_ENV)), float(np.max(np.abs(a.astype(float) - b.astype(float))))),
                             shape, seed, step, recs, tmp_path, profile)
            elif rc_e != rc_o:
                fail("return codes sharded engine %d, oracle %d" % (rc_e, rc_o), shape, seed, step, recs, tmp_path, profile)
            if len(got) != len(want):
                fail("%d reads on the engine, %d on the oracle" % (len(got), len(want)), shape, seed, step, recs, tmp_path, profile)
            for k, ((kind, a), (_, b)) in enumerate(zip(got, want)):
                d = cs.deviation(kind, a, b, undecided=info.get("undecided"))
                worst[kind] = max(worst[kind], d) if d == d else d
                if not d <= cs.BOUND:
                    fail("read %d (%s): engine against oracle %.3e, bound %.0e" % (k, kind, d, cs.BOUND), shape, seed, step, recs, tmp_path, profile)
        print("shape %s seed %d%s%s: %d calls in %.2f s; largest deviation from the oracle by kind of read: %s%s"
              % (shape, seed, ", sharded" if sharded else "", "" if profile == "base" else ", " + profile, len(recs),
                 time.perf_counter() - started, ", ".join("%s %.1e" % kv for kv in sorted(worst.items())),
                 "; %d of %d (sampler call, pattern) pairs undecided" % (undecided, pairs) if pairs else ""))
        if undecided > cs.UNDECIDED_CAP * pairs:
            fail("%d of %d (sampler call, pattern) pairs undecided" % (undecided, pairs), shape, seed, len(recs) - 1, recs, tmp_path, profile)
        return counters(eng, queries=(profile == "queries" and not sharded))
    finally:
        for b in instances:
            b.finalize()


_counters = {}


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_engine_twin_and_oracle_in_lockstep(case, oracle_lib, tmp_path):
    shape, seed = case
    _counters[case] = None                                   # (failed, unless the next line returns: not run a second time below)
    _counters[case] = lockstep(shape, seed, oracle_lib, tmp_path)


@pytest.mark.parametrize("shape", [s for s in SHAPES if s[0] in (4, 20, 61)], ids=lambda s: "S%d-C%d-T%d-P%d" % s)
def test_the_sequences_take_the_deferred_routes(shape, oracle_lib, tmp_path):
    """The sequences must not all fall back to a general path: the counters of the branches this module exists for, summed over the
    shape's seeds (a sequence that the test above has not run is run here; one that failed there counts nothing)."""
    total = collections.Counter()
    for seed in SEEDS[shape]:
        if (shape, seed) not in _counters:
            _counters[(shape, seed)] = lockstep(shape, seed, oracle_lib, tmp_path)
        total.update(_counters[(shape, seed)] or {})
    print("shape %s: %s" % (shape, dict(total)))
    if shape[0] == 4:
        for key in ("rootFusedCount", "sitePrefetchCount", "ticket_walks", "slice_accumulations", "held_answered", "late"):
            assert total[key] > 0, (key, dict(total))
    else:
        assert total["walks"] > 0, dict(total)


@pytest.mark.parametrize("seed", [1, 2])
def test_sharded_handle_and_oracle_in_lockstep(seed, oracle_lib, tmp_path):
    lockstep((4, 4, 12, 130), seed, oracle_lib, tmp_path, sharded=True)


# ---- profile "extensions": the one-call entry points in the generated orders ------------------------------------------------------
_counters_ext = {}


@pytest.mark.parametrize("case", CASES_EXT, ids=case_id)
def test_extension_calls_engine_twin_and_oracle_in_lockstep(case, oracle_lib, tmp_path):
    shape, seed = case
    _counters_ext[case] = None
    _counters_ext[case] = lockstep(shape, seed, oracle_lib, tmp_path, profile="extensions")


@pytest.mark.parametrize("shape", [s for s in SHAPES_EXT if s[0] == 4], ids=lambda s: "S%d-C%d-T%d-P%d" % s)
def test_the_extension_sequences_reach_the_deferral_decisions(shape, oracle_lib, tmp_path):
    """Summed over a 4-state shape's seeds: a held pre-order list was both run by a later call and answered while held around the
    new calls, models were decomposed on the device, a sampler demoted a folded tip, and one-launch walks ran."""
    total = collections.Counter()
    for seed in SEEDS_EXT[shape]:
        if (shape, seed) not in _counters_ext:
            _counters_ext[(shape, seed)] = lockstep(shape, seed, oracle_lib, tmp_path, profile="extensions")
        total.update(_counters_ext[(shape, seed)] or {})
    print("shape %s, extensions: %s" % (shape, dict(total)))
    for key in ("late", "held_answered", "eigen_calls", "demotions", "walks"):
        assert total[key] > 0, (key, dict(total))


@pytest.mark.parametrize("seed", [1, 2])
def test_extension_calls_sharded_handle_and_oracle_in_lockstep(seed, oracle_lib, tmp_path):
    lockstep((4, 4, 12, 130), seed, oracle_lib, tmp_path, sharded=True, profile="extensions")


# ---- profile "queries": the five entry points merged after the extension profile, in the generated orders -------------------------
_counters_q = {}


@pytest.mark.parametrize("case", CASES_Q, ids=case_id)
def test_query_calls_engine_twin_and_oracle_in_lockstep(case, oracle_lib, tmp_path):
    shape, seed = case
    _counters_q[case] = None
    _counters_q[case] = lockstep(shape, seed, oracle_lib, tmp_path, profile="queries")


@pytest.mark.parametrize("shape", [s for s in SHAPES_EXT if s[0] == 4], ids=lambda s: "S%d-C%d-T%d-P%d" % s)
def test_the_query_sequences_reach_the_deferral_decisions(shape, oracle_lib, tmp_path):
    """Summed over a 4-state shape's seeds: a held pre-order list was both run by a later call and answered while held around the
    new calls; nodePosteriors, placementScores and nodePatternLikelihoods each materialised buffers that the walk had left unstored;
    the generator call and the epoch call ran; a folded tip was demoted; models were decomposed on the device."""
    total = collections.Counter()
    for seed in SEEDS_EXT[shape]:
        if (shape, seed) not in _counters_q:
            _counters_q[(shape, seed)] = lockstep(shape, seed, oracle_lib, tmp_path, profile="queries")
        total.update(_counters_q[(shape, seed)] or {})
    print("shape %s, queries: %s" % (shape, dict(total)))
    for key in ("late", "held_answered", "posteriors_materialised", "placement_materialised", "nodepattern_materialised", "generator_calls",
                "epoch_calls", "demotions", "eigen_calls"):
        assert total[key] > 0, (key, dict(total))


@pytest.mark.parametrize("seed", [1, 2])
def test_query_calls_sharded_handle_and_oracle_in_lockstep(seed, oracle_lib, tmp_path):
    """placementScores answers NO_IMPLEMENTATION on the sharded handle before it changes anything and is left out; the four others run."""
    lockstep((4, 4, 12, 130), seed, oracle_lib, tmp_path, sharded=True, profile="queries")
