"""The topology-chain generator and driver (tests/topology_chains.py) on the CPU tier.

  * A chain's records are reproducible and survive a JSON round trip.
  * Every chain of 60 proposals holds each move kind at least five times, at least a third topology moves, a rejected topology move, an
    accepted root change in both directions, and — measured on the driver — a closed operation list that is sent more than once, and
    under DYNAMIC a write-mode cycle inside the chain.
  * Every chain returns 0 with finite reads on the oracle.
  * Every chain is well conditioned — measured, not assumed: it also runs on the oracle's long-double mode (``oracle_set_precise``), and
    the largest difference between the two runs over all reads, normalised as the GPU comparison normalises them
    (``topology_chains.deviation``), stays at or below 1e-11: a tenth of the 1e-10 the engine is held to, as
    tests/test_call_sequences_host.py does it.
  * One negative control: the same chain with the restoreState of a rejected topology move left out moves a later lnL by more than
    1e4 x 1e-10 — the comparison sees a caller-side protocol error of exactly the kind these chains are about.

The configurations (tests/test_gpu_topology_chains.py runs the same ones on the engine).  Shapes are (states, categories, tips,
patterns[, kind]); "compressed": the alignments of tests/test_gpu_repeats.py (root_to_tip 0.15, 1 % unknown, all tips compact);
"shipped": a Yule tree of 400 tips, 20 proposals.  Schemes NONE and DYNAMIC everywhere, ALWAYS on the two first 4-state shapes and on the
four shapes of the other kernels; delay_rescaling off, rescaling frequency 7.

Measured maxima of |oracle - precise oracle| over a shape's seeds and schemes (the conditioning test prints them):

    shape                              largest deviation
    (4, 4, 12, 130)                    7.5e-13
    (4, 3, 9, 257)                     1.3e-13
    (4, 1, 24, 129, compressed)        7.3e-14
    (4, 4, 48, 1000, compressed)       6.9e-13
    (4, 4, 96, 300, compressed)        4.5e-13
    (4, 4, 400, 16385, shipped)        1.3e-12
    (20, 2, 8, 33)                     2.2e-13
    (61, 1, 6, 37)                     1.0e-12
    (7, 2, 8, 67)                      2.1e-13
    (80, 1, 6, 23)                     1.2e-13

They are a decade above those of tests/test_call_sequences_host.py because these chains hold branches down to
topology_chains.MIN_BRANCH = 0.004, whose transition matrices carry their absolute rounding error into cherries of two different states;
without that floor (the trees as drawn, heights from the middle 90 % of the whole interval) chains reached branches of 3e-5 and 1.3e-11.
(96, 300, 4) is drawn with workload seed 502 instead of the rule's (topology_chains.WORKLOAD_SEEDS says why).

The gradient chains (edge sums of derivatives behind every fourth proposal, every pre-order partial at the end; shapes (4, 4, 12, 130) and
(20, 2, 8, 33), unscaled, seeds 1 and 2): edge sums within 5.4e-14, pre-order partials within 8.1e-13 of the long-double mode.
"""
import collections
import json

import numpy as np
import pytest

import beast_mcmc_amd as bm
import topology_chains as tc

WALK4 = [(4, 4, 12, 130), (4, 3, 9, 257)]
COMPRESSED = [(4, 1, 24, 129, "compressed"), (4, 4, 48, 1000, "compressed"), (4, 4, 96, 300, "compressed")]
SHIPPED = (4, 4, 400, 16385, "shipped")
OTHER_KERNELS = [(20, 2, 8, 33), (61, 1, 6, 37), (7, 2, 8, 67), (80, 1, 6, 23)]      # T32 walk, T64 walk, general kernel, level kernels
SHAPES = WALK4 + COMPRESSED + [SHIPPED] + OTHER_KERNELS
SEEDS = {shape: [1, 2, 3, 4] if shape in WALK4 else [1, 2] for shape in SHAPES}
SCHEMES = {shape: [tc.SCHEME_NONE, tc.SCHEME_DYNAMIC] + ([tc.SCHEME_ALWAYS] if shape in WALK4 + OTHER_KERNELS else []) for shape in SHAPES}
CASES = [(shape, seed, scheme) for shape in SHAPES for seed in SEEDS[shape] for scheme in SCHEMES[shape]]
CONDITIONING_BOUND = 1e-11


def steps_for(shape):
    return 20 if shape == SHIPPED else 60


def node_stride(shape):
    return 5 if shape == SHIPPED else 1                      # (the shipped shape: every fifth node)


def case_id(c):
    return "%s-seed%d-%s" % (tc.shape_id(c[0]), c[1], tc.SCHEME_NAMES[c[2]])


_records = {}


def records(shape, seed, scheme, checkpoints=True):
    key = (shape, seed, scheme, checkpoints)
    if key not in _records:
        _records[key] = tc.generate(shape, seed, steps_for(shape), scheme, checkpoints=checkpoints and shape != SHIPPED)
    return _records[key]


GRADIENT_SHAPES = [(4, 4, 12, 130), (20, 2, 8, 33)]              # gradients behind topology moves: unscaled chains, seeds 1 and 2


def run_on_oracle(shape, scheme, recs, oracle_lib, precise=False, skip_restore_at=None, gradients=False):
    """-> ([(return code, reads)] for the evaluation before the chain and every record, the driver)"""
    if precise:
        oracle_lib.lib.oracle_set_precise(1)
    try:
        b = tc.create(shape, bm.beagle.Beagle, library=oracle_lib, gradients=gradients)
        try:
            d = tc.Driver(b, shape, scheme)
            out = [tc.run_step(d, None, first=True)]
            for k, rec in enumerate(recs):
                out.append(tc.run_step(d, rec, skip_restore=(k == skip_restore_at), node_stride=node_stride(shape), gradients=gradients))
            return out, d
        finally:
            b.finalize()
    finally:
        if precise:
            oracle_lib.lib.oracle_set_precise(0)


@pytest.mark.parametrize("shape", SHAPES, ids=tc.shape_id)
def test_records_are_reproducible_and_json_stable(shape, tmp_path):
    for seed in SEEDS[shape]:
        recs = tc.generate(shape, seed, steps_for(shape), tc.SCHEME_DYNAMIC)
        assert recs == tc.generate(shape, seed, steps_for(shape), tc.SCHEME_DYNAMIC)
        assert json.loads(json.dumps(recs)) == recs
        path = str(tmp_path / "chain.json")
        tc.dump(path, shape, seed, tc.SCHEME_DYNAMIC, recs)
        assert tc.load(path) == (shape, seed, tc.SCHEME_DYNAMIC, recs)
        # the scheme changes which evaluations rescale and nothing else; the variant without checkpoints only drops reads
        strip = lambda rs, key: [{k: v for k, v in r.items() if k != key} for r in rs]
        assert strip(tc.generate(shape, seed, steps_for(shape), tc.SCHEME_NONE), "write") == strip(recs, "write")
        assert strip(tc.generate(shape, seed, steps_for(shape), tc.SCHEME_DYNAMIC, checkpoints=False), "reads") == strip(recs, "reads")


@pytest.mark.parametrize("shape", SHAPES, ids=tc.shape_id)
def test_every_chain_holds_what_it_is_for(shape):
    for seed in SEEDS[shape]:
        recs = records(shape, seed, tc.SCHEME_DYNAMIC)
        c = tc.census(recs, shape)
        print("%s seed %d: %s" % (tc.shape_id(shape), seed, c))
        assert len(recs) == steps_for(shape)
        assert 3 * c["topology"] >= len(recs), c
        assert c["rejected_topology"] >= 1 and c["root_to_parent"] >= 1 and c["root_to_sibling"] >= 1 and c["write"] >= 1, c
        if shape != SHIPPED:
            assert all(c[k] >= 5 for k in tc.MOVES), c
        assert sum("nodes" in r["reads"] for r in recs) == (1 if shape == SHIPPED else 3) and "nodes" in recs[-1]["reads"]
        assert sum("nodes" in r["reads"] for r in records(shape, seed, tc.SCHEME_DYNAMIC, checkpoints=False)) == 1


_worst = collections.defaultdict(float)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_chains_run_on_the_oracle_and_are_well_conditioned(case, oracle_lib):
    shape, seed, scheme = case
    recs = records(shape, seed, scheme)
    plain, driver = run_on_oracle(shape, scheme, recs, oracle_lib)
    precise, _ = run_on_oracle(shape, scheme, recs, oracle_lib, precise=True)
    worst = 0.0
    for step, ((rc, reads), (rc_p, reads_p)) in enumerate(zip(plain, precise)):
        assert rc == 0 and rc_p == 0, (step, rc, rc_p)
        assert len(reads) == len(reads_p) >= 1
        for (kind, a), (_, b) in zip(reads, reads_p):
            assert np.isfinite(a).all(), (step, kind)
            d = tc.deviation(kind, a, b)
            assert d <= CONDITIONING_BOUND, (step, kind, d)
            worst = max(worst, d)
    _worst[shape] = max(_worst[shape], worst)
    print("%s: largest |oracle - precise oracle| %.1e (over the shape so far %.1e); %d evaluations, %d in write mode, the most frequent "
          "closed list sent %d times" % (case_id(case), worst, _worst[shape], driver.evaluations, driver.write_evaluations,
                                         max(driver.closed_lists.values())))
    assert max(driver.closed_lists.values()) >= 2, "no closed list came twice"
    assert driver.evaluations == len(recs) + 1
    if scheme == tc.SCHEME_DYNAMIC:
        assert driver.write_evaluations >= 2                  # (the one before the chain, and a cycle inside it)
    assert driver.write_evaluations == (scheme != tc.SCHEME_NONE) + sum(bool(r["write"]) for r in recs)


@pytest.mark.parametrize("shape", GRADIENT_SHAPES, ids=tc.shape_id)
def test_gradient_chains_run_on_the_oracle_and_are_well_conditioned(shape, oracle_lib):
    """The same chains with the edge sums of derivatives behind every fourth proposal and every pre-order partial at the end: finite,
    within 1e-11 of the long-double mode, and taken on more than one set of cherries (a topology move changes which nodes the engine
    leaves unstored in a gradient chain)."""
    for seed in (1, 2):
        recs = records(shape, seed, tc.SCHEME_NONE)
        plain, driver = run_on_oracle(shape, tc.SCHEME_NONE, recs, oracle_lib, gradients=True)
        precise, _ = run_on_oracle(shape, tc.SCHEME_NONE, recs, oracle_lib, precise=True, gradients=True)
        worst = collections.defaultdict(float)
        for (rc, reads), (rc_p, reads_p) in zip(plain, precise):
            assert rc == 0 and rc_p == 0 and len(reads) == len(reads_p)
            for (kind, a), (_, b) in zip(reads, reads_p):
                d = tc.deviation(kind, a, b)
                assert np.isfinite(a).all() and d <= CONDITIONING_BOUND, (kind, d)
                worst[kind] = max(worst[kind], d)
        derivs = sum(kind == "deriv" for _, reads in plain for kind, _ in reads)
        print("%s seed %d, gradients: %d edge-sum reads on %d sets of cherries; largest |oracle - precise oracle| %s"
              % (tc.shape_id(shape), seed, derivs, len(driver.cherry_sets), ", ".join("%s %.1e" % kv for kv in sorted(worst.items()))))
        assert derivs == len(recs) // 4 + (len(recs) % 4 != 0) and len(driver.cherry_sets) >= 2


def test_a_left_out_restore_is_seen(oracle_lib):
    """The negative control: shape (4, 4, 12, 130), seed 1, DYNAMIC — the first rejected topology move's restoreState is left out
    (topology and heights go back, the buffer indices do not): a later lnL moves by more than 1e4 x 1e-10 relative."""
    shape, seed, scheme = WALK4[0], 1, tc.SCHEME_DYNAMIC
    recs = records(shape, seed, scheme)
    at = next(k for k, r in enumerate(recs) if r["move"] in tc.TOPOLOGY_MOVES and not r["accept"])
    good, _ = run_on_oracle(shape, scheme, recs, oracle_lib)
    bad, _ = run_on_oracle(shape, scheme, recs, oracle_lib, skip_restore_at=at)
    for k in range(at + 2):                                   # (up to and including the rejected proposal itself nothing differs)
        assert tc.deviation("sum", bad[k][1][0][1], good[k][1][0][1]) == 0.0
    later = [tc.deviation("sum", b[1][0][1], g[1][0][1]) for b, g in zip(bad[at + 2:], good[at + 2:]) if b[0] == 0 and len(b[1])]
    later = [d for d in later if d == d]
    print("restoreState left out at step %d (%s): largest later lnL deviation %.3e" % (at, tc.describe(recs[at]), max(later)))
    assert max(later) > 1e4 * tc.BOUND
