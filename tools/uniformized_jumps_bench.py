#!/usr/bin/env python3
"""Sampled Markov-jump histories in one device call (beagleMi355SampleMarkovJumpsUniformized via beast-mcmc_amd/markovjumps.py)
against the integrated call (beagleMi355SampleMarkovJumps), the ancestral draw alone, and the host route the reference takes with
useUniformization = true (MarkovJumpsBeagleTreeLikelihood.java:473-509): the draw, a getTransitionMatrix per branch, then one
scalar history per (branch, site, simulant) on the host — here the numpy restatement (tests/uniformized_reference.py), timed on a
subset of patterns and extrapolated linearly (said so in the JSON).

GTR+G4, 1999 rows, the three registers of examples/TestXML/testUniformizedMarkovJumps.xml (all jumps; "upper" i < j; reward
[1 0 0 1]), at 1000 x 1e4 and 1000 x 1e5, with 1 and 100 simulants and with and without histories.  Every time is a whole call,
which ends in a synchronising copy, after a warm-up call; the median of several.  Prints one JSON line
(profiles/uniformized_jumps_bench.json).  ``--trace``: a few calls at each size, no host route, for a
``rocprofv3 --kernel-trace --stats`` run of its own."""
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np                                        # noqa: E402
import beast_mcmc_amd as bm                               # noqa: E402
import bench                                              # noqa: E402
import uniformized_reference as ur                        # noqa: E402
from beast_mcmc_amd.markovjumps import MarkovJumpsSampler                    # noqa: E402
from beast_mcmc_amd.treelikelihood import BeagleTreeLikelihood, RESCALE_DYNAMIC   # noqa: E402

HOST_PATTERNS = 200


def source_hash():
    h = hashlib.sha256()
    for f in ("kernels_uniformized.hip", "kernels_ancestral.hip", "ancestral_draw.h", "engine_sampling.cpp"):
        with open(os.path.join(ROOT, "beast-mcmc_amd", "csrc", f), "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


def median_ms(ts):
    return round(1e3 * float(np.median(ts)), 3)


def timed(f, reps):
    f(0)                                                  # warm-up: scratch allocation, code objects
    ts = []
    for k in range(reps):
        t0 = time.perf_counter()
        f(k + 1)
        ts.append(time.perf_counter() - t0)
    return ts


def measure(wl, reps, host_route=True):
    tl = BeagleTreeLikelihood(wl, rescaling=RESCALE_DYNAMIC, delay_rescaling=False)
    tl.getLogLikelihood()
    s = MarkovJumpsSampler(tl)
    S = wl.state_count
    s.add_register("all", np.ones((S, S)))
    s.add_register("upper", np.triu(np.ones((S, S)), 1))
    s.add_register("reward", [1.0, 0.0, 0.0, 1.0], kind="rewards")
    rows, order = s.ancestral.node_list()
    times, rates = s.branch_times(order)
    heights = s.node_heights(order)
    Q = s.infinitesimal_matrix()
    regs, flags, eig_idx = np.stack(s.registers), s.flags(), tl.eigen_index()

    def uni(seed, sims=1, history=False):
        return s.beagle.sampleMarkovJumpsUniformized(rows, times, rates, heights, Q, 0, 0, 0, regs, flags, seed, simulants=sims,
                                                     history=history, event_capacity=4 * len(rows) * wl.pattern_count // 10)

    out = {"taxa": wl.tip_count, "patterns": wl.pattern_count, "categories": wl.category_count, "rows": int(len(rows)),
           "registers": len(regs), "reps": reps}
    out["uniformized_1_simulant_ms"] = median_ms(timed(lambda k: uni(k), reps))
    out["uniformized_1_simulant_history_ms"] = median_ms(timed(lambda k: uni(k, history=True), reps))
    out["uniformized_100_simulants_ms"] = median_ms(timed(lambda k: uni(k, 100), max(2, reps // 2)))
    out["integrated_sampleMarkovJumps_ms"] = median_ms(timed(
        lambda k: s.beagle.sampleMarkovJumps(rows, times, rates, eig_idx, 0, 0, 0, regs, flags, k), reps))
    out["sampleAncestralStates_ms"] = median_ms(timed(lambda k: s.beagle.sampleAncestralStates(rows, 0, 0, k), reps))
    res = uni(7, history=True)
    out["events_per_call"] = res["event_total"]
    out["fallbacks"] = res["fallbacks"]
    if host_route:
        seed = 12345
        pats = np.arange(HOST_PATTERNS)
        t0 = time.perf_counter()
        st, ca = s.beagle.sampleAncestralStates(rows, 0, 0, seed)
        t1 = time.perf_counter()
        mats = np.zeros((len(rows), wl.category_count, S, S))
        for r in range(1, len(rows)):
            mats[r] = s.beagle.getTransitionMatrix(int(rows[r, 1])).reshape(wl.category_count, S, S)
        t2 = time.perf_counter()
        ref = ur.restate(rows[:, 2], times, rates, heights, st[:, pats], ca[pats], tl.cat_rates, mats, Q, s.registers, flags, 1,
                         seed, pattern_count=wl.pattern_count, patterns=pats)
        t3 = time.perf_counter()
        numpy_full = (t3 - t2) * wl.pattern_count / HOST_PATTERNS
        host = (t1 - t0) + (t2 - t1) + numpy_full
        dev = s.beagle.sampleMarkovJumpsUniformized(rows, times, rates, heights, Q, 0, 0, 0, regs, flags, seed)
        ok = ~ref["near"].any(axis=0)
        agree = bool(np.all(np.abs(dev["pattern_totals"][:, pats][:, ok] - ref["pattern_totals"][:, ok])
                            <= 1e-12 * np.maximum(np.abs(ref["pattern_totals"][:, ok]), 1.0)))
        out.update({"host_route_ms": round(1e3 * host, 1), "host_route_draw_ms": round(1e3 * (t1 - t0), 1),
                    "host_route_getTransitionMatrix_ms": round(1e3 * (t2 - t1), 1),
                    "host_route_numpy_ms_extrapolated": round(1e3 * numpy_full, 1),
                    "host_route_note": "numpy restatement timed on %d patterns and scaled linearly to %d" % (HOST_PATTERNS,
                                                                                                         wl.pattern_count),
                    "speedup_vs_host_route": round(host / (out["uniformized_1_simulant_ms"] / 1e3), 1),
                    "totals_agree_with_restatement_on_subset": agree})
    tl.close()
    return out


def main():
    cache = bench.workload_cache_file(bench.default_cache_dir(), "A", 1.0, "coalescent")
    a = bench.load_workload(cache, lambda: bm.synth.config_a(scale=1.0))
    if "--trace" in sys.argv:
        print(json.dumps({"A/10": measure(a.shard(0, 10000), reps=3, host_route=False), "A": measure(a, reps=2, host_route=False)}))
        return
    out = {"source_hash": source_hash(), "kernel_source_hash": bench.kernel_source_hash()}
    out["A/10"] = measure(a.shard(0, 10000), reps=7)
    out["A"] = measure(a, reps=3)
    t = out["A/10"]
    out["target_A/10_within_2x_of_integrated"] = t["uniformized_1_simulant_ms"] <= 2.0 * t["integrated_sampleMarkovJumps_ms"]
    out["target_A/10_10x_vs_host_route"] = t["speedup_vs_host_route"] >= 10.0
    print(json.dumps(out))


if __name__ == "__main__":
    main()
