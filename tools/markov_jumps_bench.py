#!/usr/bin/env python3
"""Markov jumps in one device call (beagleMi355SampleMarkovJumps via beast-mcmc_amd/markovjumps.py) against the way
MarkovJumpsBeagleTreeLikelihood gets them through the BEAGLE interface (src/dr/evomodel/treelikelihood/
MarkovJumpsBeagleTreeLikelihood.java:429-567): the ancestral draw, a getTransitionMatrix per branch, then the Minin-Suchard algebra
and the per-site lookup on the host (numpy: tests/markov_jumps_reference.py, the restatement the GPU tests compare against — so
this run also checks the device's totals against it).

GTR+G4, 1999 rows, three registers (all counts; one from->to count scaled by time; a reward scaled by time), at A/10 (1000 taxa x
10 000 patterns) and A (1000 x 1e5).  Every time is a whole call, which ends in a synchronising copy, after a warm-up call; the
median of several.  Prints one JSON line (profiles/markov_jumps_bench.json).  ``--trace``: a few calls at each size, no host route, for a
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
import markov_jumps_reference as mr                       # noqa: E402
from beast_mcmc_amd.markovjumps import MarkovJumpsSampler                    # noqa: E402
from beast_mcmc_amd.treelikelihood import BeagleTreeLikelihood, RESCALE_DYNAMIC   # noqa: E402


def source_hash():
    h = hashlib.sha256()
    for f in ("kernels_markovjumps.hip", "kernels_ancestral.hip", "engine_sampling.cpp"):
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
    s.add_register("jump", np.ones((S, S)))
    one = np.zeros((S, S)); one[0, 1] = 1.0
    s.add_register("AC", one, scale_by_time=True)
    s.add_register("reward", [1.0, 0.0, 0.0, 1.0], kind="rewards", scale_by_time=True)
    rows, order = s.ancestral.node_list()
    times, rates = s.branch_times(order)
    regs, flags, eig_idx = np.stack(s.registers), s.flags(), tl.eigen_index()

    def jumps(seed, states=False):
        return s.beagle.sampleMarkovJumps(rows, times, rates, eig_idx, 0, 0, 0, regs, flags, seed, states=states)

    no_states = timed(lambda k: jumps(k), reps)
    with_states = timed(lambda k: jumps(k, states=True), reps)
    ancestral = timed(lambda k: s.beagle.sampleAncestralStates(rows, 0, 0, k), reps)
    out = {"taxa": wl.tip_count, "patterns": wl.pattern_count, "categories": wl.category_count, "rows": int(len(rows)),
           "registers": len(regs), "reps": reps, "jumps_no_states_ms": median_ms(no_states),
           "jumps_with_states_ms": median_ms(with_states), "sampleAncestralStates_ms": median_ms(ancestral)}
    if host_route:
        seed = 12345
        res = jumps(seed)
        t0 = time.perf_counter()
        st, ca = s.beagle.sampleAncestralStates(rows, 0, 0, seed)
        t1 = time.perf_counter()
        mats = np.zeros((len(rows), wl.category_count, S, S))
        for r in range(1, len(rows)):
            mats[r] = s.beagle.getTransitionMatrix(int(rows[r, 1])).reshape(wl.category_count, S, S)
        t2 = time.perf_counter()
        cond = mr.tables(wl.eig.evec, wl.eig.ievc, wl.eig.evals, s.registers, s.kinds, s.scale_by_time, times, rates, wl.cat_rates,
                         mats)
        _, tot, row_tot = mr.site_values(cond, st, rows[:, 2], ca)
        t3 = time.perf_counter()
        # the GPU tests' tolerance: 1e-12 relative, floor 1e-15 x the magnitudes of the summed entries
        mags = mr.magnitudes(wl.eig.evec, wl.eig.ievc, wl.eig.evals, s.registers, s.kinds, s.scale_by_time, times, rates,
                             wl.cat_rates, mats)
        _, fl_p, fl_r = mr.site_values(1e-15 * mags, st, rows[:, 2], ca)
        agree = bool(np.all(np.abs(res["pattern_totals"] - tot) <= 1e-12 * np.abs(tot) + fl_p) and
                     np.all(np.abs(res["row_totals"] - row_tot) <= 1e-12 * np.abs(row_tot) + fl_r))
        out.update({"host_route_ms": round(1e3 * (t3 - t0), 1), "host_route_draw_ms": round(1e3 * (t1 - t0), 1),
                    "host_route_getTransitionMatrix_ms": round(1e3 * (t2 - t1), 1),
                    "host_route_numpy_ms": round(1e3 * (t3 - t2), 1),
                    "speedup_vs_host_route": round((t3 - t0) / float(np.median(no_states)), 1),
                    "totals_agree_with_restatement": agree})
    tl.close()
    return out


def main():
    cache = bench.workload_cache_file(bench.default_cache_dir(), "A", 1.0, "coalescent")
    a = bench.load_workload(cache, lambda: bm.synth.config_a(scale=1.0))
    if "--trace" in sys.argv:
        print(json.dumps({"A/10": measure(a.shard(0, 10000), reps=5, host_route=False), "A": measure(a, reps=3, host_route=False)}))
        return
    out = {"source_hash": source_hash(), "kernel_source_hash": bench.kernel_source_hash()}
    out["A/10"] = measure(a.shard(0, 10000), reps=7)
    out["A"] = measure(a, reps=5)
    out["must_A_faster_than_sampleAncestralStates"] = out["A"]["jumps_no_states_ms"] < out["A"]["sampleAncestralStates_ms"]
    out["must_A/10_10x_vs_host_route"] = out["A/10"]["speedup_vs_host_route"] >= 10.0
    print(json.dumps(out))


if __name__ == "__main__":
    main()
