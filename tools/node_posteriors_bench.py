#!/usr/bin/env python3
"""Marginal state posteriors of every node in one call (beagleMi355NodePosteriors via beast-mcmc_amd/nodeposteriors.py) against the
route NodePosteriorTreeLikelihood takes (src/dr/oldevomodel/treelikelihood/NodePosteriorTreeLikelihood.java:119-235): a getPartials
and a getTransitionMatrix per node, then traverseForward / calculatePosteriors on the host (numpy, the branch products on BLAS:
nodeposteriors.NodePosteriors route="host" — so this run also checks the call against it).

Shapes: 1000 taxa x 1e4 and x 1e5 patterns GTR+G4, 500 x 5e4 at 20 states, 200 x 2e4 at 61 states, and the trait partition (1610
taxa, one pattern, 56 states, one category).  Everything the call reads is resident (the pre-order list has run).  Per shape: the whole
call with state totals and MAP states only and with the full posteriors of every node (median wall time of `--reps` calls into
arrays that are reused), the kernels alone (a totals-only call: one launch, no copy-out between the kernel timer's events) with the
bytes they read per second, and the host route once, split into getPartials, getTransitionMatrix and numpy.  The host route forms totals and MAP states; both speed-ups are against
that one run (forming the full array on the host costs more, so the second is a lower bound).  Prints one JSON line
(profiles/node_posteriors_bench.json)."""
import argparse
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np                                        # noqa: E402
import beast_mcmc_amd as bm                               # noqa: E402
import bench                                              # noqa: E402
from beast_mcmc_amd.inputs import substmodel, synth       # noqa: E402
from beast_mcmc_amd.nodeposteriors import NodePosteriors  # noqa: E402

GOAL = 10.0                                               # the project's goal for a one-call entry over the route it replaces
NODE_HEIGHT_GBS = {"1000 x 1e4 GTR+G4": 4610.9, "1000 x 1e5 GTR+G4": 4687.7}      # k_nodeHeight, profiles/node_height_bench.json


def source_hash():
    h = hashlib.sha256()
    for f in ("kernels_nodeposterior.hip", "engine_nodeposterior.cpp"):
        with open(os.path.join(ROOT, "beast-mcmc_amd", "csrc", f), "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


def median_ms(ts):
    return round(1e3 * float(np.median(ts)), 4)


def timed(fn, reps):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    return out


def trait_partition():
    eig, pi = substmodel.random_reversible(56, np.random.default_rng(156))
    return synth.make_workload("trait 1610 x 56", 1610, 1, eig, pi, categories=1, seed=56)


def workloads(names):
    a = None
    for name in names:
        if name.startswith("1000 x"):
            if a is None:
                a = bench.load_workload(bench.workload_cache_file(bench.default_cache_dir(), "A", 1.0, "coalescent"), lambda: bm.synth.config_a(scale=1.0))
            yield name, (a.shard(0, 10000) if name == "1000 x 1e4 GTR+G4" else a)
        elif name == "500 x 5e4 x 20":
            yield name, bm.synth.config_b()
        elif name == "200 x 2e4 x 61":
            yield name, bm.synth.config_c()
        else:
            yield name, trait_partition()


def design_bytes(g):
    """What the kernel reads by design: pre(i) and post(i) per node, a compact tip's post as P state bytes."""
    buf = g.P * g.S * g.C * 8
    return g.N * buf + (g.N - g.T) * buf + g.T * g.P


def measure(wl, reps, host):
    g = NodePosteriors(wl)
    lnl = g.prepare()
    small = g.posteriors(full=False, map=True, totals=True)                 # (the held pre-order list runs here)
    full = g.posteriors(full=True)
    g.b.synchronize()
    call_small = timed(lambda: g.posteriors(full=False, map=True, totals=True, out=small), reps)
    call_full = timed(lambda: g.posteriors(full=True, out=full), max(3, reps // 2))
    again = g.posteriors(full=False, map=True, totals=True)
    # the kernels alone: totals only, so that every row is in ONE launch and no copy-out sits between the timer's two events
    g.b.kernelTimer(1)
    for _ in range(reps):
        g.posteriors(full=False, totals=True)
    k_ms, launches = g.b.kernelTimer(0)
    moved = design_bytes(g)
    out = {"taxa": wl.tip_count, "patterns": wl.pattern_count, "states": g.S, "categories": g.C, "node_rows": g.N, "reps": reps, "lnL": lnl,
           "call_totals_map_ms": median_ms(call_small), "call_full_ms": median_ms(call_full),
           "full_output_bytes": int(g.N * g.P * g.S * 8),
           "kernels_totals_ms": round(k_ms / reps, 4), "launches_totals": int(launches // reps),
           "design_bytes_read": int(moved), "read_GBs_kernels": round(moved / (k_ms / reps * 1e-3) / 1e9, 1),
           "same_bits_every_call": bool(np.array_equal(again["totals"], small["totals"]) and np.array_equal(again["map_states"], small["map_states"])),
           "rows_sum_to_one_max_error": float(np.max(np.abs(full["posteriors"].sum(axis=2) - 1.0)))}
    if host:
        t0 = time.perf_counter()
        ref = g.posteriors(full=False, map=True, totals=True, route="host")
        t_ref = time.perf_counter() - t0
        hs = g.host_seconds
        out.update({"host_route_ms": round(1e3 * t_ref, 1), "host_getPartials_ms": round(1e3 * hs["getPartials"], 1),
                    "host_getTransitionMatrix_ms": round(1e3 * hs["getTransitionMatrix"], 1), "host_numpy_ms": round(1e3 * hs["numpy"], 1),
                    "speedup_totals_map": round(t_ref / float(np.median(call_small)), 1),
                    "speedup_full_lower_bound": round(t_ref / float(np.median(call_full)), 1),
                    "totals_error_vs_host_route": float(np.max(np.abs(ref["totals"] - small["totals"])) / float(np.sum(wl.weights))),
                    "map_states_differing": int(np.sum(ref["map_states"] != small["map_states"]))})
        out["goal_10x_met"] = bool(out["speedup_totals_map"] >= GOAL and out["speedup_full_lower_bound"] >= GOAL)
    g.close()
    return out


def main():
    names = ["1000 x 1e4 GTR+G4", "1000 x 1e5 GTR+G4", "500 x 5e4 x 20", "200 x 2e4 x 61", "trait 1610 x 1 x 56"]
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--shapes", nargs="*", default=names, help="any of: " + "; ".join(names))
    ap.add_argument("--no-host-route", action="store_true")
    args = ap.parse_args()
    out = {"source_hash": source_hash(), "kernel_source_hash": bench.kernel_source_hash(), "goal": GOAL,
           "k_nodeHeight_read_GBs_for_context": NODE_HEIGHT_GBS}
    for name, wl in workloads(args.shapes):
        out[name] = measure(wl, args.reps, not args.no_host_route)
        print(name, json.dumps(out[name]), file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
