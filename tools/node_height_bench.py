#!/usr/bin/env python3
"""Node-height gradient and diagonal Hessian of every internal node in one call (beagleMi355NodeHeightDerivatives via
beast-mcmc_amd/nodeheight.py) against the route DiscreteTraitNodeHeightDelegate.getNodeDerivatives takes through the BEAGLE
interface (src/dr/evomodel/treedatalikelihood/discrete/DiscreteTraitNodeHeightDelegate.java:63-200): a getPartials per post-order
and per pre-order buffer, a getTransitionMatrix per branch, then the loops on the host (numpy: tests/node_height_reference.py, the
restatement the GPU tests compare against — so this run also checks the call against it), and against the fused branch gradient
with second derivatives (gradient.BranchGradient.gradient(second=True)) in the same run.

1000 taxa, GTR+G4, 10 000 and 100 000 patterns, clock rates uniform on [0.5, 2], buffers alternating between two sets.  The call is
timed alone (everything it reads resident, the pre-order list already run): median wall time of `--reps` calls, and kernel time per
call from the instance's kernel timer.  The read-back route runs at 10 000 patterns only (at 100 000 its partials are 51 GB of
host memory).  Prints one JSON line (profiles/node_height_bench.json)."""
import argparse
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np                                        # noqa: E402
import node_height_reference as nr                        # noqa: E402
import beast_mcmc_amd as bm                               # noqa: E402
import bench                                              # noqa: E402
from beast_mcmc_amd.nodeheight import NodeHeightGradient  # noqa: E402


def source_hash():
    h = hashlib.sha256()
    for f in ("kernels_nodeheight.hip", "engine_nodeheight.cpp"):
        with open(os.path.join(ROOT, "beast-mcmc_amd", "csrc", f), "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


def median_ms(ts):
    return round(1e3 * float(np.median(ts)), 3)


def timed(fn, reps):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    return out


def design_bytes(g):
    """What the call reads by design: pre(i) and both children's post-order partials per internal node, a tip as P state bytes."""
    buf = g.P * g.S * g.C * 8
    tr = g.tree
    total = 0
    for i in g.internal:
        total += buf + sum(buf if int(ch) >= g.T else g.P for ch in (tr.left[i], tr.right[i]))
    return total


def measure(wl, reps, readback):
    rates = np.random.default_rng(12).uniform(0.5, 2.0, size=wl.tree.node_count)
    g = NodeHeightGradient(wl, rates=rates, double_buffer=True)
    for _ in range(3):                                     # (the first evaluations of an instance allocate both buffer sets)
        lnl, first, second = g.derivatives()
    full = timed(lambda: g.derivatives(), reps)
    first_only = timed(lambda: g.derivatives(second=False), reps)
    for _ in range(3):
        g.gradient(second=True)
    branch = timed(lambda: g.gradient(second=True), reps)
    branch_first = timed(lambda: g.gradient(), reps)
    # the call alone
    lnl = g.prepare()
    rows, rt = g.node_rows()
    first, second = g.b.nodeHeightDerivatives(rows, rt)     # (the held pre-order list runs here)
    g.b.synchronize()
    call = timed(lambda: g.b.nodeHeightDerivatives(rows, rt), reps)
    call_first = timed(lambda: g.b.nodeHeightDerivatives(rows, rt, second=False), reps)
    g.b.kernelTimer(1)
    for _ in range(reps):
        again = g.b.nodeHeightDerivatives(rows, rt)
    kernel_ms, launches = g.b.kernelTimer(0)
    moved = design_bytes(g)
    out = {"taxa": wl.tip_count, "patterns": wl.pattern_count, "categories": wl.category_count, "internal_nodes": int(len(g.internal)),
           "reps": reps, "lnL": lnl,
           "call_ms": median_ms(call), "call_first_only_ms": median_ms(call_first),
           "call_kernel_ms": round(kernel_ms / reps, 3), "call_launches": int(launches // reps),
           "design_bytes": int(moved), "achieved_GBs_kernel": round(moved / (kernel_ms / reps * 1e-3) / 1e9, 1),
           "achieved_GBs_wall": round(moved / float(np.median(call)) / 1e9, 1),
           "evaluation_with_call_ms": median_ms(full), "evaluation_with_call_first_only_ms": median_ms(first_only),
           "branch_gradient_second_ms": median_ms(branch), "branch_gradient_first_only_ms": median_ms(branch_first),
           "evaluation_with_call_over_branch_gradient_second": round(float(np.median(full)) / float(np.median(branch)), 3),
           "same_bits_every_call": bool(np.array_equal(again[0], first) and np.array_equal(again[1], second))}
    if readback:
        g.prepare()
        raw_get, raw_mat = g.b.getPartials, g.b.getTransitionMatrix
        spent = {"partials": 0.0, "matrices": 0.0, "n_partials": 0, "n_matrices": 0}

        def get_partials(*a):
            t0 = time.perf_counter()
            v = raw_get(*a)
            spent["partials"] += time.perf_counter() - t0; spent["n_partials"] += 1
            return v

        def get_matrix(*a):
            t0 = time.perf_counter()
            v = raw_mat(*a)
            spent["matrices"] += time.perf_counter() - t0; spent["n_matrices"] += 1
            return v

        g.b.getPartials, g.b.getTransitionMatrix = get_partials, get_matrix
        t0 = time.perf_counter()
        fr, sr = nr.from_plan(g)
        t_ref = time.perf_counter() - t0
        del g.b.getPartials, g.b.getTransitionMatrix
        scale1, scale2 = max(1.0, float(np.max(np.abs(fr)))), max(1.0, float(np.max(np.abs(sr))))
        out.update({"readback_route_ms": round(1e3 * t_ref, 1), "readback_getPartials_ms": round(1e3 * spent["partials"], 1),
                    "readback_getPartials_calls": spent["n_partials"], "readback_getTransitionMatrix_ms": round(1e3 * spent["matrices"], 1),
                    "readback_getTransitionMatrix_calls": spent["n_matrices"],
                    "readback_host_loops_ms": round(1e3 * (t_ref - spent["partials"] - spent["matrices"]), 1),
                    "speedup_vs_readback_route": round(t_ref / float(np.median(call)), 1),
                    "first_error_vs_restatement": float(np.max(np.abs(first - fr)) / scale1),
                    "second_error_vs_restatement": float(np.max(np.abs(second - sr)) / scale2)})
    g.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--patterns", type=int, nargs="*", default=[10000, 100000])
    args = ap.parse_args()
    cache = bench.workload_cache_file(bench.default_cache_dir(), "A", 1.0, "coalescent")
    a = bench.load_workload(cache, lambda: bm.synth.config_a(scale=1.0))
    out = {"source_hash": source_hash(), "kernel_source_hash": bench.kernel_source_hash()}
    for p in args.patterns:
        out["%d patterns" % p] = measure(a if p >= a.pattern_count else a.shard(0, p), args.reps, readback=p <= 10000)
    if "10000 patterns" in out:
        out["goal_10x_over_readback_at_10000_met"] = out["10000 patterns"]["speedup_vs_readback_route"] >= 10.0
    print(json.dumps(out))


if __name__ == "__main__":
    main()
