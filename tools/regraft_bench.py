#!/usr/bin/env python3
"""Scores of every regraft point of a pruned subtree in one call (beagleMi355RegraftScores via beast-mcmc_amd/regraft.py) against the
route it replaces: the reference operator's loop (GibbsPruneAndRegraft: per candidate a tree edit, an evaluation, the edit back)
through the stock API on this same engine, with its branch-move fast path (regraft.Regraft route="host": per candidate three branch
matrices and the partials of the nodes above the two edits) — so this run also checks the call against it.

Shapes: 1000 taxa x 1e4 and x 1e5 patterns GTR+G4, 500 x 5e4 at 20 states, 200 x 2e4 at 61 states (one category).  Per shape
`--prunings` seeded nodes, each with every admissible candidate and the original position.  Instances rescale, as a tree of this size
must.  Per shape, medians over the prunings: the whole device route (prune + the candidates' matrices + the call, wall time to the
call's return, which waits for the device), the call alone (median of `--reps` calls), the kernel timer over the call, the bytes the
main stage reads by design per candidate — the three partials and the pendant vector, a compact tip's partials as P state bytes —
over the kernel time, and the host route.  Prints one JSON line (profiles/regraft_bench.json)."""
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
from beast_mcmc_amd.regraft import Regraft                # noqa: E402

GOAL = 10.0                                               # the project's goal for a one-call entry over the route it replaces
NODE_POSTERIOR_TBS = (3.9, 5.1)                           # what k_nodePosterior reads: the streaming rate beside ours


def source_hash():
    h = hashlib.sha256()
    for f in ("kernels_regraft.hip", "engine_regraft.cpp"):
        with open(os.path.join(ROOT, "beast-mcmc_amd", "csrc", f), "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


def codon_like():
    eig, pi = substmodel.random_reversible(61, np.random.default_rng(161))
    return synth.make_workload("200 x 2e4 x 61", 200, 20000, eig, pi, categories=1, seed=61)


def workloads(names):
    a = None
    for name in names:
        if name.startswith("1000 x"):
            if a is None:
                a = bench.load_workload(bench.workload_cache_file(bench.default_cache_dir(), "A", 1.0, "coalescent"), lambda: bm.synth.config_a(scale=1.0))
            yield name, (a.shard(0, 10000) if name == "1000 x 1e4 GTR+G4" else a)
        elif name == "500 x 5e4 x 20":
            yield name, bm.synth.config_b()
        else:
            yield name, codon_like()


def design_bytes(g, rows):
    """What the main stage reads by design: three partials and the pendant vector per candidate, a compact tip's as P state bytes."""
    buf = g.P * g.S * g.C * 8
    total = 0
    for pre, sib, _, child, _, _, _ in rows:
        total += 2 * buf + sum((g.P if 0 <= x < g.T else buf) for x in (sib, child) if x >= 0)
    return total


def med(xs, digits=4):
    return round(float(np.median(xs)), digits)


def measure(wl, prunings, reps, host):
    rng = np.random.default_rng(11)
    g = Regraft(wl, rescale=True, max_candidates=wl.tree.node_count)
    tr = wl.tree
    nodes = [n for n in range(tr.node_count) if n != tr.root and int(tr.parent[n]) != tr.root]
    picked = [int(x) for x in rng.choice(nodes, size=prunings, replace=False)]
    g.prune(picked[0]); g.regraft_candidates(picked[0]); g.scores()      # (code objects, scratch, the plan of a pruned tree's lists)
    g.b.synchronize()
    route, call, kernel, rate, host_ms, cands, worst, finite = [], [], [], [], [], [], 0.0, []
    for i in picked:
        t0 = time.perf_counter()
        g.prune(i)
        rows = g.regraft_candidates(i)
        lnl, rc = g.scores()
        route.append(1e3 * (time.perf_counter() - t0))
        cands.append(len(rows))
        finite.append(float(np.mean(np.isfinite(lnl))))
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            again, _ = g.scores()
            ts.append(1e3 * (time.perf_counter() - t0))
        assert np.array_equal(again, lnl, equal_nan=True)
        call.append(float(np.median(ts)))
        g.b.kernelTimer(1)
        for _ in range(reps):
            g.scores()
        k_ms, _ = g.b.kernelTimer(0)
        kernel.append(k_ms / reps)
        rate.append(design_bytes(g, rows) / (k_ms / reps * 1e-3) / 1e9)
        if host:
            g.b.synchronize()
            t0 = time.perf_counter()
            ref, _ = g.scores(route="host")
            host_ms.append(1e3 * (time.perf_counter() - t0))
            both = np.isfinite(ref) & np.isfinite(lnl)
            if both.any():
                worst = max(worst, float(np.max(np.abs(ref[both] - lnl[both]) / np.maximum(1.0, np.abs(ref[both])))))
    out = {"taxa": wl.tip_count, "patterns": wl.pattern_count, "states": g.S, "categories": g.C, "prunings": prunings, "reps": reps,
           "candidates_median": int(np.median(cands)), "candidates_min": int(min(cands)), "candidates_max": int(max(cands)),
           "finite_lnL_fraction": med(finite), "device_route_ms": med(route), "call_ms": med(call), "kernel_timer_ms": med(kernel),
           "design_read_GBs": med(rate, 1), "node_posterior_TBs_for_comparison": list(NODE_POSTERIOR_TBS),
           "launches_per_call": int(g.stats()["launches"] // g.stats()["calls"])}
    if host:
        ratio = [h / r for h, r in zip(host_ms, route)]
        out.update({"host_route_ms": med(host_ms, 1), "host_evaluations": int(g.host_evaluations),
                    "speedup_of_device_route_over_host_route": med(ratio, 1), "goal_10x_met": bool(np.median(ratio) >= GOAL),
                    "largest_relative_difference_to_host_route": worst})
    g.close()
    return out


def main():
    names = ["1000 x 1e4 GTR+G4", "1000 x 1e5 GTR+G4", "500 x 5e4 x 20", "200 x 2e4 x 61"]
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--prunings", type=int, default=10)
    ap.add_argument("--shapes", nargs="*", default=names, help="any of: " + "; ".join(names))
    ap.add_argument("--no-host-route", action="store_true")
    args = ap.parse_args()
    out = {"source_hash": source_hash(), "kernel_source_hash": bench.kernel_source_hash(), "goal": GOAL}
    for name, wl in workloads(args.shapes):
        out[name] = measure(wl, args.prunings, args.reps, not args.no_host_route)
        print(name, json.dumps(out[name]), file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
