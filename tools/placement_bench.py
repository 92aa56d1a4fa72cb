#!/usr/bin/env python3
"""Scores of attaching new sequences on every branch in one call (beagleMi355PlacementScores via beast-mcmc_amd/placement.py)
against the read-back route (placement.Placement route="host": a getPartials per operand, a getTransitionMatrix per matrix, numpy on
BLAS — so this run also checks the call against it), against evaluating every augmented tree with the engine itself, and beside the
reference's own rule (route="distance": SimpleDistanceMatrix.calculatePairwiseDistance + getClosestTaxon, src/dr/app/realtime).

Shapes: 1000 taxa x 1e4 and x 1e5 patterns GTR+G4, 500 x 5e4 at 20 states, and the trait partition (1610 taxa, one pattern, 56
states, one category); 100 queries x every branch at its midpoint; one alignment site per pattern; a query is an existing taxon's row
with 5 % of the sites redrawn and 1 % missing; codes: the states and one fully ambiguous row.  Instances rescale, as a tree of this
size must.  Per shape: the whole call (median wall time of `--reps` calls), the kernel timer over the whole call and over a call with
ONE query without a kept site — the pendant tables, the log table and a product over one row of zero counts: the table stage, with
the bytes of the three partials per candidate it reads by design per second (a lower bound: the degenerate product's pass over the
table is inside the time) — their difference (counts + product), the host route once, split into getPartials, getTransitionMatrix and
numpy, the distance route, and the time of ONE ordinary evaluation of an augmented tree on the engine (median over a sample of
pairs), SCALED by queries x candidates: nobody runs 199 800 of them.  Prints one JSON line (profiles/placement_bench.json)."""
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
from beast_mcmc_amd.gradient import BranchGradient        # noqa: E402
from beast_mcmc_amd.inputs import substmodel, synth       # noqa: E402
from beast_mcmc_amd.placement import Placement            # noqa: E402

GOAL = 10.0                                               # the project's goal for a one-call entry over the route it replaces


def source_hash():
    h = hashlib.sha256()
    for f in ("kernels_placement.hip", "engine_placement.cpp"):
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
        else:
            yield name, trait_partition()


def make_queries(wl, Q, rng):
    S, P = wl.state_count, wl.pattern_count
    table = np.concatenate([np.eye(S), np.ones((1, S))])
    codes = np.minimum(np.asarray(wl.tip_states)[rng.integers(0, wl.tip_count, size=Q)], S).astype(np.uint8)
    redrawn = rng.random(codes.shape) < 0.05
    codes[redrawn] = rng.integers(0, S, size=int(redrawn.sum()))
    codes[rng.random(codes.shape) < 0.01] = 255
    return np.arange(P, dtype=np.int32), codes, table


def design_bytes(g, rows):
    """What the table stage reads by design: three partials per candidate, a compact tip's as P state bytes."""
    buf = g.P * g.S * g.C * 8
    total = 0
    for pre, sib, _, child, _, _, _ in rows:
        total += buf + sum((g.P if 0 <= x < g.T else buf) for x in (sib, child) if x >= 0)
    return total


def measure(wl, Q, reps, host, sample):
    rng = np.random.default_rng(7)
    g = Placement(wl, rescale=True, max_candidates=wl.tree.node_count)
    lnl = g.prepare()
    rows = g.candidates(fractions=(0.5,))
    pats, codes, table = make_queries(wl, Q, rng)
    scores, rc = g.scores(pats, codes, table)                              # (the held pre-order list runs here)
    g.b.synchronize()
    call = timed(lambda: g.scores(pats, codes, table), reps)
    again, _ = g.scores(pats, codes, table)
    launches0 = g.stats()["launches"]
    g.b.kernelTimer(1)
    for _ in range(reps):
        g.scores(pats, codes, table)
    k_ms, _ = g.b.kernelTimer(0)
    launches = (g.stats()["launches"] - launches0) // reps
    nothing = np.full((1, len(pats)), 255, dtype=np.uint8)
    g.scores(pats, nothing, table)
    g.b.kernelTimer(1)
    for _ in range(reps):
        g.scores(pats, nothing, table)
    t_ms, _ = g.b.kernelTimer(0)
    moved = design_bytes(g, rows)
    out = {"taxa": wl.tip_count, "patterns": wl.pattern_count, "states": g.S, "categories": g.C, "candidates": len(rows), "queries": Q,
           "sites": len(pats), "codes": len(table), "reps": reps, "lnL": lnl, "return_code": rc,
           "finite_scores_fraction": float(np.mean(np.isfinite(scores))),
           "call_ms": median_ms(call), "timer_whole_call_ms": round(k_ms / reps, 4), "launches": int(launches),
           "timer_table_stage_ms": round(t_ms / reps, 4), "counts_and_product_ms_by_difference": round((k_ms - t_ms) / reps, 4),
           "table_stage_design_bytes_read": int(moved), "table_stage_read_GBs_lower_bound": round(moved / (t_ms / reps * 1e-3) / 1e9, 1),
           "same_bits_every_call": bool(np.array_equal(again, scores, equal_nan=True))}
    t0 = time.perf_counter()
    closest, _ = g.scores(pats, codes, table, route="distance")
    out["distance_route_ms"] = round(1e3 * (time.perf_counter() - t0), 1)
    best = np.argmax(np.where(np.isfinite(scores), scores, -np.inf), axis=1)
    parent_of_closest = np.asarray(wl.tree.parent)[closest]
    out["best_candidate_is_the_closest_taxons_branch_or_its_parents"] = int(np.sum((rows[best, 3] == closest) | (rows[best, 3] == parent_of_closest)))
    # one ordinary evaluation of an augmented tree on the engine, on a sample of pairs; SCALED to every pair
    evals = []
    for _ in range(sample):
        aug = g.attach(codes[int(rng.integers(Q))], int(rng.integers(len(rows))), pats, table)
        e = BranchGradient(aug, rescale=True)
        e.b.setTipPartials(aug.new_tip, aug.new_tip_partials.ravel())
        e.log_likelihood(); e.b.synchronize()
        evals.append(float(np.median(timed(e.log_likelihood, 3))))
        e.close()
    if evals:
        one = float(np.median(evals))
        out.update({"augmented_tree_evaluation_ms_each": round(1e3 * one, 4), "augmented_tree_pairs_sampled": sample,
                    "augmented_tree_route_ms_SCALED_to_all_pairs": round(1e3 * one * Q * len(rows), 1),
                    "speedup_over_augmented_tree_route_scaled": round(one * Q * len(rows) / float(np.median(call)), 1)})
    if host:
        t0 = time.perf_counter()
        ref, _ = g.scores(pats, codes, table, route="host")
        t_ref = time.perf_counter() - t0
        hs = g.host_seconds
        both = np.isfinite(ref) & np.isfinite(scores)
        out.update({"host_route_ms": round(1e3 * t_ref, 1), "host_getPartials_ms": round(1e3 * hs["getPartials"], 1),
                    "host_getTransitionMatrix_ms": round(1e3 * hs["getTransitionMatrix"], 1), "host_numpy_ms": round(1e3 * hs["numpy"], 1),
                    "speedup_over_host_route": round(t_ref / float(np.median(call)), 1),
                    "largest_relative_difference_to_host_route": float(np.max(np.abs(ref[both] - scores[both]) / np.maximum(1.0, np.abs(ref[both])))) if both.any() else None})
        out["goal_10x_met"] = bool(out["speedup_over_host_route"] >= GOAL)
    g.close()
    return out


def main():
    names = ["1000 x 1e4 GTR+G4", "1000 x 1e5 GTR+G4", "500 x 5e4 x 20", "trait 1610 x 1 x 56"]
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--queries", type=int, default=100)
    ap.add_argument("--sample", type=int, default=3, help="pairs whose augmented tree is evaluated on the engine")
    ap.add_argument("--shapes", nargs="*", default=names, help="any of: " + "; ".join(names))
    ap.add_argument("--no-host-route", action="store_true")
    args = ap.parse_args()
    out = {"source_hash": source_hash(), "kernel_source_hash": bench.kernel_source_hash(), "goal": GOAL}
    for name, wl in workloads(args.shapes):
        out[name] = measure(wl, args.queries, args.reps, not args.no_host_route, args.sample)
        print(name, json.dumps(out[name]), file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
