#!/usr/bin/env python3
"""Tip error models at the headline size (1000 taxa x 100 000 patterns, GTR+G4): what an error-rate proposal and the evaluation behind it
cost the stock way — a setTipPartials per tip, BeagleTreeLikelihood.java:917-930 — and through beagleMi355SetTipEmission
(beast-mcmc_amd/tipmodels.py).

  (a) one error-rate proposal the stock way: 1000 setTipPartials calls (P * S doubles each; the host's own expansion of the table is
      timed apart) plus the evaluation;
  (b) the same through setTipEmission(codes=None): K * S doubles a tip, plus the evaluation;
  (c) a steady evaluation (every node dirty, nothing else changes) with every tip folded, beside the same alignment with plain compact
      tips and beside every tip as uploaded partials.

Three instances live side by side and are measured in alternating order, `--rounds` rounds in each order.  Wall times are medians of
synchronous evaluations (getLogLikelihood returns the value); kernel times come from the instance's kernel timer, which brackets the
pruning launches of an updatePartials call — the fold launch runs in front of that bracket, so what it costs shows in the wall times.
Writes one JSON object (profiles/tip_emission_bench.json) and prints it."""
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
from beast_mcmc_amd import tipmodels                      # noqa: E402
from beast_mcmc_amd.treelikelihood import BeagleTreeLikelihood  # noqa: E402

Beagle = bm.beagle.Beagle


def source_hash():
    h = hashlib.sha256()
    for f in ("kernels_tipemission.hip", "engine_tipemission.cpp"):
        with open(os.path.join(ROOT, "beast-mcmc_amd", "csrc", f), "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


def med_ms(ts):
    return round(1e3 * float(np.median(ts)), 4)


def steady(tl, raw, reps):
    """-> (wall seconds per evaluation [reps], kernel ms per evaluation, launches per evaluation)"""
    for _ in range(3):
        tl.makeDirty(); tl.getLogLikelihood()
    raw.kernelTimer(1)
    wall = []
    for _ in range(reps):
        tl.makeDirty()
        t0 = time.perf_counter()
        tl.getLogLikelihood()
        wall.append(time.perf_counter() - t0)
    ms, launches = raw.kernelTimer(0)
    return wall, ms / reps, launches / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--proposals", type=int, default=3)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tip_emission_bench.json"))
    args = ap.parse_args()
    cache = bench.workload_cache_file(bench.default_cache_dir(), "A", args.scale, "coalescent")
    wl = bench.load_workload(cache, lambda: bm.synth.config_a(scale=args.scale))
    T, P, S = wl.tip_count, wl.pattern_count, wl.state_count
    codes = np.ascontiguousarray(wl.tip_states, dtype=np.int32)
    ages = np.random.default_rng(4).uniform(0.0, 1.0, size=T)

    def tables(base):
        return [tipmodels.sequence_error_emission(tipmodels.ALL_SUBSTITUTIONS, base, 0.2, ages[t]) for t in range(T)]
    tabs = tables(0.01)
    kinds = ("folded", "compact", "partials")
    tls = {k: BeagleTreeLikelihood(wl) for k in kinds}
    raws = {k: Beagle.attach(tls[k]) for k in kinds}
    for t in range(T):
        raws["folded"].setTipEmission(t, codes[t], tabs[t])
        raws["partials"].setTipPartials(t, tipmodels.expand(codes[t], tabs[t]))
    lnl = {}
    for k in kinds:
        tls[k].makeDirty()
        lnl[k] = tls[k].getLogLikelihood()
    # (c) steady evaluations, alternating order
    wall = {k: [] for k in kinds}
    kern = {k: [] for k in kinds}
    launches = {}
    for r in range(2 * args.rounds):
        for k in (kinds if r % 2 == 0 else kinds[::-1]):
            w, ms, n = steady(tls[k], raws[k], args.reps)
            wall[k].append(float(np.median(w))); kern[k].append(ms); launches[k] = n
    # (a) / (b) one error-rate proposal and its evaluation, alternating
    stock, emission, stock_upload, stock_expand, emission_send = [], [], [], [], []
    for i in range(args.proposals):
        tabs = tables(0.01 + 0.002 * (i + 1))
        for which in (("a", "b") if i % 2 == 0 else ("b", "a")):
            if which == "a":
                t_expand = t_upload = 0.0
                t0 = time.perf_counter()
                for t in range(T):
                    t1 = time.perf_counter()
                    p = tipmodels.expand(codes[t], tabs[t])
                    t2 = time.perf_counter()
                    raws["partials"].setTipPartials(t, p)
                    t_expand += t2 - t1; t_upload += time.perf_counter() - t2
                tls["partials"].makeDirty()
                a_lnl = tls["partials"].getLogLikelihood()
                stock.append(time.perf_counter() - t0 - t_expand); stock_upload.append(t_upload); stock_expand.append(t_expand)
            else:
                t0 = time.perf_counter()
                for t in range(T):
                    raws["folded"].setTipEmission(t, None, tabs[t])
                t1 = time.perf_counter()
                tls["folded"].makeDirty()
                b_lnl = tls["folded"].getLogLikelihood()
                emission.append(time.perf_counter() - t0); emission_send.append(t1 - t0)
    stats = raws["folded"].tipEmissionStats()
    out = {"source_hash": source_hash(), "kernel_source_hash": bench.kernel_source_hash(),
           "taxa": T, "patterns": P, "states": S, "categories": wl.category_count, "reps": args.reps, "rounds": 2 * args.rounds,
           "lnL": lnl, "lnL_folded_vs_partials_rel": abs(lnl["folded"] - lnl["partials"]) / abs(lnl["partials"]),
           "c_steady_evaluation_wall_ms": {k: med_ms(wall[k]) for k in kinds},
           "c_steady_evaluation_wall_ms_by_round": {k: [round(1e3 * x, 4) for x in wall[k]] for k in kinds},
           "c_steady_evaluation_kernel_ms": {k: round(float(np.median(kern[k])), 4) for k in kinds},
           "c_launches_in_the_timer_bracket": launches,
           "c_folded_minus_compact_wall_ms": round(med_ms(wall["folded"]) - med_ms(wall["compact"]), 4),
           "c_folded_minus_compact_kernel_ms": round(float(np.median(kern["folded"]) - np.median(kern["compact"])), 4),
           "c_partials_over_folded_wall": round(float(np.median(wall["partials"]) / np.median(wall["folded"])), 2),
           "a_stock_proposal_ms": med_ms(stock), "a_of_which_setTipPartials_ms": med_ms(stock_upload),
           "a_host_expansion_not_counted_ms": med_ms(stock_expand), "a_bytes_per_proposal": int(T) * P * S * 8,
           "b_emission_proposal_ms": med_ms(emission), "b_of_which_setTipEmission_ms": med_ms(emission_send),
           "b_bytes_per_proposal": int(T) * 4 * S * 8, "a_over_b": round(float(np.median(stock) / np.median(emission)), 1),
           "proposal_lnL_rel": abs(a_lnl - b_lnl) / abs(a_lnl), "tip_emission_stats": stats,
           "device_bytes": {k: int(raws[k].deviceBytes()) for k in kinds}}
    for k in kinds:
        tls[k].close()
    text = json.dumps(out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
