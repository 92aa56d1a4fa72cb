#!/usr/bin/env python3
"""One simulant of complete histories on the device (beagleMi355SimulateCompleteHistories via beast-mcmc_amd/completehistory.py)
against the host route — one Gillespie loop per (branch, site) on the host, which is what a caller of
dr.app.beagle.tools.CompleteHistorySimulator runs today (numpy: tests/complete_history_reference.py, the restatement the GPU tests
compare against, timed on a subset of sites and scaled linearly; this run also checks the device's states and counts against it)
— and against beagleMi355SimulateSequences over the same rows x sites in the same run: the same walk without the Gillespie loop.

GTR+G4 at 1000 taxa x 1e4 and x 1e5 sites, and the 20- and 61-state models at the sizes of configs B and C; three registers (all
jumps, a random labelling, a reward).  Device times are whole calls ending in the copy of the results to the host, median of 7
(fewer where one call returns more than 1 GiB of values; "reps" says how many): totals only (tip states, row totals, site totals),
all values, and the event list.  Prints one JSON line (profiles/complete_history_bench.json).

--trace: a few calls of each kind at 1000 x 1e4 and nothing else, for a ``rocprofv3 --kernel-trace --stats`` run of its own."""
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np                                        # noqa: E402
import complete_history_reference as hr                   # noqa: E402
from beast_mcmc_amd.completehistory import CompleteHistorySimulator          # noqa: E402
from beast_mcmc_amd.inputs import substmodel, synth       # noqa: E402
from beast_mcmc_amd.simulate import SequenceSimulator     # noqa: E402
from beast_mcmc_amd.treelikelihood import BeagleTreeLikelihood, RESCALE_DYNAMIC   # noqa: E402

HOST_SITES = 256


def source_hash():
    h = hashlib.sha256()
    for f in ("kernels_history.hip", "engine_history.cpp"):
        with open(os.path.join(ROOT, "beast-mcmc_amd", "csrc", f), "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


def median_ms(ts):
    return round(1e3 * float(np.median(ts)), 3)


def timed(call, reps):
    ts = []
    for k in range(reps):
        t0 = time.perf_counter()
        out = call(k)
        ts.append(time.perf_counter() - t0)
    return out, ts


def models():
    """(name, taxa, sites, eigen system, frequencies, seed): the trees and models of tools/simulate_bench.py."""
    pi = np.array([0.30, 0.20, 0.22, 0.28])
    gtr = substmodel.gtr([1.0, 4.0, 0.8, 1.2, 4.5, 1.0], pi)
    aa, aa_pi = substmodel.random_reversible(20, np.random.default_rng(111))
    rng = np.random.default_rng(121)
    codon, codon_pi = substmodel.gy94(2.0, 0.2, rng.dirichlet(np.full(61, 20.0)))
    return [("GTR+G4 1000x1e4", 1000, 10000, gtr, pi, 1), ("GTR+G4 1000x1e5", 1000, 100000, gtr, pi, 1),
            ("AA20+G4 500x5e4", 500, 50000, aa, aa_pi, 11), ("GY94+G4 200x2e4", 200, 20000, codon, codon_pi, 21)]


def simulator(tl, S, seed):
    sim = CompleteHistorySimulator(tl)
    rng = np.random.default_rng(seed)
    sim.add_register("all", np.ones((S, S)) - np.eye(S))
    sim.add_register("labelled", (rng.random((S, S)) < 0.5).astype(np.float64) * (1.0 - np.eye(S)))
    sim.add_register("reward", rng.uniform(0.5, 2.0, size=S), "rewards")
    return sim


def measure(name, taxa, sites, eig, pi, seed, reps, trace=False):
    S = len(pi)
    wl = synth.make_workload(name, taxa, 64, eig, pi, seed=seed)
    tl = BeagleTreeLikelihood(wl, rescaling=RESCALE_DYNAMIC, delay_rescaling=False)
    tl.getLogLikelihood()                                 # (the model arrays set, and the simulator's branch matrices)
    sim, seq = simulator(tl, S, seed), SequenceSimulator(tl)
    rows, order = sim.node_list(True)
    value_bytes = 3 * len(rows) * sites * 8
    reps_values = reps if value_bytes <= (1 << 30) else 3
    if trace:
        reps = reps_values = 3
    sim.simulate(sites, 0, per_site=True, history=True)   # first call: scratch allocation
    seq.simulate(sites, 0, ancestral=True)
    last = 100 + reps - 1
    totals, t_totals = timed(lambda k: sim.simulate(sites, 100 + k, ancestral=False, per_site=False), reps)
    _, t_values = timed(lambda k: sim.simulate(sites, 200 + k, ancestral=False, per_site=True), reps_values)
    events, t_events = timed(lambda k: sim.simulate(sites, 100 + k, ancestral=True, per_site=False, history=True), reps)
    _, t_seq = timed(lambda k: seq.simulate(sites, 100 + k), reps)
    _, t_seq_all = timed(lambda k: seq.simulate(sites, 100 + k, ancestral=True), reps)
    if trace:
        tl.close()
        return {"name": name, "totals_only_ms": median_ms(t_totals), "simulate_sequences_tips_only_ms": median_ms(t_seq)}
    # the host route on the first HOST_SITES sites of the last seed, scaled to all sites
    sub = np.arange(min(HOST_SITES, sites))
    lengths = sim.branch_lengths(order)
    t0 = time.perf_counter()
    ref = hr.simulate(rows, lengths, np.stack(sim.generators), np.stack(sim.registers), sim.flags(), wl.cat_rates, wl.cat_weights, wl.freqs,
                      last, sites, heights=sim.node_heights(order), sites=sub)
    t_ref = (time.perf_counter() - t0) * sites / len(sub)
    got = np.vstack([events["alignment"], events["ancestral"]])[:, sub]
    identical = bool(np.array_equal(got[order], ref["states"]) and np.array_equal(events["categories"][sub], ref["categories"]) and
                     np.array_equal(events["event_counts"][:, sub][order], ref["counts"]) and not ref["bad"] and
                     np.array_equal(totals["alignment"], events["alignment"]))
    tl.close()
    dev = float(np.median(t_totals))
    return {"name": name, "taxa": taxa, "sites": sites, "states": S, "categories": wl.category_count, "rows": int(len(rows)),
            "registers": 3, "reps": reps, "reps_all_values": reps_values, "events_per_simulant": int(events["events"]["site"].size),
            "jumps_per_branch_and_site": round(float(events["events"]["site"].size) / ((len(rows) - 1) * sites), 4),
            "device_totals_only_ms": median_ms(t_totals), "device_all_values_ms": median_ms(t_values),
            "device_events_ms": median_ms(t_events), "all_values_bytes": value_bytes,
            "host_route_sites_timed": int(len(sub)), "host_route_scaled_ms": round(1e3 * t_ref, 1),
            "speedup_vs_host_route": round(t_ref / dev, 1),
            "simulate_sequences_tips_only_ms": median_ms(t_seq), "simulate_sequences_all_nodes_ms": median_ms(t_seq_all),
            "totals_only_vs_simulate_sequences": round(dev / float(np.median(t_seq)), 2),
            "subset_identical_to_restatement": identical}


def main():
    if "--trace" in sys.argv:
        name, taxa, sites, eig, pi, seed = models()[0]
        print(json.dumps(measure(name, taxa, sites, eig, pi, seed, reps=3, trace=True)))
        return
    out = {"history_source_hash": source_hash(), "cases": []}
    for name, taxa, sites, eig, pi, seed in models():
        out["cases"].append(measure(name, taxa, sites, eig, pi, seed, reps=7))
    out["goal_10x_host_route_at_1e4_sites_met"] = bool(out["cases"][0]["speedup_vs_host_route"] >= 10.0)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
