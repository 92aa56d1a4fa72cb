#!/usr/bin/env python3
"""Transition matrices straight from generators in one call (beagleMi355UpdateTransitionMatricesFromGenerators via
beast-mcmc_amd/generators.py) against the route SubstitutionModelDelegate takes through the BEAGLE interface for a model without a
symmetric form (SubstitutionModelDelegate.java:213-288; ComplexSubstitutionModel.java:121-173): per model a non-symmetric
decomposition and an inverse on the host — numpy.linalg.eig + inv inside inputs.substmodel.decompose_complex — a
setEigenDecomposition, and the updateTransitionMatrices over its branches.

Shapes: the Makona trait partition (1610 taxa x 56 states x 1 category, one BSSVS-like generator, one pattern), 1000 taxa x 20 states
x 4 categories with one generator, 200 taxa x 61 states with a generator per branch (398), 1000 taxa x 4 states with a generator
per branch (1998), and one 4-state generator over 10 branches — the case the device is expected to lose.  Per shape: the device call
(median wall time of `--reps` calls, each waited for; its kernels' times when `--kernel-trace DIR` names the output of a rocprofv3
--kernel-trace run over `--trace-calls`), the host route and the decompositions' share of it, the largest difference between the two
routes' matrices, the lowest entry either route wrote, and a whole evaluation by both routes.  Prints one JSON line
(profiles/generator_matrices_bench.json)."""
import argparse
import csv
import glob
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
import generator_matrices_reference as gr                 # noqa: E402
import helpers                                            # noqa: E402
from beast_mcmc_amd import generators                     # noqa: E402
from beast_mcmc_amd.gradient import BranchGradient        # noqa: E402

NONE = bm.beagle.NONE
# name -> (states, categories, taxa, patterns, a generator per branch?, kind of generator)
SHAPES = {"makona 1610 x 56": (56, 1, 1610, 1, False, "bssvs"), "1000 x 20 x 4": (20, 4, 1000, 64, False, "dense"),
          "200 x 61, 398 generators": (61, 1, 200, 64, True, "bssvs"), "1000 x 4, 1998 generators": (4, 4, 1000, 64, True, "dense"),
          "1 generator x 4 x 10 branches": (4, 4, 6, 64, False, "dense")}


def source_hash():
    h = hashlib.sha256()
    for f in ("kernels_generator.hip", "engine_generator.cpp"):
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


class Evaluation(BranchGradient):
    """BranchGradient's buffer plan and post-order list over branch matrices formed by a GeneratorModelSet route."""

    def __init__(self, wl, models, per_branch, route):
        wl.eig = models.host_decomposition(0)
        super().__init__(wl, eigen_count=models.eigen_buffer_count, requirement_flags=bm.beagle.FLAG_EIGEN_COMPLEX)
        self.models, self.route = models, route
        self.gen = np.arange(len(self._nodes), dtype=np.int32) if per_branch else None

    def matrices(self):
        self.models.update_matrices(self.b, self._edge_matrix[0], self.branch_lengths[self._nodes], self.gen,
                                    None if self.gen is None else np.zeros(len(self._nodes), dtype=np.int32), route=self.route)

    def log_likelihood(self):
        self.matrices()
        self.b.updatePartials(self._post_ops, len(self._post_ops) // 7, NONE)
        out = [0.0]
        self.b.calculateRootLogLikelihoods([self.post_index(self.tree.root)], [0], [0], [NONE], 1, out)
        return out[0]


def plan(name, route):
    S, categories, taxa, patterns, per_branch, kind = SHAPES[name]
    wl = helpers.random_workload(taxa, patterns, S, categories, seed=400 + S)
    count = wl.tree.node_count - 1 if per_branch else 1
    rng = np.random.default_rng(500 + S)
    models = generators.GeneratorModelSet(S, count, route=route)
    for k in range(count):
        models.set_generator(k, generators.normalised(getattr(gr, kind)(S, rng)))
    return Evaluation(wl, models, per_branch, route)


def trace_calls(reps):
    """Only the device calls, `reps` of each shape in the order of SHAPES after one warm-up call each: what --kernel-trace reads."""
    for name in SHAPES:
        ev = plan(name, "device")
        for _ in range(reps + 1):
            ev.matrices()
            ev.b.synchronize()
        ev.close()


def launches_per_call(name):
    """Parts a call of this shape is cut into (engine_generator.cpp: 128 MiB of power tables, a quarter of the 16 MiB staging ring)"""
    S, _, taxa, _, per_branch, _ = SHAPES[name]
    count = 2 * taxa - 2 if per_branch else 1
    per = max(1, min((128 << 20) // (21 * S * S * 8), (4 << 20) // ((S * S + 1) * 8), count))
    return -(-count // per)


def kernel_times(directory, reps):
    """-> {shape: {"powers": us, "matrices": us}}: per call the summed time of its power-table and of its matrix dispatches, median over
    the calls, from the per-dispatch trace of a --trace-calls run (the k_generator* dispatches in order; a shape's first call is
    the warm-up)."""
    files = glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        raise SystemExit("no *kernel_trace.csv under %s" % directory)
    rows = []
    for f in files:
        with open(f) as fh:
            for row in csv.DictReader(fh):
                if "k_generator" in row["Kernel_Name"]:
                    rows.append((int(row["Start_Timestamp"]), "powers" if "Powers" in row["Kernel_Name"] else "matrices",
                                 int(row["End_Timestamp"]) - int(row["Start_Timestamp"])))
    rows.sort()
    expected = sum(2 * launches_per_call(name) * (reps + 1) for name in SHAPES)
    if len(rows) != expected:
        raise SystemExit("%d k_generator dispatches in the trace, expected %d" % (len(rows), expected))
    out, at = {}, 0
    for name in SHAPES:
        per_call = 2 * launches_per_call(name)
        calls = [rows[at + c * per_call:at + (c + 1) * per_call] for c in range(1, reps + 1)]
        at += per_call * (reps + 1)
        out[name] = {k: round(float(np.median([sum(d for _, kk, d in call if kk == k) for call in calls])) / 1e3, 2)
                     for k in ("powers", "matrices")}
        out[name]["launches_per_call"] = per_call
    return out


def measure(name, reps):
    S, categories, taxa, patterns, per_branch, kind = SHAPES[name]
    dev, host = plan(name, "device"), plan(name, "host")
    n, count = len(dev._nodes), dev.models.count

    def run(ev):
        ev.matrices()
        ev.b.synchronize()

    run(dev); run(host)
    slots = dev._edge_matrix[0][:16]
    m_dev = np.stack([dev.b.getTransitionMatrix(int(s)) for s in slots])
    m_host = np.stack([host.b.getTransitionMatrix(int(s)) for s in slots])
    call = timed(lambda: run(dev), reps)
    host_reps = max(1, reps // 3)
    route = timed(lambda: run(host), host_reps)
    decompose = timed(lambda: [host.models.host_decomposition(k) for k in range(count)], host_reps)
    stats = dev.b.generatorStats()
    for _ in range(2):
        ld, lh = dev.log_likelihood(), host.log_likelihood()
    ev_dev = timed(dev.log_likelihood, reps)
    ev_host = timed(host.log_likelihood, host_reps)
    out = {"states": S, "categories": categories, "branches": n, "generators": count, "patterns": patterns, "reps": reps,
           "device_call_ms": median_ms(call), "input_MB": round((count * S * S + n) * 8 / 1e6, 3),
           "power_tables_MB": round(count * 21 * S * S * 8 / 1e6, 3), "largest_s": stats["max_squarings"], "refused": stats["refused"],
           "host_route_ms": median_ms(route), "host_decompositions_ms": median_ms(decompose),
           "speedup_vs_host_route": round(float(np.median(route)) / float(np.median(call)), 2),
           "max_abs_difference_of_routes_first_16_branches": float(np.max(np.abs(m_dev - m_host))),
           "lowest_entry_device_route": float(m_dev.min()), "lowest_entry_host_route": float(m_host.min()),
           "evaluation_device_route_ms": median_ms(ev_dev), "evaluation_host_route_ms": median_ms(ev_host),
           "evaluation_speedup": round(float(np.median(ev_host)) / float(np.median(ev_dev)), 2),
           "evaluation_routes_relative_difference": abs(ld - lh) / abs(lh)}
    dev.close(); host.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--trace-calls", action="store_true", help="only the device calls (the program of a rocprofv3 --kernel-trace run)")
    ap.add_argument("--kernel-trace", help="directory of that run's csv output: kernel times join the record")
    ap.add_argument("--shapes", nargs="*", default=list(SHAPES))
    args = ap.parse_args()
    if args.trace_calls:
        trace_calls(args.reps)
        return
    out = {"source_hash": source_hash(),
           "host_route": "inputs.substmodel.decompose_complex (numpy.linalg.eig + inv) + setEigenDecomposition per model + updateTransitionMatrices[WithMultipleModels]"}
    kernels = kernel_times(args.kernel_trace, args.reps) if args.kernel_trace else {}
    for name in args.shapes:
        out[name] = measure(name, args.reps)
        if name in kernels:
            out[name]["device_kernel_us"] = kernels[name]
    out["device_route_faster"] = {k: out[k]["speedup_vs_host_route"] > 1.0 for k in args.shapes}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
