#!/usr/bin/env python3
"""Branch matrices of epoch models in one call (beagleMi355UpdateTransitionMatricesWithEpochs via beast-mcmc_amd/epochs.py
route="device") against the reference's protocol over the stock natives on the same build and GPU (route="host":
SubstitutionModelDelegate.java:162-405 restated — a pool of 100 extra matrix buffers, one updateTransitionMatrices per eigen system,
rounds of convolveTransitionMatrices, flushes when the pool runs short).  The host route uses only natives this extension does not
touch.

Shapes: 1000 taxa x 4 states x 4 categories and 500 x 20 x 4 with three epochs, 200 x 61 with three, the Makona trait partition
(1610 taxa x 56 states x 1 category) with two.  The boundaries sit at low quantiles of the internal nodes' heights, so that most branches cross at
least one (the record says how many cross how many).  Per shape: the call (median wall time of `--reps` calls, each waited for), the
host route and the natives it issues per evaluation, the largest difference between the two routes' matrices, a whole evaluation
(matrices + updatePartials + root) by both routes, and — when `--kernel-trace DIR` names the output of a rocprofv3 --kernel-trace run
over `--trace-calls` — the kernel time of either route per call.  Prints one JSON line (profiles/epoch_matrices_bench.json)."""
import argparse
import copy
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
import helpers                                            # noqa: E402
from beast_mcmc_amd import epochs                         # noqa: E402
from beast_mcmc_amd.gradient import BranchGradient        # noqa: E402
from beast_mcmc_amd.inputs import substmodel              # noqa: E402

NONE = bm.beagle.NONE
GOAL = 10.0                                               # the project's goal for a one-call entry over the route it replaces
PHASE_GAP_S = 0.05                                        # --trace-calls: idle time between two phases (kernel_times splits the trace there)
# name -> (states, categories, taxa, patterns, models, quantiles of the internal nodes' heights the boundaries sit at)
SHAPES = {"1000 x 4 x 4, 3 epochs": (4, 4, 1000, 64, 3, (0.05, 0.2)), "500 x 20 x 4, 3 epochs": (20, 4, 500, 64, 3, (0.05, 0.2)),
          "200 x 61, 3 epochs": (61, 1, 200, 64, 3, (0.05, 0.2)), "makona 1610 x 56, 2 epochs": (56, 1, 1610, 1, 2, (0.03,))}


def source_hash():
    h = hashlib.sha256()
    for f in ("kernels_epoch.hip", "engine_epoch.cpp", "transition_body.h"):
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
    """BranchGradient's buffer plan and post-order list over the branch matrices of an epoch model formed by `route`."""

    def __init__(self, wl, systems, times, route, library=None):
        wl = copy.copy(wl)
        wl.eig = systems[0]
        super().__init__(wl, library=library, eigen_count=len(systems), extra_matrices=epochs.POOL_SIZE_DEFAULT + 1)
        for k, e in enumerate(systems):
            self.b.setEigenDecomposition(k, e.evec, e.ievc, e.evals)
        self.route = route
        self.etm = epochs.EpochTransitionMatrices(epochs.EpochBranchModel(times, len(systems)), self.tree, self.extra_index)

    def matrices(self):
        self.etm.update(self.b, self._nodes, self.branch_lengths[self._nodes], route=self.route)

    def log_likelihood(self):
        self.matrices()
        self.b.updatePartials(self._post_ops, len(self._post_ops) // 7, NONE)
        out = [0.0]
        self.b.calculateRootLogLikelihoods([self.post_index(self.tree.root)], [0], [0], [NONE], 1, out)
        return out[0]


def plan(name, route, library=None):
    S, categories, taxa, patterns, models, quantiles = SHAPES[name]
    wl = helpers.random_workload(taxa, patterns, S, categories, seed=600 + S)
    rng = np.random.default_rng(700 + S)
    systems = []
    for _ in range(models):
        if S == 4:
            systems.append(substmodel.gtr(rng.gamma(2.0, 1.0, size=6) + 0.1, rng.dirichlet(np.full(4, 10.0))))
        else:
            systems.append(substmodel.random_reversible(S, rng)[0])
    times = [float(t) for t in np.quantile(wl.tree.height[wl.tree.tip_count:], quantiles)]
    return Evaluation(wl, systems, times, route, library)


def run(ev):
    ev.matrices()
    ev.b.synchronize()


def trace_calls(shapes, reps):
    """Per shape a phase of `reps` + 1 device calls and a phase of as many host-route updates, idle time between the phases: what
    --kernel-trace reads."""
    for name in shapes:
        for route in ("device", "host"):
            ev = plan(name, route)
            ev.b.synchronize()
            time.sleep(PHASE_GAP_S)
            for _ in range(reps + 1):
                run(ev)
            time.sleep(PHASE_GAP_S)
            ev.close()


def kernel_times(directory, shapes, reps):
    """-> {shape: {"device_route": us, "host_route": us}}: the summed time of the route's matrix kernels per call (k_epoch*; k_transition*
    and k_convolve), the mean over the phase's calls, from the per-dispatch trace of a --trace-calls run.  Phases are the runs of such
    dispatches with no gap of PHASE_GAP_S / 2 between them, in the order --trace-calls issues them."""
    files = glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        raise SystemExit("no *kernel_trace.csv under %s" % directory)
    rows = []
    for f in files:
        with open(f) as fh:
            for row in csv.DictReader(fh):
                kind = "device" if "k_epoch" in row["Kernel_Name"] else \
                    "host" if ("k_transition" in row["Kernel_Name"] or "k_convolve" in row["Kernel_Name"]) else None
                if kind:
                    rows.append((int(row["Start_Timestamp"]), int(row["End_Timestamp"]), kind))
    rows.sort()
    phases = []
    for start, end, kind in rows:
        if not phases or start - phases[-1]["end"] > PHASE_GAP_S / 2 * 1e9:
            phases.append({"kinds": set(), "ns": 0, "end": end, "dispatches": 0})
        p = phases[-1]
        p["kinds"].add(kind); p["ns"] += end - start; p["end"] = max(p["end"], end); p["dispatches"] += 1
    if len(phases) != 2 * len(shapes) or any(p["kinds"] != {("device", "host")[i % 2]} for i, p in enumerate(phases)):
        raise SystemExit("the trace does not hold a device and a host phase per shape: %s" % [(sorted(p["kinds"]), p["dispatches"]) for p in phases])
    out = {}
    for i, name in enumerate(shapes):
        d, h = phases[2 * i], phases[2 * i + 1]
        out[name] = {"device_route": round(d["ns"] / (reps + 1) / 1e3, 2), "device_route_dispatches_per_call": d["dispatches"] / (reps + 1),
                     "host_route": round(h["ns"] / (reps + 1) / 1e3, 2), "host_route_dispatches_per_call": h["dispatches"] / (reps + 1)}
    return out


def measure(name, reps):
    S, categories, taxa, patterns, models, _ = SHAPES[name]
    dev, host = plan(name, "device"), plan(name, "host")
    n = len(dev._nodes)
    segments = [len(dev.etm.branch_mapping(b)[0]) for b in dev._nodes]
    run(dev); run(host)
    slots = dev._edge_matrix[0][:16]
    m_dev = np.stack([dev.b.getTransitionMatrix(int(s)) for s in slots])
    m_host = np.stack([host.b.getTransitionMatrix(int(s)) for s in slots])
    call = timed(lambda: run(dev), reps)
    route = timed(lambda: run(host), reps)
    # the same lists with the Python in front of the natives taken out of the clock: the packed arguments of the one call, prepared once
    offsets, eig, seg = dev.etm.segments([int(b) for b in dev._nodes], [float(t) for t in dev.branch_lengths[dev._nodes]])
    packed = (np.asarray(offsets, dtype=np.int32), np.asarray(eig, dtype=np.int32), np.asarray(seg), np.asarray(dev._edge_matrix[0], dtype=np.int32))

    def native_only():
        dev.b.updateTransitionMatricesWithEpochs(packed[0], packed[1], packed[2], None, packed[3])
        dev.b.synchronize()

    native = timed(native_only, reps)
    for _ in range(2):
        ld, lh = dev.log_likelihood(), host.log_likelihood()
    ev_dev = timed(dev.log_likelihood, reps)
    ev_host = timed(host.log_likelihood, reps)
    out = {"states": S, "categories": categories, "branches": n, "models": models, "patterns": patterns, "reps": reps,
           "branches_by_segments": {str(k): segments.count(k) for k in sorted(set(segments))},
           "device_call_ms": median_ms(call), "device_native_call_only_ms": median_ms(native),
           "host_route_ms": median_ms(route), "host_route_native_calls": host.etm.native_calls, "host_route_flushes": dict(host.etm.flushes),
           "speedup_vs_host_route": round(float(np.median(route)) / float(np.median(call)), 2),
           "max_abs_difference_of_routes_first_16_branches": float(np.max(np.abs(m_dev - m_host))),
           "evaluation_device_route_ms": median_ms(ev_dev), "evaluation_host_route_ms": median_ms(ev_host),
           "evaluation_speedup": round(float(np.median(ev_host)) / float(np.median(ev_dev)), 2),
           "evaluation_routes_relative_difference": abs(ld - lh) / abs(lh)}
    dev.close(); host.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--trace-calls", action="store_true", help="only the two routes' updates (the program of a rocprofv3 --kernel-trace run)")
    ap.add_argument("--kernel-trace", help="directory of that run's csv output: kernel times join the record")
    ap.add_argument("--shapes", nargs="*", default=list(SHAPES))
    args = ap.parse_args()
    if args.trace_calls:
        trace_calls(args.shapes, args.reps)
        return
    out = {"source_hash": source_hash(), "goal_speedup": GOAL,
           "host_route": "epochs.EpochTransitionMatrices route='host': pool of 100 buffers, updateTransitionMatrices per eigen system + rounds of convolveTransitionMatrices (both routes include their Python)"}
    kernels = kernel_times(args.kernel_trace, args.shapes, args.reps) if args.kernel_trace else {}
    for name in args.shapes:
        out[name] = measure(name, args.reps)
        if name in kernels:
            out[name]["matrix_kernels_us_per_call"] = kernels[name]
    out["reaches_goal"] = {k: out[k]["speedup_vs_host_route"] >= GOAL for k in args.shapes}
    out["device_route_faster"] = {k: out[k]["speedup_vs_host_route"] > 1.0 for k in args.shapes}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
