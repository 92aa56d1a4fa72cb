#!/usr/bin/env python3
"""Reversible substitution models decomposed on the device in one call (beagleMi355SetReversibleModels via
beast-mcmc_amd/eigensystems.py) against the route SubstitutionModelDelegate.updateSubstitutionModels takes through the BEAGLE interface
(SubstitutionModelDelegate.java:272-288): a decomposition per model on the host — here numpy's symmetric eigensolver on the
pi-symmetrised Q, inputs.substmodel.decompose_reversible — and a setEigenDecomposition per model.

Shapes: 1 998 models x 4 states (a kappa per branch of a 1000-taxon tree), 998 x 20 (a random reversible model per branch, 500 taxa),
398 x 61 (a GY94 omega per branch, 200 taxa), and one model at each of these state counts.  Per shape: the device call (median wall
time of `--reps` calls, each waited for; its kernel time when `--kernel-trace DIR` names the output of a rocprofv3 --kernel-trace run
over `--trace-calls`), the host route split into the decompositions and the uploads (Q is formed outside the timed part), the sweeps
the device took and the restatement takes (tests/eigen_reference.py), the largest device-versus-host-route difference of P(0.3), and,
for the many-model shapes, a whole branch-specific evaluation on both routes.  Prints one JSON line
(profiles/eigen_decomposition_bench.json)."""
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
import eigen_reference as er                              # noqa: E402
from beast_mcmc_amd import eigensystems                   # noqa: E402

# name -> (states, models, kind of tests/eigen_reference.branch_model_plan, (taxa, patterns) of the whole evaluation)
SHAPES = {"1998 x 4": (4, 1998, "hky", (1000, 2000)), "998 x 20": (20, 998, "reversible20", (500, 500)),
          "398 x 61": (61, 398, "gy94", (200, 200)),
          "1 x 4": (4, 1, "hky", None), "1 x 20": (20, 1, "reversible20", None), "1 x 61": (61, 1, "gy94", None)}


def source_hash():
    h = hashlib.sha256()
    for f in ("kernels_eigen.hip", "engine_eigen.cpp"):
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


def model_set(S, count, kind):
    rng = np.random.default_rng(300 + S)
    models = eigensystems.SubstitutionModelSet(S, count, route="device")
    if kind == "hky":
        models.set_hky(rng.gamma(4.0, 0.6, size=count) + 0.2, rng.dirichlet(np.full(4, 10.0)))
    elif kind == "gy94":
        models.set_gy94(2.0, rng.gamma(2.0, 0.2, size=count) + 0.02, rng.dirichlet(np.full(61, 5.0)))
    else:
        for k in range(count):
            models.set_model(k, *er.random_model(S, rng))
    return models


def device_call(b, models):
    b.setReversibleModels(np.arange(models.count), models.rates, models.freqs)
    b.synchronize()


def trace_calls(reps):
    """Only the device calls, `reps` of each shape in the order of SHAPES after one warm-up call each: what --kernel-trace reads."""
    for name, (S, count, kind, _) in SHAPES.items():
        models = model_set(S, count, kind)
        b = bm.beagle.Beagle(2, 3, 2, S, 16, count, 8, 4, 0)
        for _ in range(reps + 1):
            device_call(b, models)
        b.finalize()


def kernel_times(directory, reps):
    """-> {shape: median kernel time in microseconds} from the per-dispatch trace of a --trace-calls run: the k_eigen* dispatches in
    order, reps + 1 per shape (the first is the warm-up)."""
    files = glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        raise SystemExit("no *kernel_trace.csv under %s" % directory)
    rows = []
    for f in files:
        with open(f) as fh:
            for row in csv.DictReader(fh):
                if "k_eigen" in row["Kernel_Name"]:
                    rows.append((int(row["Start_Timestamp"]), int(row["End_Timestamp"]) - int(row["Start_Timestamp"])))
    rows.sort()
    if len(rows) != (reps + 1) * len(SHAPES):
        raise SystemExit("%d k_eigen dispatches in the trace, expected %d" % (len(rows), (reps + 1) * len(SHAPES)))
    out = {}
    for k, name in enumerate(SHAPES):
        ns = [d for _, d in rows[k * (reps + 1) + 1:(k + 1) * (reps + 1)]]
        out[name] = round(float(np.median(ns)) / 1e3, 2)
    return out


def measure(name, reps):
    S, count, kind, tree = SHAPES[name]
    models = model_set(S, count, kind)
    b = bm.beagle.Beagle(2, 3, 2, S, 16, count, 8, 4, 0)
    b.setCategoryRates(er.CATEGORY_RATES)
    device_call(b, models)
    call = timed(lambda: device_call(b, models), reps)
    stats = b.eigenStats()
    dev_slots = [b.getEigenDecomposition(k) for k in range(min(count, 16))]
    # the host route, in its two parts (Q formed outside the timed part)
    decompose, uploads = [], []
    qs = []
    for k in range(count):
        r = np.zeros((S, S))
        r[np.triu_indices(S, 1)] = models.rates[k]
        q = (r + r.T) * models.freqs[k][None, :]
        np.fill_diagonal(q, -q.sum(axis=1))
        qs.append(q)
    for _ in range(max(1, reps // 3)):
        t0 = time.perf_counter()
        eigs = [bm.substmodel.decompose_reversible(q, pi) for q, pi in zip(qs, models.freqs)]
        t1 = time.perf_counter()
        for k, e in enumerate(eigs):
            b.setEigenDecomposition(k, e.evec, e.ievc, e.evals)
        b.synchronize()
        t2 = time.perf_counter()
        decompose.append(t1 - t0); uploads.append(t2 - t1)
    p_diff = 0.0
    for k, (u, ui, lam) in enumerate(dev_slots):
        p_dev = (u * np.exp(0.3 * lam)[None, :]) @ ui
        p_diff = max(p_diff, float(np.max(np.abs(p_dev - eigs[k].transition_probabilities(0.3)))))
    # what float64 leaves of the SMALL entries of P on a short branch, either route (model 0, dist 1e-3, against the longdouble yardstick)
    yard = er.yardstick_p(models.rates[0], models.freqs[0], 1e-3)
    u, ui, lam = dev_slots[0]
    rel_dev = float(np.max(np.abs((u * np.exp(1e-3 * lam)[None, :]) @ ui - yard) / yard))
    rel_host = float(np.max(np.abs(eigs[0].transition_probabilities(1e-3) - yard) / yard))
    sample = [er.decompose(models.rates[k], models.freqs[k]).sweeps for k in range(min(count, 8))]
    b.finalize()
    host_ms = 1e3 * (float(np.median(decompose)) + float(np.median(uploads)))
    out = {"states": S, "models": count, "reps": reps, "device_call_ms": median_ms(call),
           "input_MB": round(count * (S * (S - 1) // 2 + S) * 8 / 1e6, 3),
           "host_decompose_ms": median_ms(decompose), "host_setEigenDecomposition_ms": median_ms(uploads),
           "host_setEigenDecomposition_MB": round(count * (2 * S * S + S) * 8 / 1e6, 3), "host_route_ms": round(host_ms, 4),
           "speedup_vs_host_route": round(host_ms / (1e3 * float(np.median(call))), 2),
           "device_max_sweeps": stats["max_sweeps"], "device_capped_models": stats["capped"],
           "restatement_sweeps_first_models": sample, "max_abs_difference_of_P_0.3_from_host_route": p_diff,
           "max_relative_error_of_P_1e-3_device_route": rel_dev, "max_relative_error_of_P_1e-3_host_route": rel_host}
    if tree is not None:
        taxa, patterns = tree
        _, dev_models, dev = er.branch_model_plan(kind, None, "device", seed=200 + S, taxa=taxa, patterns=patterns)
        _, host_models, host = er.branch_model_plan(kind, None, "host", seed=200 + S, taxa=taxa, patterns=patterns)

        def evaluation(models_, plan):
            models_.dirty[:] = True
            return plan.log_likelihood()

        for _ in range(2):
            ld, lh = evaluation(dev_models, dev), evaluation(host_models, host)
        ev_dev = timed(lambda: evaluation(dev_models, dev), reps)
        ev_host = timed(lambda: evaluation(host_models, host), max(1, reps // 3))
        out.update({"evaluation_taxa": taxa, "evaluation_patterns": patterns,
                    "evaluation_device_route_ms": median_ms(ev_dev), "evaluation_host_route_ms": median_ms(ev_host),
                    "evaluation_speedup": round(float(np.median(ev_host)) / float(np.median(ev_dev)), 2),
                    "evaluation_routes_relative_difference": abs(ld - lh) / abs(lh)})
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
           "host_route": "inputs.substmodel.decompose_reversible (numpy.linalg.eigh) + one setEigenDecomposition per model, Q formed outside the timed part"}
    kernels = kernel_times(args.kernel_trace, args.reps) if args.kernel_trace else {}
    for name in args.shapes:
        out[name] = measure(name, args.reps)
        if name in kernels:
            out[name]["device_kernel_us"] = kernels[name]
    out["goal_10x_over_host_route_met"] = {k: out[k]["speedup_vs_host_route"] >= 10.0 for k in args.shapes if SHAPES[k][1] > 1}
    out["one_model_device_faster_than_host"] = {k: out[k]["speedup_vs_host_route"] > 1.0 for k in args.shapes if SHAPES[k][1] == 1}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
