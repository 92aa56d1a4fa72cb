#!/usr/bin/env python3
"""Substitution-parameter differential matrices of every branch in one call (beagleMi355UpdateDifferentialMatrices via
beast-mcmc_amd/substgradient.py) against the route BranchSubstitutionParameterDelegate.cacheDifferentialMassMatrix takes through the
BEAGLE interface (BranchSubstitutionParameterDelegate.java:62-81): a getExactDifferentialMassMatrix per branch and category on the
host — here the numpy restatement of substgradient.py, the one the GPU tests compare with — and a setDifferentialMatrix per branch.

Cases: 1000 taxa x 4 categories x 4 states (HKY kappa), 500 x 4 x 20 (one exchangeability of a reversible model), 200 x 4 x 61
(GY94 omega); one parameter, every branch under one model.  Per case: the device call alone (median wall time of `--reps` calls, each
waited for), its first-order form (the same stores without the products) and a one-branch call (the launch floor); the host route
split into forming the matrices and the uploads; a whole gradient both ways; and the largest float64-versus-longdouble error of the
restatement and device-versus-restatement error over a sample of branches.  "accuracy_by_state_count": the same two errors, the
largest per state count over the shape table of tests/test_gpu_differential_matrices.py.  Prints one JSON line
(profiles/differential_matrices_bench.json)."""
import argparse
import contextlib
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np                                        # noqa: E402
import helpers                                            # noqa: E402
from beast_mcmc_amd import substgradient as sg            # noqa: E402

CASES = {4: (1000, 2000), 20: (500, 500), 61: (200, 200)}      # states -> (taxa, patterns)


def source_hash():
    h = hashlib.sha256()
    for f in ("kernels_differential.hip", "engine_differential.cpp"):
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


def model_for(S, wl):
    if S == 4:
        return sg.hky_kappa(2.3, wl.freqs)
    if S == 61:
        return sg.gy94_omega(2.0, 0.4, np.random.default_rng(0).dirichlet(np.full(61, 5.0)))
    rng = np.random.default_rng(S)
    return sg.reversible_rate(rng.gamma(1.0, 1.0, size=S * (S - 1) // 2) + 0.05, wl.freqs, [10])


def measure(S, reps):
    taxa, patterns = CASES[S]
    wl = helpers.random_workload(taxa, patterns, S, 4, seed=200 + S)
    model = model_for(S, wl)
    dev = sg.SubstitutionParameterGradient(wl, [model], route="device")
    host = sg.SubstitutionParameterGradient(wl, [model], route="host")
    n = len(dev._nodes)
    for g in (dev, host):
        for _ in range(2):
            g.gradient()

    def device_call(mode=sg.EXACT, count=n):
        dev.b.updateDifferentialMatrices(None, None, model.dq[:1], None, dev._d_idx[:count], dev.branch_lengths[dev._nodes[:count]], count, mode)
        dev.b.synchronize()

    device_call()
    call = timed(device_call, reps)
    first_order = timed(lambda: device_call(sg.FIRST_ORDER), reps)
    one_branch = timed(lambda: device_call(count=1), reps)
    # the host route, in its two parts
    form, uploads = [], []
    for _ in range(max(1, reps // 3)):
        t0 = time.perf_counter()
        mats = host.host_matrices(0)
        t1 = time.perf_counter()
        for slot, m in zip(host._d_idx, mats):
            host.b.setDifferentialMatrix(int(slot), m)
        host.b.synchronize()
        t2 = time.perf_counter()
        form.append(t1 - t0); uploads.append(t2 - t1)
    grad_dev = timed(lambda: dev.gradient(), reps)
    grad_host = timed(lambda: host.gradient(), max(1, reps // 3))
    _, gd = dev.gradient()
    _, gh = host.gradient()
    # accuracy over a sample of branches: the shortest, the longest and 14 spread between them
    order = np.argsort(dev.branch_lengths[dev._nodes])
    sample = order[np.unique(np.linspace(0, n - 1, 16).astype(int))]
    device_call()
    e_ref = e_dev = 0.0
    rates = np.asarray(wl.cat_rates)
    for e in sample:
        got = dev.b.getTransitionMatrix(int(dev._d_idx[e]))
        for c, r in enumerate(rates):
            dist = dev.branch_lengths[dev._nodes[e]] * r
            d64 = sg.exact(model.eig.evec, model.eig.ievc, model.eig.evals, model.dq[0], dist)[0]
            dld = sg.exact(model.eig.evec, model.eig.ievc, model.eig.evals, model.dq[0], dist, dtype=np.longdouble)[0]
            e_ref = max(e_ref, float(np.max(np.abs(d64 - dld)) / np.max(np.abs(dld))))
            e_dev = max(e_dev, float(np.max(np.abs(got[c] - d64)) / np.max(np.abs(d64))))
    matrices = n * 4
    host_ms = 1e3 * (float(np.median(form)) + float(np.median(uploads)))
    out = {"taxa": taxa, "patterns": patterns, "categories": 4, "states": S, "branches": n, "matrices": matrices, "reps": reps,
           "device_call_ms": median_ms(call), "device_call_first_order_ms": median_ms(first_order),
           "device_call_one_branch_ms": median_ms(one_branch),
           "stored_MB": round(matrices * S * S * 8 / 1e6, 2),
           "product_GFLOP": round(2 * 2 * S ** 3 * matrices / 1e9, 3),
           "product_GFLOPs_wall": round(2 * 2 * S ** 3 * matrices / float(np.median(call)) / 1e9, 1),
           "host_form_ms": median_ms(form), "host_setDifferentialMatrix_ms": median_ms(uploads),
           "host_setDifferentialMatrix_calls": n, "host_route_ms": round(host_ms, 3),
           "speedup_vs_host_route": round(host_ms / (1e3 * float(np.median(call))), 1),
           "gradient_device_route_ms": median_ms(grad_dev), "gradient_host_route_ms": median_ms(grad_host),
           "gradient_speedup": round(float(np.median(grad_host)) / float(np.median(grad_dev)), 1),
           "gradient_routes_relative_difference": float(np.max(np.abs(gd - gh)) / max(1.0, float(np.max(np.abs(gh))))),
           "e_ref_float64_vs_longdouble": e_ref, "device_error_vs_restatement": e_dev,
           "device_error_bound_8_max_eref_S_eps": 8 * max(e_ref, S * float(np.finfo(float).eps))}
    dev.close(); host.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--states", type=int, nargs="*", default=[4, 20, 61])
    args = ap.parse_args()
    out = {"source_hash": source_hash(), "host_route": "numpy restatement (substgradient.exact) + one setDifferentialMatrix per branch"}
    for S in args.states:
        out["%d states" % S] = measure(S, args.reps)
    import test_gpu_differential_matrices as shapes       # (the tests' shape table and check; its progress lines go to stderr)
    with contextlib.redirect_stdout(sys.stderr):
        errors = {S: shapes.shape_table_errors(S) for S in shapes.STATES}
    out["accuracy_by_state_count"] = {str(S): {"device_error_vs_restatement": e[0], "e_ref_float64_vs_longdouble": e[1]} for S, e in errors.items()}
    out["goal_10x_over_host_route_met"] = {k: v["speedup_vs_host_route"] >= 10.0 for k, v in out.items() if k.endswith(" states")}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
