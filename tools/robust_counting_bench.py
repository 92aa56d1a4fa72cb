#!/usr/bin/env python3
"""Codon robust counts in one device call (beagleMi355RobustCounts / beagleMi355SimulateUnconditionedCounts via
beast-mcmc_amd/robustcounting.py) against the way CodonPartitionedRobustCounting gets them through the BEAGLE interface
(src/dr/evomodel/substmodel/CodonPartitionedRobustCounting.java:216-307): three ancestral draws read back, then per branch and
labelling a Minin-Suchard table of the 64-state product chain and the per-site lookup on the host.  The host tables here are numpy
(batched BLAS matrix products over all branches at once, as many threads as numpy takes; not the ordered restatement of the tests,
which is slower), the gather numpy fancy indexing.

Three HKY positions over one tree, two registers (syn, non-syn), 1999 rows, at 1000 taxa x 10 000 codon sites and x 100 000.  Every
time is a whole call, which ends in a synchronising copy, after a warm-up call; the median of several.  Prints one JSON line
(profiles/robust_counting_bench.json).  ``--trace``: a few calls at each size, no host route, for a
``rocprofv3 --kernel-trace --stats`` run of its own."""
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
import bench                                              # noqa: E402
from beast_mcmc_amd.inputs import substmodel, synth       # noqa: E402
from beast_mcmc_amd.robustcounting import CodonPartitionedRobustCounting     # noqa: E402
from beast_mcmc_amd.treelikelihood import BeagleTreeLikelihood, RESCALE_DYNAMIC   # noqa: E402


def source_hash():
    h = hashlib.sha256()
    for f in ("kernels_robustcounts.hip", "engine_robustcounts.cpp", "kernels_ancestral.hip", "engine_sampling.cpp"):
        with open(os.path.join(ROOT, "beast-mcmc_amd", "csrc", f), "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


def median_ms(ts):
    return round(1e3 * float(np.median(ts)), 3)


def timed(f, reps):
    f(0)                                                  # warm-up: scratch allocation, code objects
    ts = []
    for k in range(reps):
        t0 = time.perf_counter()
        f(k + 1)
        ts.append(time.perf_counter() - t0)
    return ts


def host_tables(U, Ui, lam, Q, registers, taus):
    """Cond [K][n][64][64] by batched numpy products (row 0: 0)."""
    taus = np.asarray(taus)[1:]
    e = np.exp(lam[None, :] * taus[:, None])
    d = lam[:, None] - lam[None, :]
    tie = np.abs(d) < 1e-7
    with np.errstate(divide="ignore", invalid="ignore"):
        A = np.where(tie, e[:, :, None] * taus[:, None, None], (e[:, :, None] - e[:, None, :]) / np.where(tie, 1.0, d))
    P = np.abs(U @ (e[:, :, None] * Ui))
    out = np.zeros((len(registers), len(taus) + 1, 64, 64))
    for k, R in enumerate(registers):
        Rz = R.copy()
        np.fill_diagonal(Rz, 0.0)
        M = Ui @ ((Q * Rz) @ U)
        with np.errstate(divide="ignore", invalid="ignore"):
            out[k, 1:] = (U @ ((A * M) @ Ui)) / P
    return out


def measure(wl, reps, host_route=True):
    pi = np.full(4, 0.25)
    tls = []
    for q, (kappa, rate) in enumerate(((2.0, 0.7), (3.0, 0.5), (5.0, 1.8))):
        w = synth.Workload("codon-%d" % q, wl.tree, substmodel.hky(kappa, pi), pi, [rate], [1.0],
                           np.roll(wl.tip_states, 7919 * q, axis=1), np.ones(wl.pattern_count), 4)
        tl = BeagleTreeLikelihood(w, rescaling=RESCALE_DYNAMIC, delay_rescaling=False)
        tl.getLogLikelihood()
        tls.append(tl)
    rc = CodonPartitionedRobustCounting(*tls)
    rows, order = rc.node_lists()
    taus = rc.branch_lengths(order)
    U, Ui, lam, Q, freqs = rc.chain()
    others = [s.beagle for s in rc.samplers[1:]]
    n, P = len(order), wl.pattern_count

    def counts(seed, **kw):
        return rc.beagle.robustCounts(others, rows, taus, U, Ui, lam, Q, rc.registers, (seed, seed + 1, seed + 2), **kw)

    def draws(seed):
        return [s.beagle.sampleAncestralStates(rows[q], 0, 0, seed + q)[0] for q, s in enumerate(rc.samplers)]

    totals_only = timed(lambda k: counts(k), reps)
    with_counts = timed(lambda k: counts(k, counts=True), max(2, reps // 2))
    three_draws = timed(lambda k: draws(k), reps)
    two_rows = timed(lambda k: rc.beagle.robustCounts(others, rows[:, :2], taus[:2], U, Ui, lam, Q, rc.registers, (k, k, k)), reps)
    length = [rc.expected_tree_length()]
    uncond_site = timed(lambda k: rc.beagle.simulateUnconditionedCounts(Q, freqs, length, P, rc.registers, k, totals=False), reps)
    uncond_branch = timed(lambda k: rc.beagle.simulateUnconditionedCounts(Q, freqs, taus, P, rc.registers, k, totals=False),
                          max(2, reps // 2))
    uncond_branch_totals = timed(lambda k: rc.beagle.simulateUnconditionedCounts(Q, freqs, taus, P, rc.registers, k, counts=False), reps)
    out = {"taxa": wl.tip_count, "sites": P, "rows": int(n), "registers": int(len(rc.registers)), "reps": reps,
           "robustCounts_totals_only_ms": median_ms(totals_only), "robustCounts_with_outCounts_ms": median_ms(with_counts),
           "outCounts_bytes": int(len(rc.registers) * n * P * 8), "three_sampleAncestralStates_ms": median_ms(three_draws),
           "robustCounts_two_rows_ms": median_ms(two_rows),
           "unconditioned_per_site_ms": median_ms(uncond_site), "unconditioned_per_branch_ms": median_ms(uncond_branch),
           "unconditioned_per_branch_totals_only_ms": median_ms(uncond_branch_totals)}
    if host_route:
        seed = 12345
        res = counts(seed)
        t0 = time.perf_counter()
        st = np.stack(draws(seed)).astype(np.int64)
        t1 = time.perf_counter()
        cond = host_tables(U, Ui, lam, Q, rc.registers, taus)
        t2 = time.perf_counter()
        codon = st[0] * 16 + st[1] * 4 + st[2]
        site = np.zeros((len(rc.registers), P))
        branch = np.zeros((len(rc.registers), n))
        for r in range(1, n):
            v = cond[:, r, codon[rows[0][r, 2]], codon[r]]
            site += v
            branch[:, r] = v.sum(axis=1)
        t3 = time.perf_counter()
        scale = np.abs(branch).max()
        out.update({"host_route_ms": round(1e3 * (t3 - t0), 1), "host_route_three_draws_ms": round(1e3 * (t1 - t0), 1),
                    "host_route_tables_numpy_ms": round(1e3 * (t2 - t1), 1), "host_route_gather_numpy_ms": round(1e3 * (t3 - t2), 1),
                    "speedup_vs_host_route": round((t3 - t0) / float(np.median(totals_only)), 1),
                    "branch_totals_max_abs_difference_over_largest": float(np.abs(res["branch_totals"] - branch).max() / scale),
                    "site_totals_max_abs_difference": float(np.abs(res["site_totals"] - site).max())})
    for tl in tls:
        tl.close()
    return out


def main():
    cache = bench.workload_cache_file(bench.default_cache_dir(), "A", 1.0, "coalescent")
    a = bench.load_workload(cache, lambda: bm.synth.config_a(scale=1.0))
    if "--trace" in sys.argv:
        print(json.dumps({"1e4": measure(a.shard(0, 10000), reps=4, host_route=False), "1e5": measure(a, reps=2, host_route=False)}))
        return
    out = {"source_hash": source_hash(), "kernel_source_hash": bench.kernel_source_hash()}
    out["1e4"] = measure(a.shard(0, 10000), reps=7)
    out["1e5"] = measure(a, reps=5)
    out["goal_10x_vs_host_route_met"] = {k: out[k]["speedup_vs_host_route"] >= 10.0 for k in ("1e4", "1e5")}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
