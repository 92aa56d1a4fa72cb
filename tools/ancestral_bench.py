#!/usr/bin/env python3
"""One ancestral-state draw on the device (beagleMi355SampleAncestralStates via beast-mcmc_amd/ancestral.py) against the same
draw done the way AncestralStateBeagleTreeLikelihood.traverseSample does it through the BEAGLE interface
(src/dr/evomodel/treelikelihood/AncestralStateBeagleTreeLikelihood.java:414-625): getPartials per internal node,
getTransitionMatrix per branch, then the draw on the host (numpy: tests/ancestral_reference.py, the restatement the GPU tests
compare against — so this run also checks the device's states against it).

At A/10 (1000 taxa x 10 000 patterns) and A (1000 x 1e5), GTR+G4.  Device draw: right after an evaluation (virtual buffers
still definitions: the draw materialises them) and again with nothing left to materialise; both include the host copy of the
[nodes][P] states.  Prints one JSON line (profiles/ancestral_bench.json)."""
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np                                        # noqa: E402
import ancestral_reference as ar                          # noqa: E402
import beast_mcmc_amd as bm                               # noqa: E402
import bench                                              # noqa: E402
from beast_mcmc_amd.ancestral import AncestralStateSampler                   # noqa: E402
from beast_mcmc_amd.treelikelihood import BeagleTreeLikelihood, RESCALE_DYNAMIC   # noqa: E402


def sampler_source_hash():
    h = hashlib.sha256()
    for f in ("kernels_ancestral.hip", "engine_sampling.cpp"):
        with open(os.path.join(ROOT, "beast-mcmc_amd", "csrc", f), "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


def median_ms(ts):
    return round(1e3 * float(np.median(ts)), 3)


def measure(wl, reps):
    tl = BeagleTreeLikelihood(wl, rescaling=RESCALE_DYNAMIC, delay_rescaling=False)
    tl.getLogLikelihood()
    sampler = AncestralStateSampler(tl)
    raw = sampler.beagle
    sampler.sample(0)                                     # first call: scratch allocation
    fresh, again = [], []
    for k in range(reps):
        tl.makeDirty(); tl.getLogLikelihood()             # virtual buffers are definitions again
        t0 = time.perf_counter()
        states, cats = sampler.sample(100 + k)
        fresh.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        sampler.sample(200 + k)
        again.append(time.perf_counter() - t0)
    # the reference's way, with the seed of the last fresh draw: same partials, so the same states
    seed = 100 + reps - 1
    rows, order = sampler.node_list()
    compact = set(range(wl.tip_count))
    t_part, t_mat = [0.0], [0.0]
    mats = {}

    def partials_of(b):
        t0 = time.perf_counter()
        v = raw.getPartials(b)
        t_part[0] += time.perf_counter() - t0
        return v

    def matrix_of(m):
        if m not in mats:
            t0 = time.perf_counter()
            mats[m] = raw.getTransitionMatrix(m).reshape(wl.category_count, 4, 4)
            t_mat[0] += time.perf_counter() - t0
        return mats[m]

    t0 = time.perf_counter()
    ref, ref_cats, bad = ar.sample(rows, partials_of, matrix_of, raw.getTipStates, lambda b: b in compact, wl.cat_weights, wl.freqs,
                                   seed)
    t_ref = time.perf_counter() - t0
    identical = bool(np.array_equal(states[order], ref) and np.array_equal(cats, ref_cats) and not bad)
    tl.close()
    return {"taxa": wl.tip_count, "patterns": wl.pattern_count, "categories": wl.category_count, "rows": int(len(rows)),
            "device_draw_ms": median_ms(fresh), "device_draw_no_materialise_ms": median_ms(again), "reps": reps,
            "readback_path_ms": round(1e3 * t_ref, 1), "readback_getPartials_ms": round(1e3 * t_part[0], 1),
            "readback_getTransitionMatrix_ms": round(1e3 * t_mat[0], 1),
            "readback_host_draw_ms": round(1e3 * (t_ref - t_part[0] - t_mat[0]), 1),
            "speedup_vs_readback_path": round(t_ref / float(np.median(fresh)), 1), "states_identical_to_restatement": identical}


def main():
    cache = bench.workload_cache_file(bench.default_cache_dir(), "A", 1.0, "coalescent")
    a = bench.load_workload(cache, lambda: bm.synth.config_a(scale=1.0))
    out = {"sampler_source_hash": sampler_source_hash(), "kernel_source_hash": bench.kernel_source_hash()}
    out["A/10"] = measure(a.shard(0, 10000), reps=5)
    out["A"] = measure(a, reps=3)
    out["goal_10x_at_A/10_met"] = out["A/10"]["speedup_vs_readback_path"] >= 10.0
    print(json.dumps(out))


if __name__ == "__main__":
    main()
