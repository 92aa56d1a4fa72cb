#!/usr/bin/env python3
"""One simulated alignment on the device (beagleMi355SimulateSequences via beast-mcmc_amd/simulate.py) against the same replicate
done the way dr.app.beagle.tools.Partition.traverse does it through the BEAGLE interface (src/dr/app/beagle/tools/Partition.java:
292-431): getTransitionMatrix per branch, then every site's draw on the host (numpy: tests/simulate_reference.py, the restatement
the GPU tests compare against — so this run also checks the device's states against it), the two parts timed separately; and
against beagleMi355SampleAncestralStates over the same rows x sites (an instance whose alignment is the simulated one).

GTR+G4 at 1000 taxa x 1e4 and x 1e5 sites, and the 20- and 61-state models at the sizes of configs B and C.  Device times are whole
calls, the copy of the states to the host included: tips only (what a replicate is) and every node (what the ancestral draw
returns).  Prints one JSON line (profiles/simulate_bench.json)."""
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np                                        # noqa: E402
import simulate_reference as sr                           # noqa: E402
from beast_mcmc_amd.ancestral import AncestralStateSampler                   # noqa: E402
from beast_mcmc_amd.inputs import substmodel, synth       # noqa: E402
from beast_mcmc_amd.simulate import SequenceSimulator     # noqa: E402
from beast_mcmc_amd.treelikelihood import BeagleTreeLikelihood, RESCALE_DYNAMIC   # noqa: E402


def source_hash():
    h = hashlib.sha256()
    for f in ("kernels_simulate.hip", "engine_simulate.cpp"):
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
    """(name, taxa, sites, eigen system, frequencies): the trees and models of configs A, B and C over a token alignment."""
    pi = np.array([0.30, 0.20, 0.22, 0.28])
    gtr = substmodel.gtr([1.0, 4.0, 0.8, 1.2, 4.5, 1.0], pi)
    aa, aa_pi = substmodel.random_reversible(20, np.random.default_rng(111))
    rng = np.random.default_rng(121)
    codon, codon_pi = substmodel.gy94(2.0, 0.2, rng.dirichlet(np.full(61, 20.0)))
    return [("GTR+G4 1000x1e4", 1000, 10000, gtr, pi, 1), ("GTR+G4 1000x1e5", 1000, 100000, gtr, pi, 1),
            ("AA20+G4 500x5e4", 500, 50000, aa, aa_pi, 11), ("GY94+G4 200x2e4", 200, 20000, codon, codon_pi, 21)]


def measure(name, taxa, sites, eig, pi, seed, reps):
    wl = synth.make_workload(name, taxa, 64, eig, pi, seed=seed)
    tl = BeagleTreeLikelihood(wl, rescaling=RESCALE_DYNAMIC, delay_rescaling=False)
    tl.getLogLikelihood()                                 # (updateTransitionMatrices for every branch)
    sim = SequenceSimulator(tl)
    raw = sim.beagle
    sim.simulate(sites, 0, ancestral=True)                # first call: scratch allocation
    (tips, _, cats), t_tips = timed(lambda k: sim.simulate(sites, 100 + k), reps)
    (_, internal, _), t_all = timed(lambda k: sim.simulate(sites, 100 + reps - 1 if k == reps - 1 else 200 + k, ancestral=True), reps)
    # the reference's route, with the seed of the last calls: the same matrices, so the same states
    rows, order = sim.node_list(True)
    t_mat, mats = [0.0], {}

    def matrix_of(m):
        if m not in mats:
            t0 = time.perf_counter()
            mats[m] = raw.getTransitionMatrix(m)
            t_mat[0] += time.perf_counter() - t0
        return mats[m]

    t0 = time.perf_counter()
    ref, ref_cats, bad = sr.simulate(rows, matrix_of, wl.cat_weights, wl.freqs, 100 + reps - 1, sites)
    t_ref = time.perf_counter() - t0
    got = np.vstack([tips, internal])
    identical = bool(np.array_equal(got[order], ref) and np.array_equal(cats, ref_cats) and not bad)
    tl.close()
    # the ancestral draw over the same rows x sites: the simulated alignment as a new instance's data
    anc = BeagleTreeLikelihood(tree=wl.tree, tip_states=tips.astype(np.int32), weights=np.ones(sites), eig=eig, freqs=pi,
                               cat_rates=wl.cat_rates, cat_weights=wl.cat_weights, state_count=len(pi), rescaling=RESCALE_DYNAMIC,
                               delay_rescaling=False)
    anc.getLogLikelihood()
    sampler = AncestralStateSampler(anc)
    sampler.sample(0)                                     # scratch allocation, virtual buffers materialised
    _, t_anc = timed(lambda k: sampler.sample(300 + k), reps)
    anc.close()
    dev = float(np.median(t_tips))
    return {"name": name, "taxa": taxa, "sites": sites, "states": len(pi), "categories": wl.category_count, "rows": int(len(rows)),
            "reps": reps, "device_tips_only_ms": median_ms(t_tips), "device_all_nodes_ms": median_ms(t_all),
            "reference_route_ms": round(1e3 * t_ref, 1), "reference_getTransitionMatrix_ms": round(1e3 * t_mat[0], 1),
            "reference_host_draws_ms": round(1e3 * (t_ref - t_mat[0]), 1),
            "speedup_vs_reference_route": round(t_ref / dev, 1),
            "speedup_vs_getTransitionMatrix_part_alone": round(t_mat[0] / dev, 2),
            "ancestral_draw_all_nodes_ms": median_ms(t_anc),
            "all_nodes_vs_ancestral_draw": round(float(np.median(t_anc)) / float(np.median(t_all)), 2),
            "states_identical_to_restatement": identical}


def main():
    out = {"simulate_source_hash": source_hash(), "cases": []}
    for name, taxa, sites, eig, pi, seed in models():
        out["cases"].append(measure(name, taxa, sites, eig, pi, seed, reps=5))
    out["goal_10x_reference_route_met"] = all(c["speedup_vs_reference_route"] >= 10.0 for c in out["cases"])
    out["not_slower_than_ancestral_draw"] = all(c["all_nodes_vs_ancestral_draw"] >= 1.0 for c in out["cases"])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
