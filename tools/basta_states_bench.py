#!/usr/bin/env python3
"""beagleBastaSampleStates (a deme for every lineage at every sub-interval boundary, per replicate, in one call) at the BASTA
benchmark's size — 1000 tips sampled through time, 4e5 operations; 4, 20 and 61 demes — against the two ways of doing it on the
host.  Nothing here was measured before; no ratio is asserted.

Per deme count, after one evaluation (tools/basta_bench.py times that):
  device     replicateCount 1 and 1024, counts only (outOccupancy, outChanges) and with outStates: whole calls, the median of
             several after a warm-up; the kernel time and the launches of one call (beagleMi355KernelTimer); the share of the call
             with outStates that the copy-out adds (its time minus the counts-only time, over its time).
  read-back  the route the reference takes (BastaLikelihood.java:755-943): one getPartials per input vector and one
             getTransitionMatrix per matrix, timed in full, then the numpy restatement of the draw (tests/basta_states_reference.py),
             ONE replicate, timed on the last NUMPY_OPERATIONS operations of the list (the top of the tree) and scaled to the
             list's length — it is a Python loop over operations; the JSON says so.
  C++        a single-threaded restatement (tools/basta_states_host_restatement.cpp, g++ -O3 -ffp-contract=off) handed the device's
             vectors and matrices: one replicate in full (its states must be the device's bit for bit), and HOST_REPLICATES
             replicates scaled to 1024 (replicates are independent: the time is linear in them).
And the stated worst case of the launch count: a ladder of 1000 tips at 4 demes, tips - 1 launches.
Prints one JSON line (profiles/basta_states_bench.json)."""
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np                                        # noqa: E402
import basta_states_reference as sr                       # noqa: E402
from beast_mcmc_amd import basta                          # noqa: E402
from beast_mcmc_amd.inputs import substmodel, trees       # noqa: E402

TIPS = 1000
NUMPY_OPERATIONS = 4000
HOST_REPLICATES = 32
I, D = C.POINTER(C.c_int), C.POINTER(C.c_double)


def host_library(tmp):
    out = os.path.join(tmp, "libbasta_states_host_restatement.so")
    subprocess.check_call(["g++", "-O3", "-ffp-contract=off", "-std=c++17", "-fPIC", "-shared",
                           os.path.join(ROOT, "tools", "basta_states_host_restatement.cpp"), "-o", out])
    lib = C.CDLL(out)
    lib.basta_sample_states.argtypes = [C.c_int, I, C.c_int, I, C.c_int, D, C.c_int, D, D, C.c_int, C.c_ulonglong, C.c_int, C.c_void_p, D, D]
    lib.basta_sample_states.restype = C.c_int
    return lib


def ms(seconds):
    return round(1e3 * float(seconds), 3)


def timed(f, reps):
    f()                                                   # warm-up: scratch, code objects, the chains
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def device_case(like, frequencies, replicates, states, reps, seed=7):
    call = lambda: like.sample_states(replicates, seed, states=states, occupancy=True, changes=True, root_frequencies=frequencies)
    whole = timed(call, reps)
    b = like.beagle
    b.kernelTimer(1)
    call()
    kernel_ms, launches = b.kernelTimer(0)
    return whole, {"call_ms": ms(whole), "kernel_ms": round(kernel_ms, 3), "launches": int(launches), "chunks": int(b.bastaStatesStats()[2])}


def measure(state_count, host, reps):
    rng = np.random.default_rng(state_count)
    tree = trees.heterochronous_coalescent_tree(TIPS, np.random.default_rng(1), sampling_span=1.0, population=30.0)
    eig, _ = substmodel.random_reversible(state_count, rng)
    sizes = rng.gamma(4.0, 0.5, size=state_count) + 0.05
    frequencies = rng.dirichlet(np.full(state_count, 3.0))
    demes = rng.integers(0, state_count, size=TIPS)
    like = basta.BastaLikelihood(tree, demes, basta.transpose_eigen(eig), sizes, rate=0.5)
    like.log_likelihood()
    tr, b = like.traversal, like.beagle
    ops, iv = np.ascontiguousarray(tr.operations), np.ascontiguousarray(tr.intervals)
    n = len(ops)
    out = {"demes": state_count, "tips": TIPS, "operations": int(n), "intervals": int(len(iv) - 1), "reps": reps}
    for replicates in (1, 1024):
        counts_s, counts = device_case(like, frequencies, replicates, False, reps)
        states_s, with_states = device_case(like, frequencies, replicates, True, reps)
        with_states["copy_out_share"] = round(max(0.0, states_s - counts_s) / states_s, 3)
        out["device_R%d_counts" % replicates], out["device_R%d_states" % replicates] = counts, with_states
    out["chains"] = int(b.bastaStatesStats()[3])
    # the read-back route: every input vector and every matrix through the API, then numpy
    buffers = b.bastaStats()[3]
    vectors = np.zeros((buffers, state_count))
    inputs = np.unique(np.concatenate([ops[:, 1], ops[ops[:, 3] >= 0, 3], ops[-1:, 0]]))
    t0 = time.perf_counter()
    for i in inputs:
        vectors[i] = b.getPartials(int(i)).reshape(state_count)
    n_matrices = max(m for m, _ in tr.matrices) + 1
    matrices = np.zeros((n_matrices, state_count, state_count))
    for m, _ in tr.matrices:
        matrices[m] = like.transition_matrix(m)
    read_s = time.perf_counter() - t0
    top = ops[n - NUMPY_OPERATIONS:]
    top_iv = np.concatenate([[0], iv[iv > n - NUMPY_OPERATIONS] - (n - NUMPY_OPERATIONS)])
    t0 = time.perf_counter()
    sr.sample(top, top_iv, vectors, lambda m: matrices[m], frequencies, 1, 7)
    numpy_s = (time.perf_counter() - t0) * n / NUMPY_OPERATIONS
    out["read_back_R1"] = {"reads": int(len(inputs) + len(tr.matrices)), "read_ms": ms(read_s), "numpy_draw_ms": ms(numpy_s),
                           "numpy_draw_scaled_from_operations": NUMPY_OPERATIONS, "total_ms": ms(read_s + numpy_s)}
    # the C++ restatement on the device's vectors (those the list does not read stay zero: it never looks at them)
    for i in np.setdiff1d(np.unique(ops[:, 0]), inputs):
        vectors[i] = b.getPartials(int(i)).reshape(state_count)

    def run_host(replicates, states):
        got = np.zeros((replicates, buffers), dtype=np.uint8) if states else None
        occupancy, changes = np.zeros((len(iv) - 1, state_count)), np.zeros((state_count, state_count))
        t0 = time.perf_counter()
        host.basta_sample_states(state_count, ops.ctypes.data_as(I), n, iv.ctypes.data_as(I), len(iv), vectors.ctypes.data_as(D), buffers,
                                 matrices.ctypes.data_as(D), frequencies.ctypes.data_as(D), replicates, 7, 0,
                                 got.ctypes.data if states else None, occupancy.ctypes.data_as(D), changes.ctypes.data_as(D))
        return time.perf_counter() - t0, got, occupancy, changes

    one_s, host_states, host_occupancy, host_changes = run_host(1, True)
    device = like.sample_states(1, 7, occupancy=True, changes=True, root_frequencies=frequencies)
    out["host_states_equal_device"] = bool(np.array_equal(device["states"], host_states) and np.array_equal(device["occupancy"], host_occupancy)
                                           and np.array_equal(device["changes"], host_changes))
    many_s = run_host(HOST_REPLICATES, False)[0] * 1024 / HOST_REPLICATES
    out["cpp_R1_ms"], out["cpp_R1024_ms"], out["cpp_R1024_scaled_from_replicates"] = ms(one_s), ms(many_s), HOST_REPLICATES
    for replicates, host_s in ((1, one_s), (1024, many_s)):
        out["cpp_over_device_R%d_states" % replicates] = round(1e3 * host_s / out["device_R%d_states" % replicates]["call_ms"], 2)
    out["read_back_over_device_R1_states"] = round(out["read_back_R1"]["total_ms"] / out["device_R1_states"]["call_ms"], 1)
    like.close()
    return out


def ladder(reps):
    rng = np.random.default_rng(4)
    tree = trees.caterpillar_tree(TIPS, root_height=2.0)
    eig, _ = substmodel.random_reversible(4, rng)
    like = basta.BastaLikelihood(tree, rng.integers(0, 4, size=TIPS), basta.transpose_eigen(eig), rng.gamma(4.0, 0.5, size=4) + 0.05, rate=0.5)
    like.log_likelihood()
    out = {"demes": 4, "tips": TIPS, "operations": int(len(like.traversal.operations))}
    for replicates in (1, 1024):
        out["device_R%d_counts" % replicates] = device_case(like, None, replicates, False, reps)[1]
    like.close()
    return out


def main():
    with tempfile.TemporaryDirectory() as tmp:
        host = host_library(tmp)
        out = {"note": "device: whole beagleBastaSampleStates calls, medians; read-back: getPartials per input vector + numpy draw of ONE "
                       "replicate (draw time scaled from the top of the list); C++: single-threaded restatement on the device's vectors "
                       "(1024 replicates scaled from %d)" % HOST_REPLICATES}
        for s in (4, 20, 61):
            out["S%d" % s] = measure(s, host, reps=5)
        out["ladder"] = ladder(reps=3)
        print(json.dumps(out))


if __name__ == "__main__":
    main()
