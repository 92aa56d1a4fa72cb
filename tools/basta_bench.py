#!/usr/bin/env python3
"""One BASTA evaluation on the device (beast-mcmc_amd/basta.py: eigen system, sizes, matrices, update, accumulate, log-density on
the host) against a single-threaded C++ restatement of the same three functions (tools/basta_host_restatement.cpp, compiled here
with g++ -O3; the reference's generic delegate is single-threaded too) on the same operation list and the same matrices.

1000 tips sampled through time (seeded; population 30 sampling spans, so that hundreds of lineages coexist: 4e5 operations of 8
ints in 1998 intervals), 4, 20 and 61 demes.  Every device time is a whole evaluation, which ends in a synchronising copy of the
result, after a warm-up; the median of several.  The host time leaves the matrix exponentials out (it is handed the device's
matrices), which favours the host.  Per state count the JSON holds both times, their ratio, the kernel launches of the update
(beagleMi355KernelTimer), and the share of an evaluation spent sending the operation list: the time with a new list minus the
time with the list already on the device, over the former.  Prints one JSON line (profiles/basta_bench.json)."""
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np                                        # noqa: E402
import beast_mcmc_amd as bm                               # noqa: E402
from beast_mcmc_amd import basta                          # noqa: E402
from beast_mcmc_amd.inputs import substmodel, trees       # noqa: E402

TIPS = 1000


def host_library(tmp):
    out = os.path.join(tmp, "libbasta_host_restatement.so")
    subprocess.check_call(["g++", "-O3", "-std=c++17", "-fPIC", "-shared", os.path.join(ROOT, "tools", "basta_host_restatement.cpp"), "-o", out])
    lib = C.CDLL(out)
    I, D = C.POINTER(C.c_int), C.POINTER(C.c_double)
    lib.basta_evaluate.argtypes = [C.c_int, I, I, C.c_int, D, D, D, D, D, C.c_int]
    lib.basta_evaluate.restype = C.c_double
    return lib


def median_ms(ts):
    return round(1e3 * float(np.median(ts)), 3)


def measure(state_count, host, reps):
    rng = np.random.default_rng(state_count)
    tree = trees.heterochronous_coalescent_tree(TIPS, np.random.default_rng(1), sampling_span=1.0, population=30.0)
    other = trees.heterochronous_coalescent_tree(TIPS, np.random.default_rng(2), sampling_span=1.0, population=30.0)
    eig, _ = substmodel.random_reversible(state_count, rng)
    sizes = rng.gamma(4.0, 0.5, size=state_count) + 0.05
    demes = rng.integers(0, state_count, size=TIPS)
    like = basta.BastaLikelihood(tree, demes, basta.transpose_eigen(eig), sizes, rate=0.5)
    value = like.log_likelihood()                         # warm-up: the resize, code objects, staging buffers
    tr = like.traversal
    same = []
    for _ in range(reps):
        t0 = time.perf_counter()
        like.log_likelihood()
        same.append(time.perf_counter() - t0)
    # a new list with every evaluation: two trees in turn (the traversals are made outside the timed region)
    lists = [tr, basta.traverse(other, 0.5, 1)]
    fresh = []
    for k in range(2 * reps):
        like.traversal = lists[(k + 1) % 2]
        t0 = time.perf_counter()
        like.log_likelihood()
        fresh.append(time.perf_counter() - t0)
    like.traversal = tr
    assert like.log_likelihood() == value
    b = like.beagle
    b.kernelTimer(1)
    b.updateBastaPartials(tr.operations, len(tr.operations), tr.intervals, len(tr.intervals), 0, 0)
    update_ms, launches = b.kernelTimer(0)
    # the host restatement on the device's own matrices
    n_matrices = max(m for m, _ in tr.matrices) + 1
    matrices = np.zeros((n_matrices, state_count, state_count))
    for m, _ in tr.matrices:
        matrices[m] = like.transition_matrix(m)
    I, D = C.POINTER(C.c_int), C.POINTER(C.c_double)
    partials = np.zeros((tr.buffer_count, state_count))
    partials[:TIPS] = like.tips
    coalescent = np.zeros(tr.interval_count)
    ops, iv, ln = np.ascontiguousarray(tr.operations), np.ascontiguousarray(tr.intervals), np.ascontiguousarray(tr.lengths)
    host_times = []
    for _ in range(max(2, reps // 2)):
        t0 = time.perf_counter()
        host_value = host.basta_evaluate(state_count, ops.ctypes.data_as(I), iv.ctypes.data_as(I), len(iv), ln.ctypes.data_as(D),
                                         matrices.ctypes.data_as(D), sizes.ctypes.data_as(D), partials.ctypes.data_as(D),
                                         coalescent.ctypes.data_as(D), tr.interval_count)
        host_times.append(time.perf_counter() - t0)
    like.close()
    dev_new, dev_same, host_ms = median_ms(fresh), median_ms(same), median_ms(host_times)
    return {"demes": state_count, "tips": TIPS, "operations": int(len(tr.operations)), "intervals": int(len(tr.intervals) - 1),
            "operation_list_bytes": int(tr.operations.nbytes), "reps": reps,
            "device_evaluation_ms": dev_new, "device_evaluation_list_resident_ms": dev_same,
            "host_restatement_ms": host_ms, "host_over_device": round(host_ms / dev_new, 1),
            "update_kernel_ms": round(update_ms, 3), "update_launches": int(launches),
            "operation_list_upload_share": round(max(0.0, dev_new - dev_same) / dev_new, 3),
            "log_likelihood": value, "host_log_likelihood": host_value,
            "relative_difference": abs(value - host_value) / abs(host_value)}


def main():
    with tempfile.TemporaryDirectory() as tmp:
        host = host_library(tmp)
        out = {"note": "device: whole evaluations (matrices + update + accumulate, result on the host); host: single-threaded C++ "
                       "restatement without the matrix exponentials; times are medians"}
        for s in (4, 20, 61):
            out["S%d" % s] = measure(s, host, reps=5)
        print(json.dumps(out))


if __name__ == "__main__":
    main()
