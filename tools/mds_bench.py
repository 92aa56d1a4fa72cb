#!/usr/bin/env python3
"""Multidimensional scaling on the device (beast-mcmc_amd/mds.py over libmds2_jni.so) against a single-threaded C++ restatement
of the same work (tools/mds_host_restatement.cpp, compiled here with g++ -O3; the reference's Java core is single-threaded too).

For N in {1000, 10 000, 20 000}, D in {2, 6}, untruncated and left-truncated, medians after a warm-up of
  (a) a full evaluation: makeDirty + getSumOfIncrements, which ends in the synchronising read of the sum;
  (b) a single-location step: updateLocations(k) + getSumOfIncrements (the row path, one launch), accepted;
  (c) a gradient: getLocationGradient, N * D doubles back on the host;
next to each the host restatement's time for the same call and the ratio, and the design bytes (4 N^2 for the triangle, 8 N^2 for
the gradient) over the device's wall time.  Kernel times are not in here: they come from a ``rocprofv3 --kernel-trace --stats``
run of its own (``--trace N D TRUNCATED`` runs one configuration for it, ``--summarize DIR...`` turns the runs' kernel_stats
CSVs into the table of profiles/mds_kernel_trace.txt).  Prints one JSON line (profiles/mds_bench.json)."""
import csv
import ctypes as C
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np                                        # noqa: E402
from beast_mcmc_amd import mds                            # noqa: E402

TAU = 1.7
_D = C.POINTER(C.c_double)


def host_library(tmp):
    out = os.path.join(tmp, "libmds_host_restatement.so")
    subprocess.check_call(["g++", "-O3", "-std=c++17", "-fPIC", "-shared", os.path.join(ROOT, "tools", "mds_host_restatement.cpp"), "-o", out])
    lib = C.CDLL(out)
    lib.mds_host_synthesize.argtypes = [C.c_int, C.c_int, C.c_uint64, _D, _D]
    lib.mds_host_setup.argtypes = [C.c_int, C.c_int, C.c_int, C.c_double, _D, _D]
    lib.mds_host_full.restype = C.c_double
    lib.mds_host_row.argtypes, lib.mds_host_row.restype = [C.c_int, _D], C.c_double
    lib.mds_host_gradient.argtypes = [_D]
    return lib


def ptr(a):
    return a.ctypes.data_as(_D)


def timed(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), out


def inputs(host, n, d):
    x, y = np.empty((n, d)), np.empty((n, n))
    host.mds_host_synthesize(n, d, 1000 * d + n, ptr(x), ptr(y))
    return x, y


def measure(host, n, d, truncated, x, y, with_host=True):
    like = mds.MultiDimensionalScalingLikelihood(d, y, x, TAU, left_truncated=truncated)
    native, inst = like.native, like.instance
    reps = 20 if n <= 10000 else 8
    value = native.getSumOfIncrements(inst)                 # warm-up: code objects, first launches
    native.getLocationGradient(inst, np.empty(n * d))

    def full():
        native.makeDirty(inst)
        return native.getSumOfIncrements(inst)

    rng = np.random.default_rng(n + d)
    moves = [(int(rng.integers(n)), rng.normal(0.0, 0.3, size=d)) for _ in range(200)]
    xs = x.copy()

    def steps_device():
        t = []
        for k, delta in moves:
            xs[k] += delta
            native.storeState(inst)
            t0 = time.perf_counter()
            native.updateLocations(inst, k, xs[k])
            s = native.getSumOfIncrements(inst)
            t.append(time.perf_counter() - t0)
            native.acceptState(inst)
            assert native.stats(inst)["last_path"] == mds.PATH_ROW
        return float(np.median(t)), s

    grad = np.empty(n * d)
    full_s, full_value = timed(full, reps)
    assert np.float64(full_value).tobytes() == np.float64(value).tobytes()
    row_s, row_value = steps_device()
    grad_s, _ = timed(lambda: native.getLocationGradient(inst, grad), reps)
    like.close()
    out = {"N": n, "D": d, "left_truncated": bool(truncated), "reps": reps,
           "device_full_ms": round(1e3 * full_s, 4), "device_step_ms": round(1e3 * row_s, 4), "device_gradient_ms": round(1e3 * grad_s, 4),
           "triangle_bytes": 4 * n * n, "gradient_bytes": 8 * n * n,
           "full_design_GBps_wall": round(4 * n * n / full_s / 1e9, 1), "gradient_design_GBps_wall": round(8 * n * n / grad_s / 1e9, 1),
           "sum_of_increments": full_value}
    if with_host:
        host.mds_host_setup(n, d, int(truncated), TAU, ptr(x), ptr(y))
        host_reps = 3 if n <= 1000 else 1
        host_full_s, host_value = timed(host.mds_host_full, host_reps)
        xh, t = x.copy(), []
        for k, delta in moves:
            xh[k] += delta
            moved = np.ascontiguousarray(xh[k])
            t0 = time.perf_counter()
            host_row_value = host.mds_host_row(k, ptr(moved))
            t.append(time.perf_counter() - t0)
        host_row_s = float(np.median(t))
        host_grad = np.empty(n * d)
        host_grad_s, _ = timed(lambda: host.mds_host_gradient(ptr(host_grad)), host_reps)
        out.update({"host_full_ms": round(1e3 * host_full_s, 3), "host_step_ms": round(1e3 * host_row_s, 4),
                    "host_gradient_ms": round(1e3 * host_grad_s, 3),
                    "host_over_device_full": round(host_full_s / full_s, 1), "host_over_device_step": round(host_row_s / row_s, 3),
                    "host_over_device_gradient": round(host_grad_s / grad_s, 1),
                    "relative_difference_full": abs(full_value - host_value) / abs(host_value),
                    "relative_difference_after_steps": abs(row_value - host_row_value) / abs(host_row_value)})
    return out


def trace(host, n, d, truncated):
    """One configuration for a kernel trace: 10 full evaluations, 100 row updates, 10 gradients."""
    x, y = inputs(host, n, d)
    like = mds.MultiDimensionalScalingLikelihood(d, y, x, TAU, left_truncated=truncated)
    native, inst, rng, grad = like.native, like.instance, np.random.default_rng(1), np.empty(n * d)
    for _ in range(10):
        native.makeDirty(inst)
        native.getSumOfIncrements(inst)
    for _ in range(100):
        k = int(rng.integers(n))
        x[k] += rng.normal(0.0, 0.3, size=d)
        native.storeState(inst)
        native.updateLocations(inst, k, x[k])
        native.getSumOfIncrements(inst)
        native.acceptState(inst)
    for _ in range(10):
        native.getLocationGradient(inst, grad)
    like.close()


def summarize(directories):
    """directories named <N>_<D>_<truncated 0/1>, each with a *kernel_stats.csv of rocprofv3: one line per kernel with calls,
    average time, and the design bytes of the call over that time."""
    print("kernel times of libmds2_jni.so, rocprofv3 --kernel-trace --stats, one run per configuration (tools/mds_bench.py --trace)")
    print("%-7s %-2s %-9s %-26s %6s %12s %14s" % ("N", "D", "truncated", "kernel", "calls", "average us", "design GB/s"))
    for directory in directories:
        n, d, truncated = (int(v) for v in os.path.basename(os.path.normpath(directory)).split("_"))
        for path in glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                name = row["Name"]
                short = next((s for s in ("mdsSumKernel", "mdsFinishKernel", "mdsRowKernel", "mdsGradientKernel") if s in name), None)
                if short is None:
                    continue
                average_ns = float(row["AverageNs"])
                design = {"mdsSumKernel": 4.0 * n * n, "mdsGradientKernel": 8.0 * n * n, "mdsRowKernel": 8.0 * n}.get(short)
                print("%-7d %-2d %-9s %-26s %6s %12.2f %14s" % (n, d, bool(truncated), short, row["Calls"], average_ns / 1e3,
                                                            "%.1f" % (design / average_ns) if design else "-"))


def main():
    if "--summarize" in sys.argv:
        return summarize(sys.argv[sys.argv.index("--summarize") + 1:])
    with tempfile.TemporaryDirectory() as tmp:
        host = host_library(tmp)
        if "--trace" in sys.argv:
            n, d, truncated = (int(v) for v in sys.argv[sys.argv.index("--trace") + 1:][:3])
            return trace(host, n, d, bool(truncated))
        sizes = [int(v) for v in sys.argv[sys.argv.index("--sizes") + 1].split(",")] if "--sizes" in sys.argv else [1000, 10000, 20000]
        out = {"note": "device: wall times of whole calls, each ending in a synchronising read; host: single-threaded C++ restatement "
                       "with the Java core's table of increments; medians; tau = 1.7, 5 % of the pairs missing",
               "results": []}
        for n in sizes:
            for d in (2, 6):
                x, y = inputs(host, n, d)
                for truncated in (False, True):
                    out["results"].append(measure(host, n, d, truncated, x, y, with_host="--no-host" not in sys.argv))
                    print("N = %d D = %d truncated = %s done" % (n, d, truncated), file=sys.stderr, flush=True)
        print(json.dumps(out))


if __name__ == "__main__":
    main()
