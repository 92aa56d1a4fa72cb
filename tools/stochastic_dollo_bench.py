#!/usr/bin/env python3
"""The stochastic Dollo node-pattern likelihood in one call (beagleMi355NodePatternLikelihoods via
beast-mcmc_amd/stochasticdollo.py) against the same values formed the way AbstractObservationProcess.nodePatternLikelihood forms
them through the BEAGLE interface (src/dr/oldevomodel/MSSD/AbstractObservationProcess.java:174-210): a getPartials per node held as
partials, a getLogScaleFactors per internal node, then the loop over nodes x patterns x states on the host — numpy here, timed part
by part — and against a single-threaded C++ restatement of that loop that already has every partial in memory.

Sizes: 100 taxa x 2 000 binary patterns; 1 000 x 1e4 and 1 000 x 1e5 at S = 2; 500 x 5e4 at S = 21 (20 live states); one rate
category, every internal node rescaled.  The device call is timed whole (host copy of the [P] values included, no node terms), the
pruning pass is not part of either side.  Prints one JSON line (profiles/stochastic_dollo_bench.json).  ``--kernel-only N``: only
N device calls at the first size — what a kernel-trace run wraps."""
import argparse
import ctypes as C
import hashlib
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
import beast_mcmc_amd as bm                               # noqa: E402
import stochastic_dollo_cases as cases                    # noqa: E402
from beast_mcmc_amd.stochasticdollo import ALSTreeLikelihood   # noqa: E402

SIZES = [("100x2000-S2", 100, 2000, 2), ("1000x1e4-S2", 1000, 10000, 2), ("1000x1e5-S2", 1000, 100000, 2),
         ("500x5e4-S21", 500, 50000, 21)]

CPP = r"""
#include <cmath>
#include <vector>
// the loop of nodePatternLikelihood over partials that are already here: [node][P][S] (one category), children before parents
extern "C" void node_pattern_loop(const double* partials, const double* ownScale, const int* left, const int* right, const int* order,
                                  const double* logw, const int* extant, const double* freqs, int nodes, int tips, int P, int S,
                                  double* out) {
    std::vector<double> lam((size_t)nodes * P, 0.0), m(P, -INFINITY), s(P, 0.0);
    std::vector<int> below((size_t)nodes * P, 0), total(P, 0);
    for (int t = 0; t < tips; t++) for (int j = 0; j < P; j++) { below[(size_t)t * P + j] = extant[(size_t)t * P + j]; total[j] += extant[(size_t)t * P + j]; }
    for (int k = 0; k < nodes; k++) {
        const int n = order[k];
        const double* x = partials + (size_t)n * P * S;
        for (int j = 0; j < P; j++) {
            const size_t here = (size_t)n * P + j;
            if (n >= tips) {
                const size_t a = (size_t)left[n] * P + j, b = (size_t)right[n] * P + j;
                lam[here] = (lam[a] + lam[b]) + ownScale[here];
                below[here] = below[a] + below[b];
            }
            if (below[here] < total[j]) continue;
            double site = 0.0;
            for (int i = 0; i < S; i++) site += freqs[i] * x[(size_t)j * S + i];
            const double term = (std::log(site) + lam[here]) + logw[n];
            if (term > m[j]) { s[j] = s[j] * std::exp(m[j] - term) + 1.0; m[j] = term; }
            else if (term > -INFINITY) s[j] += std::exp(term - m[j]);
        }
    }
    for (int j = 0; j < P; j++) out[j] = s[j] > 0.0 ? m[j] + std::log(s[j]) : -INFINITY;
}
"""


def source_hash():
    h = hashlib.sha256()
    for f in ("kernels_nodepattern.hip", "engine_nodepattern.cpp"):
        with open(os.path.join(ROOT, "beast-mcmc_amd", "csrc", f), "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


def cpp_loop(tmp):
    src, lib = os.path.join(tmp, "loop.cpp"), os.path.join(tmp, "libloop.so")
    with open(src, "w") as fh:
        fh.write(CPP)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", src, "-o", lib])
    f = C.CDLL(lib).node_pattern_loop
    f.argtypes = [C.c_void_p] * 8 + [C.c_int] * 4 + [C.c_void_p]
    f.restype = None
    return f


def make(tips, P, S):
    tree = cases.random_tree(tips, seed=tips + S, root_height=1.0)
    states = cases.random_alignment(tips, P, S, seed=P + S, death_fraction=0.6, unknown_fraction=0.0)
    freqs, base = cases.random_model(S, S)
    return ALSTreeLikelihood.create(tree, states, np.ones(P), freqs, [1.0], [1.0], base_generator=base, death_rate=0.6, lam=1.0,
                                    rescale=True)


def median_ms(ts):
    return round(1e3 * float(np.median(ts)), 3)


def readback_route(als, loop):
    """The reference's way, streamed node by node; -> (values, seconds by part, the C++ loop's seconds over the kept partials)."""
    tree, b, P, S = als.tree, als.beagle, als.P, als.S
    t_part = t_scale = t_host = 0.0
    t0 = time.perf_counter()
    extant = als.tip_extant()
    total = extant.sum(axis=0)
    t_host += time.perf_counter() - t0
    keep = np.empty((tree.node_count, P, S))
    own = np.zeros((tree.node_count, P))
    live = {}
    m, s = np.full(P, -np.inf), np.zeros(P)
    order = tree.postorder()
    for n in order:
        if n < tree.tip_count:
            t0 = time.perf_counter()
            codes = als.tip_states[n]
            x = np.zeros((P, S))
            x[np.arange(P), np.minimum(codes, S - 1)] = 1.0
            lam, below = np.zeros(P), extant[n]
            t_host += time.perf_counter() - t0
        else:
            t0 = time.perf_counter()
            x = b.getPartials(als.tl.node_buffer_index(n), bm.beagle.NONE)[0]
            t_part += time.perf_counter() - t0
            t0 = time.perf_counter()
            own[n] = b.getLogScaleFactors(als.scale_index(n))
            t_scale += time.perf_counter() - t0
            t0 = time.perf_counter()
            (la, ba), (lb, bb) = live.pop(int(tree.left[n])), live.pop(int(tree.right[n]))
            lam, below = (la + lb) + own[n], ba + bb
            t_host += time.perf_counter() - t0
        t0 = time.perf_counter()
        keep[n] = x
        with np.errstate(divide="ignore", invalid="ignore"):
            term = np.where(below >= total, (np.log(x @ als.freqs) + lam) + np.log(als.node_survival_probability(n)), -np.inf)
            up = term > m
            s = np.where(up, s * np.exp(m - term) + 1.0, s + np.where(term > -np.inf, np.exp(term - m), 0.0))
            m = np.where(up, term, m)
        live[n] = (lam, below)
        t_host += time.perf_counter() - t0
    with np.errstate(divide="ignore"):
        value = np.where(s > 0, m + np.log(s), -np.inf)
    logw = np.array([np.log(als.node_survival_probability(n)) for n in range(tree.node_count)])
    out = np.empty(P)
    ext32, left, right, order32 = (np.ascontiguousarray(a, dtype=np.int32) for a in (extant, tree.left, tree.right, order))
    t0 = time.perf_counter()
    loop(keep.ctypes.data, own.ctypes.data, left.ctypes.data, right.ctypes.data, order32.ctypes.data, logw.ctypes.data, ext32.ctypes.data,
         als.freqs.ctypes.data, tree.node_count, tree.tip_count, P, S, out.ctypes.data)
    t_cpp = time.perf_counter() - t0
    return value, (t_part, t_scale, t_host), t_cpp, out


def measure(name, tips, P, S, reps, loop):
    als = make(tips, P, S)
    als.prune()
    rows, logw, _ = als.node_rows()
    als.beagle.nodePatternLikelihoods(rows, logw, als.death_state)       # first call: scratch allocation
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        value, _, total, rc = als.beagle.nodePatternLikelihoods(rows, logw, als.death_state)
        ts.append(time.perf_counter() - t0)
    back, (t_part, t_scale, t_host), t_cpp, cpp = readback_route(als, loop)
    finite = np.isfinite(value)
    worst = float(np.max(np.abs(value[finite] - back[finite]) / np.abs(back[finite])))
    worst_cpp = float(np.max(np.abs(value[finite] - cpp[finite]) / np.abs(cpp[finite])))
    t_back = t_part + t_scale + t_host
    out = {"taxa": tips, "patterns": P, "states": S, "rows": int(len(rows)), "reps": reps, "return_code": int(rc),
           "device_call_ms": median_ms(ts), "readback_route_ms": round(1e3 * t_back, 1), "readback_getPartials_ms": round(1e3 * t_part, 1),
           "readback_getLogScaleFactors_ms": round(1e3 * t_scale, 1), "readback_numpy_ms": round(1e3 * t_host, 1),
           "cpp_loop_with_partials_ms": round(1e3 * t_cpp, 1), "speedup_vs_readback_route": round(t_back / float(np.median(ts)), 1),
           "speedup_vs_cpp_loop": round(t_cpp / float(np.median(ts)), 1), "goal_10x_met": bool(t_back / float(np.median(ts)) >= 10.0),
           "largest_relative_difference_from_readback": worst, "largest_relative_difference_from_cpp": worst_cpp,
           "all_finite": bool(finite.all())}
    als.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default=",".join(s[0] for s in SIZES))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--kernel-only", type=int, default=0)
    args = ap.parse_args()
    wanted = [s for s in SIZES if s[0] in args.sizes.split(",")]
    if args.kernel_only:
        name, tips, P, S = wanted[0]
        als = make(tips, P, S)
        als.prune()
        rows, logw, _ = als.node_rows()
        for _ in range(args.kernel_only):
            als.beagle.nodePatternLikelihoods(rows, logw, als.death_state)
        als.close()
        return
    out = {"source_hash": source_hash()}
    with tempfile.TemporaryDirectory() as tmp:
        loop = cpp_loop(tmp)
        for name, tips, P, S in wanted:
            out[name] = measure(name, tips, P, S, args.reps, loop)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
