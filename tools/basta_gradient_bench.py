#!/usr/bin/env python3
"""beagleBastaGradient (the migration-rate and population-size gradients of the BASTA log-density in one adjoint call) at the BASTA
benchmark's size — 1000 tips sampled through time, 4e5 operations; 4, 20 and 61 demes.  Nothing here was measured before; no ratio
is asserted.

Per deme count, after one evaluation:
  device      whole ``BastaLikelihood.gradient`` calls (both gradients, no adjoints out), the median of several after a warm-up; the
              kernel time and the launches of one call (beagleMi355KernelTimer); beside it the device's own likelihood on the same
              list, beagleBastaUpdatePartials + beagleBastaAccumulatePartials, timed the same way.
  C++ adjoint a single-threaded restatement of the same sweep (tools/basta_gradient_host_restatement.cpp, g++ -O3 -ffp-contract=off) on
              the vectors tools/basta_host_restatement.cpp forms from the device's matrices; its W, G_theta and adjoints must be the
              device's bit for bit.
  forward     the reference's route, S^2 tangent vectors per buffer (the same file, single-threaded like the reference's generic
              delegate), timed in full on FORWARD_TIPS tips — where it finishes and fits — checked against the adjoint there, and
              scaled by the operation count to the list's length.
And the stated worst case of the launch count: a ladder of 1000 tips at 4 demes, tips - 1 levels.
Prints one JSON line (profiles/basta_gradient_bench.json)."""
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
from beast_mcmc_amd import basta                          # noqa: E402
from beast_mcmc_amd.inputs import substmodel, trees       # noqa: E402

TIPS = 1000
FORWARD_TIPS = 12
I, D = C.POINTER(C.c_int), C.POINTER(C.c_double)


def host_library(tmp):
    out = os.path.join(tmp, "libbasta_gradient_host_restatement.so")
    subprocess.check_call(["g++", "-O3", "-ffp-contract=off", "-std=c++17", "-fPIC", "-shared",
                           os.path.join(ROOT, "tools", "basta_gradient_host_restatement.cpp"),
                           os.path.join(ROOT, "tools", "basta_host_restatement.cpp"), "-o", out])
    lib = C.CDLL(out)
    common = [C.c_int, I, C.c_int, I, C.c_int, D, D, D, D, D, C.c_int, D, C.c_int]
    lib.basta_gradient.argtypes = common + [D, D, D]
    lib.basta_gradient.restype = None
    lib.basta_gradient_forward.argtypes = common + [D, D]
    lib.basta_gradient_forward.restype = None
    lib.basta_evaluate.argtypes = [C.c_int, I, I, C.c_int, D, D, D, D, D, C.c_int]
    lib.basta_evaluate.restype = C.c_double
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


def dp(a):
    return a.ctypes.data_as(D)


class HostSide:
    """The list, the matrices (dense by number) and the vectors of one evaluation on the host."""

    def __init__(self, host, tr, tips, matrices, sizes, buffers):
        self.host, self.tr = host, tr
        self.s = s = tips.shape[1]
        self.ops, self.iv = np.ascontiguousarray(tr.operations), np.ascontiguousarray(tr.intervals)
        self.lengths, self.distances = np.ascontiguousarray(tr.lengths), np.ascontiguousarray(basta.interval_distances(tr))
        self.sizes, self.buffers, self.numbers = np.ascontiguousarray(sizes), buffers, tr.interval_count
        self.matrices = np.zeros((max(matrices) + 1, s, s))
        for m, x in matrices.items():
            self.matrices[m] = x
        self.partials = np.zeros((buffers, s))
        self.partials[:tips.shape[0]] = tips
        self.coalescent = np.zeros(self.numbers)
        self.logl = host.basta_evaluate(s, self.ops.ctypes.data_as(I), self.iv.ctypes.data_as(I), len(self.iv), dp(self.lengths),
                                        dp(self.matrices), dp(self.sizes), dp(self.partials), dp(self.coalescent), self.numbers)

    def _common(self):
        return (self.s, self.ops.ctypes.data_as(I), len(self.ops), self.iv.ctypes.data_as(I), len(self.iv), dp(self.lengths),
                dp(self.distances), dp(self.matrices), dp(self.sizes), dp(self.partials), self.buffers, dp(self.coalescent), self.numbers)

    def adjoint(self):
        lam, g, w = np.zeros((self.buffers, self.s)), np.zeros(self.s), np.zeros((self.s, self.s))
        t0 = time.perf_counter()
        self.host.basta_gradient(*self._common(), dp(lam), dp(g), dp(w))
        return time.perf_counter() - t0, {"adjoints": lam, "theta": g, "migration": w}

    def forward(self):
        g, w = np.zeros(self.s), np.zeros((self.s, self.s))
        t0 = time.perf_counter()
        self.host.basta_gradient_forward(*self._common(), dp(g), dp(w))
        return time.perf_counter() - t0, {"theta": g, "migration": w}


def make(state_count, tip_count, ladder=False):
    rng = np.random.default_rng(state_count)
    if ladder:
        tree = trees.caterpillar_tree(tip_count, root_height=2.0)
    else:
        tree = trees.heterochronous_coalescent_tree(tip_count, np.random.default_rng(1), sampling_span=1.0, population=30.0 * tip_count / TIPS)
    eig, _ = substmodel.random_reversible(state_count, rng)
    sizes = rng.gamma(4.0, 0.5, size=state_count) + 0.05
    demes = rng.integers(0, state_count, size=tip_count)
    like = basta.BastaLikelihood(tree, demes, basta.transpose_eigen(eig), sizes, rate=0.5)
    like.log_likelihood()
    return like


def device_times(like, reps):
    tr, b = like.traversal, like.beagle
    n, m = len(tr.operations), len(tr.intervals)
    out = np.zeros(1)

    def likelihood():
        b.updateBastaPartials(tr.operations, n, tr.intervals, m, like.sizes_index, 0)
        b.accumulateBastaPartials(tr.operations, n, tr.intervals, m, tr.lengths, like.sizes_index, 0, out)

    result = {"likelihood_ms": ms(timed(likelihood, reps)), "gradient_ms": ms(timed(like.gradient, reps))}
    b.kernelTimer(1)
    like.gradient()
    kernel_ms, launches = b.kernelTimer(0)
    calls, stat_launches, levels, chains = b.bastaGradientStats()
    result.update(gradient_kernel_ms=round(kernel_ms, 3), launches=int(launches), levels=int(levels), chains=int(chains),
                  gradient_over_likelihood=round(result["gradient_ms"] / result["likelihood_ms"], 2))
    return result


def host_side(host, like):
    tr, s = like.traversal, like.state_count
    matrices = {m: like.transition_matrix(m) for m, _ in tr.matrices}
    return HostSide(host, tr, like.tips, matrices, like.sizes, like.beagle.bastaStats()[3])


def worst(a, b):
    return max(float(np.abs(a[k] - b[k]).max() / np.abs(b[k]).max()) for k in ("theta", "migration"))


def measure(state_count, host, reps):
    like = make(state_count, TIPS)
    tr = like.traversal
    out = {"demes": state_count, "tips": TIPS, "operations": int(len(tr.operations)), "intervals": int(len(tr.intervals) - 1), "reps": reps}
    out["device"] = device_times(like, reps)
    side = host_side(host, like)
    device = like.gradient(adjoints=True)
    cpp_s = min(side.adjoint()[0] for _ in range(3))
    restated = side.adjoint()[1]
    out["cpp_adjoint_ms"] = ms(cpp_s)
    out["cpp_adjoint_over_device"] = round(1e3 * cpp_s / out["device"]["gradient_ms"], 2)
    out["host_equal_device"] = {k: bool(np.array_equal(device[k], restated[k])) for k in ("adjoints", "theta", "migration")}
    # the device against the same sweep in longdouble is the restatement's own error when the bits are equal: ratio 1
    out["device_over_restatement_error"] = 1.0 if all(out["host_equal_device"].values()) else None
    like.close()
    # the forward route at a size where it finishes
    small = make(state_count, FORWARD_TIPS)
    side = host_side(host, small)
    forward_s, forward = side.forward()
    small_adjoint = side.adjoint()[1]
    n_small = len(small.traversal.operations)
    out["forward"] = {"tips": FORWARD_TIPS, "operations": int(n_small), "ms": ms(forward_s),
                      "scaled_to_the_list_ms": ms(forward_s * out["operations"] / n_small),
                      "worst_relative_difference_from_adjoint": float("%.2e" % worst(small_adjoint, forward))}
    out["forward_scaled_over_device"] = round(out["forward"]["scaled_to_the_list_ms"] / out["device"]["gradient_ms"], 1)
    small.close()
    return out


def ladder(reps):
    like = make(4, TIPS, ladder=True)
    out = {"demes": 4, "tips": TIPS, "operations": int(len(like.traversal.operations)), "device": device_times(like, reps)}
    like.close()
    return out


def main():
    with tempfile.TemporaryDirectory() as tmp:
        host = host_library(tmp)
        out = {"note": "device: whole BastaLikelihood.gradient calls (W and G_theta) and whole update + accumulate calls, medians; C++: "
                       "single-threaded restatement of the adjoint sweep on the host's vectors; forward: the reference's S^2-tangent "
                       "route in single-threaded C++ at %d tips, scaled by the operation count" % FORWARD_TIPS}
        for s in (4, 20, 61):
            out["S%d" % s] = measure(s, host, reps=5)
        out["ladder"] = ladder(reps=3)
        print(json.dumps(out))


if __name__ == "__main__":
    main()
