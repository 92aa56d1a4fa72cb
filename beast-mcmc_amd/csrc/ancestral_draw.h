// ancestral_draw.h — the stateless random numbers and the weighted draw shared by the device samplers (kernels_ancestral.hip,
// kernels_simulate.hip, kernels_uniformized.hip, kernels_robustcounts.hip, kernels_history.hip).  Device code only; include it from
// a .hip file that turns FMA contraction off.
#pragma once

#include <float.h>

namespace mi355 {
namespace draw {

// SplitMix64: the (key + 1)-th output from `state`, as a 64-bit integer (a draw, or the state of a stream of its own)
__device__ __forceinline__ unsigned long long mix64(unsigned long long state, unsigned long long key) {
    unsigned long long z = state + (key + 1ull) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// ... as a double in [0, 1) with 53 random bits
__device__ __forceinline__ double ancestralUniform(unsigned long long seed, unsigned long long ctr) {
    return (double)(mix64(seed, ctr) >> 11) * 0x1.0p-53;
}

// drawChoice over n weights w(i): MAP = first index of the strict maximum; otherwise randomChoicePDF with U = u * total, and the
// largest index of a positive weight when rounding lets the walk fall through.  A total that is not finite and > 0 sets `bad`
// and gives 0 (the reference's root: AncestralStateBeagleTreeLikelihood.java:473-477).
template <class W>
__device__ __forceinline__ int drawChoice(const W& w, int n, double u, bool map, bool& bad) {
    double total = 0.0, best = 0.0;
    int lastPositive = 0, choice = 0;
    for (int i = 0; i < n; i++) {
        const double v = w(i);
        total = total + v;
        if (v > 0.0) lastPositive = i;
        if (i == 0 || v > best) { best = v; choice = i; }
    }
    if (!(total > 0.0) || !(total <= DBL_MAX)) { bad = true; return 0; }
    if (map) return choice;
    double U = u * total;
    for (int i = 0; i < n; i++) {
        U = U - w(i);
        if (U < 0.0) return i;
    }
    return lastPositive;
}

}  // namespace draw
}  // namespace mi355
