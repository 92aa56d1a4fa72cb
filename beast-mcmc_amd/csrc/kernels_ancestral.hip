// kernels_ancestral.hip — one draw of every listed node's state per site (beagleMi355SampleAncestralStates).
//
// What it restates (reference = /root/reference): AncestralStateBeagleTreeLikelihood.traverseSample
// (src/dr/evomodel/treelikelihood/AncestralStateBeagleTreeLikelihood.java:414-625) with linear-space conditionals, and its
// drawChoice (:246-256) -> MathUtils.randomChoicePDF (src/dr/math/MathUtils.java:82-104).
//
// One thread per pattern walks the rows of the node list in order (row 0 is the root, every other row's parent comes earlier):
// patterns are independent, so no thread waits for another.  A row's state goes to states[row][p]; a child reads its parent's
// state back from there — the same thread wrote it, so program order makes it visible.  The row descriptor is the same for every
// lane (scalar loads); partials are read at the pattern's own address (plain [c][p][S] or T32 [c][p>>5][S][32]), the branch
// matrix row M[r*][parentState][.] is a gather from a few hundred bytes that stay in the L1/L2.
//
// Every weight, sum and difference is formed exactly as the host restatement forms it (tests/ancestral_reference.py): no FMA
// contraction anywhere in this file, sums in index order.  The weights of a draw are computed twice — once for the total, once
// for the walk down the cumulative sum — instead of being held in an array: the same operands give the same products, and no
// state count needs a per-thread array.
#pragma clang fp contract(off)

#include "kernels.h"
#include "ancestral_draw.h"

namespace mi355 {

namespace {

using draw::ancestralUniform;
using draw::drawChoice;

// SS = 4: the state count as a constant (loops unrolled, the row's partials held in registers); SS = 0: any state count
template <int SS>
__global__ __launch_bounds__(256) void k_sampleAncestral(const AncestralRow* __restrict__ rows, int nRows,
                                                         const double* __restrict__ catWeights, const double* __restrict__ freqs,
                                                         int P, int Sdyn, int C, int tiled, int globalP, int pOffset,
                                                         unsigned long long seed, int map, uint8_t* __restrict__ states,
                                                         int* __restrict__ cats, unsigned* __restrict__ fpError) {
    const int S = SS ? SS : Sdyn;
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= P) return;
    const int ntile = (P + 31) >> 5;
    const unsigned long long gp = (unsigned long long)(pOffset + p), GP = (unsigned long long)globalP;
    // element i of category c of a partials buffer, at this thread's pattern
    auto at = [&](const double* buf, int c, int i) -> double {
        const double MI355_GLOBAL* b = gptr(buf);
        return tiled ? b[(((size_t)c * ntile + (p >> 5)) * S + i) * 32 + (p & 31)] : b[((size_t)c * P + p) * S + i];
    };
    bool bad = false;

    // ---- root: rate category (C > 1), then the state
    const AncestralRow root = rows[0];
    int cat = 0;
    if (C > 1) {
        auto wc = [&](int r) {
            double s = 0.0;
            for (int k = 0; k < S; k++) s = s + at(root.partials, r, k);
            return s * gptr(catWeights)[r];
        };
        cat = drawChoice(wc, C, ancestralUniform(seed, gp * 2 + 1), map != 0, bad);
    }
    {
        auto w = [&](int i) { return at(root.partials, cat, i) * gptr(freqs)[i]; };
        states[p] = (uint8_t)drawChoice(w, S, ancestralUniform(seed, gp * 2), map != 0, bad);
    }

    // ---- every other row, in list order
    for (int r = 1; r < nRows; r++) {
        const AncestralRow row = rows[r];
        const int parentState = states[(size_t)row.parent * P + p];
        const double MI355_GLOBAL* m = gptr(row.matrix) + ((size_t)cat * S + parentState) * S;
        const double u = ancestralUniform(seed, ((unsigned long long)r * GP + gp) * 2);
        int s;
        if (row.states) {
            s = gptr(row.states)[p];
            if (s >= S) {
                auto w = [&](int i) { return m[i]; };
                s = drawChoice(w, S, u, map != 0, bad);
            }
        } else if (SS) {
            double part[SS > 0 ? SS : 1], mrow[SS > 0 ? SS : 1];
#pragma unroll
            for (int i = 0; i < SS; i++) { part[i] = at(row.partials, cat, i); mrow[i] = m[i]; }
            auto w = [&](int i) { return part[i] * mrow[i]; };
            s = drawChoice(w, SS, u, map != 0, bad);
        } else {
            auto w = [&](int i) { return at(row.partials, cat, i) * m[i]; };
            s = drawChoice(w, S, u, map != 0, bad);
        }
        states[(size_t)r * P + p] = (uint8_t)s;
    }
    if (cats) cats[p] = cat;
    if (bad) atomicOr(fpError, 1u);
}

}  // namespace

void launchSampleAncestral(hipStream_t stream, const AncestralRow* dRows, int nRows, const double* catWeights, const double* freqs,
                           int P, int S, int C, bool tiled, int globalP, int pOffset, unsigned long long seed, bool map,
                           uint8_t* states, int* cats, unsigned* fpError) {
    const dim3 grid((P + 255) / 256), block(256);
    if (S == 4)
        hipLaunchKernelGGL(k_sampleAncestral<4>, grid, block, 0, stream, dRows, nRows, catWeights, freqs, P, S, C, tiled ? 1 : 0,
                           globalP, pOffset, seed, map ? 1 : 0, states, cats, fpError);
    else
        hipLaunchKernelGGL(k_sampleAncestral<0>, grid, block, 0, stream, dRows, nRows, catWeights, freqs, P, S, C, tiled ? 1 : 0,
                           globalP, pOffset, seed, map ? 1 : 0, states, cats, fpError);
}

}  // namespace mi355
