// kernels_nodepattern.hip — the stochastic Dollo (ALS) node-pattern likelihood of every pattern in one launch
// (beagleMi355NodePatternLikelihoods).
//
// What it restates: AbstractObservationProcess.nodePatternLikelihood's loop over nodes and patterns
// (src/dr/oldevomodel/MSSD/AbstractObservationProcess.java:174-210), the inclusion masks of AnyTipObservationProcess
// (AnyTipObservationProcess.java:97-168) and ScaleFactorsHelper.traverseComputeScaleFactors
// (src/dr/oldevomodel/treelikelihood/ScaleFactorsHelper.java:83-104).  The reference reads ONE category's worth of partials, so it
// only runs with one rate category; the category-weighted sum is this library's extension (include/beagle_mi355.h).  It adds the
// rows' terms in linear space; here they are added by a running-maximum log-sum-exp, which does not underflow on large trees.
//
// One thread per pattern walks the rows of the post-order node list: patterns are independent, so no thread waits for another.  The
// row descriptor is the same for every lane (scalar loads); partials are read at the pattern's own address (plain [c][p][S] or T32
// [c][p>>5][S][32]).  A first loop over the tip rows totals the extant tips of the pattern; the walk then takes a row's Lambda (the
// log scale factors of its whole subtree) and its count of extant tips below from its children's entries of two [slot][stride]
// arrays — the same thread wrote them, so program order makes them visible.  A row's slot is free again once its parent has read
// it (the host hands slots out: engine_nodepattern.cpp), so the arrays hold as many rows as are ever pending at once — a few, and
// they stay in the L2 — instead of every row of the list.  A row that is not included in the pattern (most are not: only the
// ancestors of the extant tips' common ancestor are) costs its scale factor and two additions; the partials, the logarithm and
// the exponential are for included rows only.  The weighted sum over patterns leaves each workgroup through a fixed tree in LDS;
// k_blockTotals (kernels_markovjumps.hip) adds the workgroups in ascending order.  No atomics.
//
// Every product is rounded on its own (no FMA contraction in this file) and every sum runs over its index in ascending order from
// 0.0, as the host restatement forms it (tests/stochastic_dollo_reference.py): the two differ only where exp() and log() do.
#pragma clang fp contract(off)

#include "kernels.h"

namespace mi355 {

namespace {

// SS = 2, 4: the state count as a constant (the dot product unrolled); SS = 0: any state count
template <int SS>
__global__ __launch_bounds__(256) void k_nodePattern(const NodePatternRow* __restrict__ rows, int nRows,
                                                     const double* __restrict__ catWeights, const double* __restrict__ freqs,
                                                     const double* __restrict__ patternWeights, int P, int Sdyn, int C, int tiled,
                                                     int deathState, int p0, int count, int stride, double* __restrict__ lambda,
                                                     int* __restrict__ below, double* __restrict__ terms,
                                                     double* __restrict__ logPattern, double* __restrict__ blockSums) {
    __shared__ double red[256];
    const int S = SS ? SS : Sdyn;
    const int q = blockIdx.x * 256 + threadIdx.x;          // the pattern's column of the [slot][stride] arrays
    const int p = p0 + q;
    double weighted = 0.0;
    if (q < count) {
        const int ntile = (P + 31) >> 5;
        // element i of category c of a partials buffer, at this thread's pattern
        auto at = [&](const double* buf, int c, int i) -> double {
            const double MI355_GLOBAL* b = gptr(buf);
            return tiled ? b[(((size_t)c * ntile + (p >> 5)) * S + i) * 32 + (p & 31)] : b[((size_t)c * P + p) * S + i];
        };
        const double MI355_GLOBAL* w = gptr(catWeights);
        const double MI355_GLOBAL* pi = gptr(freqs);

        // ---- the tip rows: at how many tips the pattern is extant
        auto extantAt = [&](const NodePatternRow& row) -> int {
            if (row.states) {
                const int s = gptr(row.states)[p];
                return (s < S && s != deathState) ? 1 : 0;
            }
            return at(row.partials, 0, deathState) == 0.0 ? 1 : 0;
        };
        int total = 0;
        for (int r = 0; r < nRows; r++) {
            const NodePatternRow row = rows[r];
            if (row.child1 < 0) total += extantAt(row);
        }
        double piSum = 0.0;                                // what a compact tip's unknown code stands for
        for (int i = 0; i < S; i++) piSum = piSum + pi[i];

        // ---- every row in list order (children before their parent)
        double m = -INFINITY, sum = 0.0;
        bool bad = false;
        for (int r = 0; r < nRows; r++) {
            const NodePatternRow row = rows[r];
            const size_t here = (size_t)row.slot * stride + q;
            double lam = 0.0;
            int b;
            if (row.child1 >= 0) {
                const size_t c1 = (size_t)row.slot1 * stride + q, c2 = (size_t)row.slot2 * stride + q;
                lam = lambda[c1] + lambda[c2];
                if (row.scale) {
                    const double f = gptr(row.scale)[p];
                    lam = lam + (row.scaleRaw ? log(f) : f);
                }
                b = below[c1] + below[c2];
            } else {
                b = extantAt(row);
            }
            lambda[here] = lam;
            below[here] = b;
            double term = -INFINITY;
            if (b >= total) {                              // (few rows of a pattern are: the others cost no partials, no log, no exp)
                double site = 0.0;
                if (row.states) {
                    const int s = gptr(row.states)[p];
                    const double inner = s < S ? pi[s] : piSum;
                    for (int c = 0; c < C; c++) site = site + w[c] * inner;
                } else {
                    for (int c = 0; c < C; c++) {
                        double inner = 0.0;
#pragma unroll
                        for (int i = 0; i < S; i++) inner = inner + pi[i] * at(row.partials, c, i);
                        site = site + w[c] * inner;
                    }
                }
                term = (log(site) + lam) + row.logWeight;
                if (term > m) {
                    if (term == INFINITY) bad = true;
                    else { sum = sum * exp(m - term) + 1.0; m = term; }
                } else if (term > -INFINITY) {
                    sum = sum + exp(term - m);
                } else if (term != term) {
                    bad = true;
                }
            }
            if (terms) terms[(size_t)r * stride + q] = term;
        }
        const double v = bad ? (double)NAN : (sum > 0.0 ? m + log(sum) : -INFINITY);
        logPattern[p] = v;
        weighted = gptr(patternWeights)[p] * v;
    }
    red[threadIdx.x] = weighted;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) red[threadIdx.x] = red[threadIdx.x] + red[threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0) blockSums[p0 / 256 + blockIdx.x] = red[0];
}

}  // namespace

int nodePatternBlocks(int P) { return (P + 255) / 256; }

void launchNodePattern(hipStream_t stream, const NodePatternRow* dRows, int nRows, const double* catWeights, const double* freqs,
                       const double* patternWeights, int P, int S, int C, bool tiled, int deathState, int p0, int count, int stride,
                       double* lambda, int* below, double* terms, double* logPattern, double* blockSums) {
    const dim3 grid((count + 255) / 256), block(256);
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, grid, block, 0, stream, dRows, nRows, catWeights, freqs, patternWeights, P, S, C, tiled ? 1 : 0,
                           deathState, p0, count, stride, lambda, below, terms, logPattern, blockSums);
    };
    if (S == 2) launch(k_nodePattern<2>);
    else if (S == 4) launch(k_nodePattern<4>);
    else launch(k_nodePattern<0>);
}

}  // namespace mi355
