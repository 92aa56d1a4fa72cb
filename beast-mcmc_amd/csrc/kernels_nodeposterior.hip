// kernels_nodeposterior.hip — marginal node state posteriors from resident pre- and post-order partials
// (beagleMi355NodePosteriors; kernels.h NodePosteriorRow has the formula).
//
// What the reference does for it (src/dr/oldevomodel/treelikelihood/NodePosteriorTreeLikelihood.java:119-235): a getPartials and a
// getNodeMatrix per node, then host loops over nodes, patterns and state pairs that rebuild the pre-order side.  Here both sides are
// already on the device, so a (row, pattern) is one elementwise product of two partials, a sum over the categories, and a division by
// the sum over the states.  It is a streaming pass: two partials read, at most one written.
//
// One kernel serves every state count and both layouts.  A workgroup takes the 64 patterns of one block of the totals.  In the
// plain layout [c][p][S] those are 64 S consecutive doubles of each category; in the T32 layout [c][p >> 5][S][32] they are two
// consecutive tiles, again 64 S consecutive doubles.  So the 256 threads sweep that run element by element — neighbouring lanes read
// neighbouring doubles whatever S is — and only the element's (pattern, state) differs between the layouts.  m[s] goes to LDS as
// [pattern][state] (rows padded to an odd length: a thread that walks its pattern's states meets no bank twice in a wave); one thread
// per pattern forms Z and the MAP state in ascending state order; the posteriors leave in the plain order, element by element again.
// Totals: the weighted posteriors stay in LDS and are folded over the 64 patterns by a fixed tree; launchBlockTotals
// (kernels_markovjumps.hip) adds the workgroups in ascending order.  No atomics on values.
//
// Every product is rounded on its own (no FMA contraction in this file) and every sum runs over its index in ascending order from
// 0.0, as the host restatement forms it (tests/node_posteriors_reference.py): the two agree bit for bit.
#pragma clang fp contract(off)

#include "kernels.h"

namespace mi355 {

namespace {

constexpr int NP_PATTERNS = 64;              // patterns per workgroup = per entry of blockSums (edgeBlocks)
constexpr int NP_THREADS = 256;

__device__ __forceinline__ bool npBad(double z) { return !(z != 0.0 && isfinite(z)); }

template <bool TILED>
__global__ __launch_bounds__(NP_THREADS) void k_nodePosterior(const NodePosteriorRow* __restrict__ rows, const double* __restrict__ catWeights,
                                                              const double* __restrict__ patternWeights, int P, int S, int C, int nRows,
                                                              double* __restrict__ posteriors, uint8_t* __restrict__ mapStates,
                                                              double* __restrict__ mapProbabilities, double* __restrict__ blockSums,
                                                              unsigned* __restrict__ fpError) {
    extern __shared__ double npLds[];              // m [64][SP] | Z [64] | pattern weights [64]
    const int tid = threadIdx.x, SP = S | 1, p0 = (int)blockIdx.x * NP_PATTERNS;
    double* m = npLds; double* zs = m + NP_PATTERNS * SP; double* pw = zs + NP_PATTERNS;
    const NodePosteriorRow row = rows[blockIdx.y];
    const int nPat = min(NP_PATTERNS, P - p0);                                     // patterns of this block that exist
    const int inMemory = TILED ? min(NP_PATTERNS, ((P + 31) >> 5) * 32 - p0) : nPat;    // ... that the layout holds (T32: whole tiles)
    const int nElem = NP_PATTERNS * S, nLoad = inMemory * S;
    const size_t stride = TILED ? (size_t)((P + 31) >> 5) * 32 * S : (size_t)P * S;   // doubles per category
    const size_t base = (size_t)p0 * S;
    const double MI355_GLOBAL* pre = gptr(row.pre);
    const double MI355_GLOBAL* post = gptr(reinterpret_cast<const double*>(row.post));
    const uint8_t MI355_GLOBAL* states = gptr(reinterpret_cast<const uint8_t*>(row.post));
    const bool compact = row.statesPost != 0;

    for (int e = tid; e < nElem; e += NP_THREADS) {
        int pl, s;
        if (TILED) { const int t = e / (32 * S), r = e - t * 32 * S; s = r >> 5; pl = t * 32 + (r & 31); }
        else { pl = e / S; s = e - pl * S; }
        double acc = 0.0;
        if (e < nLoad) {
            double y = 1.0;
            if (compact) { const int st = pl < nPat ? (int)states[p0 + pl] : S; y = (st >= S || st == s) ? 1.0 : 0.0; }
            for (int c = 0; c < C; c++) {
                const size_t at = (size_t)c * stride + base + e;
                const double x = pre[at];
                if (!compact) y = post[at];
                acc = acc + (x * y) * catWeights[c];
            }
        }
        m[pl * SP + s] = acc;
    }
    __syncthreads();

    if (tid < NP_PATTERNS) {
        double z = 1.0, w = 0.0;
        if (tid < nPat) {
            const double* mine = m + tid * SP;
            z = 0.0;
            for (int s = 0; s < S; s++) z = z + mine[s];
            const bool bad = npBad(z);
            if (bad) { z = NAN; *fpError = 1u; }
            if (mapStates || mapProbabilities) {
                int best = 0;
                double bestValue = mine[0] / z;
                for (int s = 1; s < S; s++) { const double v = mine[s] / z; if (v > bestValue) { bestValue = v; best = s; } }
                const size_t at = (size_t)row.slot * P + p0 + tid;
                if (mapStates) mapStates[at] = (uint8_t)best;
                if (mapProbabilities) mapProbabilities[at] = bestValue;
            }
            w = patternWeights[p0 + tid];
        }
        zs[tid] = z; pw[tid] = w;
    }
    __syncthreads();

    // the plain order from here on, whatever the layout of the partials: out[slot][p][s] is written element by element
    const int nOut = nPat * S;
    double* out = posteriors ? posteriors + ((size_t)row.slot * P + p0) * S : nullptr;
    for (int e = tid; e < nElem; e += NP_THREADS) {
        const int pl = e / S, s = e - pl * S;
        double v = 0.0;
        if (e < nOut) {
            v = m[pl * SP + s] / zs[pl];
            if (out) out[e] = v;
            v = pw[pl] * v;
        }
        m[pl * SP + s] = v;                                                        // (patterns past the end: 0.0)
    }
    if (!blockSums) return;
    __syncthreads();
    for (int off = NP_PATTERNS / 2; off > 0; off >>= 1) {
        for (int e = tid; e < off * S; e += NP_THREADS) {
            const int pl = e / S, s = e - pl * S;
            m[pl * SP + s] = m[pl * SP + s] + m[(pl + off) * SP + s];
        }
        __syncthreads();
    }
    double* sums = blockSums + ((size_t)blockIdx.x * nRows + row.slot) * S;
    for (int s = tid; s < S; s += NP_THREADS) sums[s] = m[s];
}

// one thread per pattern of ONE row: a thousandth of the call's work, so the strided reads of the plain layout do not matter
template <bool TILED>
__global__ __launch_bounds__(NP_THREADS) void k_nodePosteriorCategories(const NodePosteriorRow* __restrict__ rowPtr, const double* __restrict__ catWeights,
                                                                        int P, int S, int C, double* __restrict__ categories,
                                                                        unsigned* __restrict__ fpError) {
    const int p = (int)blockIdx.x * NP_THREADS + (int)threadIdx.x;
    if (p >= P) return;
    const NodePosteriorRow row = *rowPtr;
    const double MI355_GLOBAL* pre = gptr(row.pre);
    const double MI355_GLOBAL* post = gptr(reinterpret_cast<const double*>(row.post));
    const bool compact = row.statesPost != 0;
    const int st = compact ? (int)gptr(reinterpret_cast<const uint8_t*>(row.post))[p] : 0;
    const int ntile = (P + 31) >> 5;
    double* mine = categories + (size_t)p * C;
    double d = 0.0;
    for (int c = 0; c < C; c++) {
        double n = 0.0;
        for (int s = 0; s < S; s++) {
            const size_t at = TILED ? (((size_t)c * ntile + (p >> 5)) * S + s) * 32 + (p & 31) : ((size_t)c * P + p) * S + s;
            const double y = compact ? ((st >= S || st == s) ? 1.0 : 0.0) : post[at];
            n = n + pre[at] * y;
        }
        n = n * catWeights[c];
        mine[c] = n;
        d = d + n;
    }
    if (npBad(d)) { d = NAN; *fpError = 1u; }
    for (int c = 0; c < C; c++) mine[c] = mine[c] / d;
}

}  // namespace

bool launchNodePosteriors(hipStream_t stream, const NodePosteriorRow* dRows, int nRows, const double* catWeights,
                          const double* patternWeights, int P, int S, int C, bool tiled, double* posteriors, uint8_t* mapStates,
                          double* mapProbabilities, double* blockSums, unsigned* fpError) {
    if (nRows <= 0 || P <= 0) return true;
    if (nRows > NODE_POSTERIOR_MAX_ROWS) return false;
    const size_t lds = ((size_t)NP_PATTERNS * (S | 1) + 2 * NP_PATTERNS) * sizeof(double);
    if (lds > 160 * 1024) return false;
    if (!grantDynamicLds(reinterpret_cast<const void*>(k_nodePosterior<false>), 160 * 1024) ||
        !grantDynamicLds(reinterpret_cast<const void*>(k_nodePosterior<true>), 160 * 1024)) return false;
    const dim3 grid((unsigned)edgeBlocks(P), (unsigned)nRows), block(NP_THREADS);
    if (tiled) hipLaunchKernelGGL(k_nodePosterior<true>, grid, block, lds, stream, dRows, catWeights, patternWeights, P, S, C, nRows, posteriors,
                                  mapStates, mapProbabilities, blockSums, fpError);
    else hipLaunchKernelGGL(k_nodePosterior<false>, grid, block, lds, stream, dRows, catWeights, patternWeights, P, S, C, nRows, posteriors,
                            mapStates, mapProbabilities, blockSums, fpError);
    return true;
}

void launchNodePosteriorCategories(hipStream_t stream, const NodePosteriorRow* dRow, const double* catWeights, int P, int S, int C,
                                   bool tiled, double* categories, unsigned* fpError) {
    if (P <= 0) return;
    const dim3 grid((unsigned)((P + NP_THREADS - 1) / NP_THREADS)), block(NP_THREADS);
    if (tiled) hipLaunchKernelGGL(k_nodePosteriorCategories<true>, grid, block, 0, stream, dRow, catWeights, P, S, C, categories, fpError);
    else hipLaunchKernelGGL(k_nodePosteriorCategories<false>, grid, block, 0, stream, dRow, catWeights, P, S, C, categories, fpError);
}

}  // namespace mi355
