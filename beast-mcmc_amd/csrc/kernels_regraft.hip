// kernels_regraft.hip — scores of hanging a pruned subtree at candidate points of the tree it was cut from, from resident partials and
// matrices (beagleMi355RegraftScores; kernels.h has the formulas).
//
// What the reference does for it (src/dr/evomodel/operators/GibbsPruneAndRegraft.java:89-160, :162-269): per candidate branch two tree
// edits and a whole likelihood evaluation.  After a gradient pass over the tree without the subtree the engine holds what every one of
// those likelihoods is made of, exactly as for a new tip (kernels_placement.hip) — but what is attached is a partials vector per
// pattern, not a code, so there is no table over codes and the result is ONE number per (candidate, pattern):
//   k_regraftPendants    q[m][c][p][a] = sum_b Mpend_c[a][b] post_sub,c,p(b), once per distinct pendant matrix of the list (the Gibbs
//                        operator has one), stored in the layout of the instance's partials: the main stage streams it as a fourth
//                        partials buffer and pays no fourth mat-vec per candidate.
//   k_regraftRatios      R_k[p] = log(N_p / D_p) + logscale_sub[p] for a chunk of candidates.  A workgroup takes one candidate and one
//                        block of patterns and sweeps, per category, the three partials into LDS as k_placementTable does (the same
//                        loads, the same mat-vecs, ONE matrix of ONE category in LDS at a time); then q's block replaces the child's
//                        vector and a thread per pattern adds e . q and sum e into N and D.  One logarithm and one division a pattern.
//   k_regraftRatios4     the same at 4 states (the plain layout): a thread per pattern, 32-byte loads, wave-uniform matrix loads,
//                        registers only — no LDS, no barrier.
//   k_regraftSegments    per segment of REGRAFT_SEGMENT patterns ONE accumulator per candidate, sum of w_p R_k[p] ascending from 0.0, a
//                        pattern of weight 0 left out; k_regraftScoreSum adds the segments in ascending order from 0.0.  The order is
//                        a function of P alone, whatever the chunking or the list.
// No atomics on values, nothing waits on another workgroup, plain stores only.
#include "kernels.h"

#include <algorithm>

namespace mi355 {

namespace {

constexpr int RG_THREADS = 256;
constexpr int RG_MATRIX_LDS_BYTES = 40 * 1024;       // a matrix of one category is kept in LDS up to this size

struct RgShape { int P, S, C, PB, SP; };             // PB patterns per workgroup; SP the odd row length

// element (c, p, a) of a partials buffer in the instance's layout
template <bool TILED>
__device__ __forceinline__ size_t rgIndex(int c, int p, int a, int P, int S) {
    if (TILED) return ((size_t)c * ((P + 31) >> 5) * 32 + (size_t)(p >> 5) * 32) * S + (size_t)a * 32 + (p & 31);
    return ((size_t)c * P + p) * S + a;
}

template <bool TILED>
__global__ __launch_bounds__(RG_THREADS) void k_regraftPendants(const double* __restrict__ matrices, const int* __restrict__ slots, int nSlots,
                                                                const void* __restrict__ subtree, int subtreeStates, int P, int S, int C,
                                                                size_t perVector, double* __restrict__ out) {
    const size_t n = (size_t)nSlots * C * P * S, i = (size_t)blockIdx.x * RG_THREADS + threadIdx.x;
    if (i >= n) return;
    const int a = (int)(i % S), p = (int)(i / S % P), c = (int)(i / S / P % C), m = (int)(i / S / P / C);
    const double* row = matrices + ((size_t)slots[m] * C + c) * S * S + (size_t)a * S;
    double acc = 0.0;
    if (subtreeStates) {
        const int st = (int)reinterpret_cast<const uint8_t*>(subtree)[p];
        for (int b = 0; b < S; b++) acc += row[b] * ((st >= S || st == b) ? 1.0 : 0.0);
    } else {
        const double* x = reinterpret_cast<const double*>(subtree);
        for (int b = 0; b < S; b++) acc += row[b] * x[rgIndex<TILED>(c, p, b, P, S)];
    }
    out[(size_t)m * perVector + rgIndex<TILED>(c, p, a, P, S)] = acc;
}

// the block's PB patterns of category c of a partials buffer (or of a compact tip's states) into v [PB][SP]; rows past the block's
// last pattern are zeros (k_placementTable's plLoadVector)
template <bool TILED>
__device__ __forceinline__ void rgLoadVector(double* v, const void* src, bool compact, int c, int p0, int nPat, const RgShape& g) {
    const int tid = threadIdx.x, S = g.S, P = g.P;
    const int nElem = g.PB * S;
    const int inMemory = TILED ? min(g.PB, ((P + 31) >> 5) * 32 - p0) : nPat;
    const int nLoad = inMemory * S;
    const size_t stride = TILED ? (size_t)((P + 31) >> 5) * 32 * S : (size_t)P * S;
    const double MI355_GLOBAL* x = gptr(reinterpret_cast<const double*>(src)) + (size_t)c * stride + (size_t)p0 * S;
    const uint8_t MI355_GLOBAL* states = gptr(reinterpret_cast<const uint8_t*>(src));
    for (int e = tid; e < nElem; e += RG_THREADS) {
        int pl, s;
        if (TILED) { const int t = e / (32 * S), r = e - t * 32 * S; s = r >> 5; pl = t * 32 + (r & 31); }
        else { pl = e / S; s = e - pl * S; }
        double y = 0.0;
        if (e < nLoad && pl < nPat) {
            if (compact) { const int st = (int)states[p0 + pl]; y = (st >= S || st == s) ? 1.0 : 0.0; }
            else y = x[e];
        }
        v[pl * g.SP + s] = y;
    }
}

__device__ __forceinline__ void rgLoadMatrix(double* m, const double* src, int n) {
    const double MI355_GLOBAL* x = gptr(src);
    for (int e = threadIdx.x; e < n; e += RG_THREADS) m[e] = x[e];
}

// (a pattern of weight 0 reaches no score: its NaN is written and is no error)
__device__ __forceinline__ double rgRatio(double N, double D, const double* scale, int scaleRaw, const double* patternWeights, int p,
                                          unsigned* fpError) {
    if (!(D != 0.0 && isfinite(D))) { if (gptr(patternWeights)[p] != 0.0) *fpError = 1u; return NAN; }
    double r = log(N / D);
    if (scale) { const double f = gptr(scale)[p]; r += scaleRaw ? log(f) : f; }
    return r;
}

template <bool TILED, bool MLDS>
__global__ __launch_bounds__(RG_THREADS) void k_regraftRatios(const PlacementCandidate* __restrict__ cands, const double* __restrict__ catWeights,
                                                              const double* __restrict__ pendants, size_t perVector,
                                                              const double* __restrict__ scale, int scaleRaw,
                                                              const double* __restrict__ patternWeights, RgShape g,
                                                              double* __restrict__ ratios, unsigned* __restrict__ fpError) {
    extern __shared__ __attribute__((aligned(16))) double rgLds[];        // A [PB][SP] | B [PB][SP] | N [PB] | D [PB] | matrix [S][S] (MLDS)
    const int tid = threadIdx.x, S = g.S, PB = g.PB, SP = g.SP;
    double* A = rgLds; double* B = A + PB * SP; double* N = B + PB * SP; double* D = N + PB; double* ML = D + PB;
    const PlacementCandidate cand = cands[blockIdx.y];
    const int p0 = (int)blockIdx.x * PB, nPat = min(PB, g.P - p0);
    const size_t SS = (size_t)S * S;
    const double* q = pendants + (size_t)cand.pendant * perVector;

    if (tid < PB) { N[tid] = 0.0; D[tid] = 0.0; }

    for (int c = 0; c < g.C; c++) {
        double* t = A; double* other = B;
        // u = pre * (Msib post_sib)
        __syncthreads();                                                           // (the last category's readers are done)
        rgLoadVector<TILED>(A, cand.pre, false, c, p0, nPat, g);
        if (cand.sib) {
            rgLoadVector<TILED>(B, cand.sib, cand.sibStates != 0, c, p0, nPat, g);
            const double* Mg = cand.mSib + c * SS;
            if (MLDS) rgLoadMatrix(ML, Mg, (int)SS);
            __syncthreads();
            const double MI355_GLOBAL* Mx = gptr(Mg);
            for (int e = tid; e < PB * S; e += RG_THREADS) {
                const int pl = e % PB, a = e / PB;
                const double* v = B + pl * SP;
                double acc = 0.0;
                for (int b = 0; b < S; b++) acc += (MLDS ? ML[a * S + b] : Mx[a * S + b]) * v[b];
                A[pl * SP + a] *= acc;
            }
        }
        __syncthreads();
        // t = u Mup
        if (cand.mUp) {
            const double* Mg = cand.mUp + c * SS;
            if (MLDS) { rgLoadMatrix(ML, Mg, (int)SS); __syncthreads(); }
            const double MI355_GLOBAL* Mx = gptr(Mg);
            for (int e = tid; e < PB * S; e += RG_THREADS) {
                const int pl = e % PB, a = e / PB;
                const double* v = A + pl * SP;
                double acc = 0.0;
                for (int b = 0; b < S; b++) acc += v[b] * (MLDS ? ML[b * S + a] : Mx[b * S + a]);
                B[pl * SP + a] = acc;
            }
            t = B; other = A;
            __syncthreads();
        }
        // e = t * (Mlow post_child)
        {
            rgLoadVector<TILED>(other, cand.child, cand.childStates != 0, c, p0, nPat, g);
            const double* Mg = cand.mLow + c * SS;
            if (MLDS) rgLoadMatrix(ML, Mg, (int)SS);
            __syncthreads();
            const double MI355_GLOBAL* Mx = gptr(Mg);
            for (int e = tid; e < PB * S; e += RG_THREADS) {
                const int pl = e % PB, a = e / PB;
                const double* v = other + pl * SP;
                double acc = 0.0;
                for (int b = 0; b < S; b++) acc += (MLDS ? ML[a * S + b] : Mx[a * S + b]) * v[b];
                t[pl * SP + a] *= acc;
            }
            __syncthreads();
        }
        // N += w_c e . q_c, D += w_c sum e: the pendant vector's block takes the child's place
        {
            rgLoadVector<TILED>(other, q, false, c, p0, nPat, g);
            __syncthreads();
            if (tid < PB) {
                const double w = catWeights[c];
                const double* v = t + tid * SP;
                const double* y = other + tid * SP;
                double n = 0.0, d = 0.0;
                for (int a = 0; a < S; a++) { d += v[a]; n += v[a] * y[a]; }
                N[tid] += w * n;
                D[tid] += w * d;
            }
        }
    }
    if (tid < nPat) ratios[(size_t)cand.slot * g.P + p0 + tid] = rgRatio(N[tid], D[tid], scale, scaleRaw, patternWeights, p0 + tid, fpError);
}

// 4 states (the plain layout): one thread per pattern, everything in registers.  A pattern's four doubles of a partial are one
// 32-byte run, so a wave reads 2 KiB in a row; the 4 x 4 matrices are wave-uniform loads.  The same sums in the same order as
// k_regraftRatios.
typedef double Rg4Vector __attribute__((ext_vector_type(4)));       // a pattern's four states: 32 bytes, 32-byte aligned in every buffer

__device__ __forceinline__ void rg4Load(double* y, const void* src, bool compact, int c, int P, int p) {
    if (compact) {
        const int st = (int)gptr(reinterpret_cast<const uint8_t*>(src))[p];
        for (int b = 0; b < 4; b++) y[b] = (st >= 4 || st == b) ? 1.0 : 0.0;
    } else {
        const Rg4Vector v = gptr(reinterpret_cast<const Rg4Vector*>(src))[(size_t)c * P + p];
        y[0] = v[0]; y[1] = v[1]; y[2] = v[2]; y[3] = v[3];
    }
}

__global__ __launch_bounds__(RG_THREADS) void k_regraftRatios4(const PlacementCandidate* __restrict__ cands, const double* __restrict__ catWeights,
                                                               const double* __restrict__ pendants, size_t perVector,
                                                               const double* __restrict__ scale, int scaleRaw,
                                                               const double* __restrict__ patternWeights, int P, int C,
                                                               double* __restrict__ ratios, unsigned* __restrict__ fpError) {
    const int p = (int)blockIdx.x * RG_THREADS + (int)threadIdx.x;
    if (p >= P) return;
    const PlacementCandidate cand = cands[blockIdx.y];
    const double* q = pendants + (size_t)cand.pendant * perVector;
    double N = 0.0, D = 0.0;
    for (int c = 0; c < C; c++) {
        double u[4], t[4], y[4];
        rg4Load(u, cand.pre, false, c, P, p);
        if (cand.sib) {
            rg4Load(y, cand.sib, cand.sibStates != 0, c, P, p);
            const double MI355_GLOBAL* M = gptr(cand.mSib) + c * 16;
            for (int a = 0; a < 4; a++) {
                double acc = 0.0;
                for (int b = 0; b < 4; b++) acc += M[a * 4 + b] * y[b];
                u[a] *= acc;
            }
        }
        if (cand.mUp) {
            const double MI355_GLOBAL* M = gptr(cand.mUp) + c * 16;
            for (int a = 0; a < 4; a++) {
                double acc = 0.0;
                for (int b = 0; b < 4; b++) acc += u[b] * M[b * 4 + a];
                t[a] = acc;
            }
        } else {
            for (int a = 0; a < 4; a++) t[a] = u[a];
        }
        rg4Load(y, cand.child, cand.childStates != 0, c, P, p);
        const double MI355_GLOBAL* M = gptr(cand.mLow) + c * 16;
        double e[4];
        for (int a = 0; a < 4; a++) {
            double acc = 0.0;
            for (int b = 0; b < 4; b++) acc += M[a * 4 + b] * y[b];
            e[a] = t[a] * acc;
        }
        rg4Load(y, q, false, c, P, p);
        double n = 0.0, d = 0.0;
        for (int a = 0; a < 4; a++) { d += e[a]; n += e[a] * y[a]; }
        const double w = catWeights[c];
        N += w * n;
        D += w * d;
    }
    ratios[(size_t)cand.slot * P + p] = rgRatio(N, D, scale, scaleRaw, patternWeights, p, fpError);
}

// A workgroup: one candidate, RG_TILE_SEGMENTS segments.  The products w_p R[p] go to LDS as they lie in memory (0.0 for a pattern of
// weight 0 or past the end: adding 0.0 to an accumulator that started at 0.0 leaves its bits, so this IS leaving the pattern out);
// then a thread per segment adds its row in ascending order.
constexpr int RG_TILE_SEGMENTS = 64;

__global__ __launch_bounds__(RG_THREADS) void k_regraftSegments(const double* __restrict__ ratios, const double* __restrict__ patternWeights,
                                                                int nCands, int P, int nSegments, double* __restrict__ partial) {
    __shared__ double wr[RG_TILE_SEGMENTS][REGRAFT_SEGMENT + 1];
    const int tid = threadIdx.x, k = (int)blockIdx.y;
    const int s0 = (int)blockIdx.x * RG_TILE_SEGMENTS;
    const size_t pBase = (size_t)s0 * REGRAFT_SEGMENT;
    const double* row = ratios + (size_t)k * P;
    for (int e = tid; e < RG_TILE_SEGMENTS * REGRAFT_SEGMENT; e += RG_THREADS) {
        const size_t p = pBase + e;
        double v = 0.0;
        if (p < (size_t)P) { const double w = patternWeights[p]; if (w != 0.0) v = w * row[p]; }
        wr[e / REGRAFT_SEGMENT][e % REGRAFT_SEGMENT] = v;
    }
    __syncthreads();
    if (tid >= RG_TILE_SEGMENTS || s0 + tid >= nSegments) return;
    double acc = 0.0;
    for (int j = 0; j < REGRAFT_SEGMENT; j++) acc += wr[tid][j];
    partial[(size_t)(s0 + tid) * nCands + k] = acc;
}

__global__ __launch_bounds__(RG_THREADS) void k_regraftScoreSum(const double* __restrict__ partial, int nSegments, int nCands, double* __restrict__ scores) {
    const int k = (int)blockIdx.x * RG_THREADS + (int)threadIdx.x;
    if (k >= nCands) return;
    double acc = 0.0;
#pragma unroll 8
    for (int s = 0; s < nSegments; s++) acc += partial[(size_t)s * nCands + k];
    scores[k] = acc;
}

size_t rgLdsBytes(int S, int PB, bool mlds) {
    const size_t SP = (size_t)(S | 1);
    return ((size_t)PB * (2 * SP + 2) + (mlds ? (size_t)S * S : 0)) * sizeof(double);
}

bool rgMatrixInLds(int S) { return (size_t)S * S * sizeof(double) <= (size_t)RG_MATRIX_LDS_BYTES; }

}  // namespace

int regraftPatternBlock(int S) {
    for (int pb = 64; pb >= 8; pb >>= 1) if (rgLdsBytes(S, pb, rgMatrixInLds(S)) <= 160 * 1024) return pb;
    return 0;
}

void launchRegraftPendants(hipStream_t stream, const double* matrices, const int* dSlots, int nSlots, const void* subtree, bool subtreeStates,
                           int P, int S, int C, bool tiled, double* out) {
    const size_t n = (size_t)nSlots * C * P * S, perVector = regraftPendantDoubles(P, S, C, tiled);
    if (!n) return;
    const dim3 grid((unsigned)((n + RG_THREADS - 1) / RG_THREADS)), block(RG_THREADS);
    if (tiled) hipLaunchKernelGGL(k_regraftPendants<true>, grid, block, 0, stream, matrices, dSlots, nSlots, subtree, (int)subtreeStates, P, S, C, perVector, out);
    else hipLaunchKernelGGL(k_regraftPendants<false>, grid, block, 0, stream, matrices, dSlots, nSlots, subtree, (int)subtreeStates, P, S, C, perVector, out);
}

bool launchRegraftRatios(hipStream_t stream, const PlacementCandidate* dCands, int nCands, const double* catWeights, const double* pendants,
                         const double* scale, bool scaleRaw, const double* patternWeights, int P, int S, int C, bool tiled, double* ratios,
                         unsigned* fpError) {
    if (nCands <= 0 || P <= 0) return true;
    if (nCands > REGRAFT_MAX_CANDIDATES) return false;
    const size_t perVector = regraftPendantDoubles(P, S, C, tiled);
    if (S == 4 && !tiled) {
        hipLaunchKernelGGL(k_regraftRatios4, dim3((unsigned)((P + RG_THREADS - 1) / RG_THREADS), (unsigned)nCands), dim3(RG_THREADS), 0, stream,
                           dCands, catWeights, pendants, perVector, scale, (int)scaleRaw, patternWeights, P, C, ratios, fpError);
        return true;
    }
    const int PB = regraftPatternBlock(S);
    if (PB == 0 || (tiled && PB < 32)) return false;
    const bool mlds = rgMatrixInLds(S);
    const RgShape g = {P, S, C, PB, S | 1};
    const size_t lds = rgLdsBytes(S, PB, mlds);
    const dim3 grid((unsigned)((P + PB - 1) / PB), (unsigned)nCands), block(RG_THREADS);
#define RG_LAUNCH(T, M)                                                                                                          \
    do {                                                                                                                         \
        if (!grantDynamicLds(reinterpret_cast<const void*>(k_regraftRatios<T, M>), 160 * 1024)) return false;                    \
        hipLaunchKernelGGL((k_regraftRatios<T, M>), grid, block, lds, stream, dCands, catWeights, pendants, perVector, scale,    \
                           (int)scaleRaw, patternWeights, g, ratios, fpError);                                                   \
    } while (0)
    if (tiled) { if (mlds) RG_LAUNCH(true, true); else RG_LAUNCH(true, false); }
    else { if (mlds) RG_LAUNCH(false, true); else RG_LAUNCH(false, false); }
#undef RG_LAUNCH
    return true;
}

void launchRegraftScores(hipStream_t stream, const double* ratios, const double* patternWeights, int nCands, int P, double* partial,
                         double* scores) {
    if (nCands <= 0 || P <= 0) return;
    const int segments = regraftSegments(P);
    const dim3 grid((unsigned)((segments + RG_TILE_SEGMENTS - 1) / RG_TILE_SEGMENTS), (unsigned)nCands), block(RG_THREADS);
    hipLaunchKernelGGL(k_regraftSegments, grid, block, 0, stream, ratios, patternWeights, nCands, P, segments, partial);
    hipLaunchKernelGGL(k_regraftScoreSum, dim3((unsigned)((nCands + RG_THREADS - 1) / RG_THREADS)), block, 0, stream, partial, segments, nCands, scores);
}

}  // namespace mi355
