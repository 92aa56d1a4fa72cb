// kernels_placement.hip — scores of attaching new sequences at candidate points of the tree, from resident partials and matrices
// (beagleMi355PlacementScores; kernels.h PlacementCandidate has the formula).
//
// What the reference does for it (src/dr/app/realtime/CheckPointTreeModifier.java:434-800 with SimpleDistanceMatrix.java:63-93): the
// closest existing taxon by p-distance and a height from ad-hoc rules.  The likelihood of the new sequence attached at a point of a
// branch is made of three partials the engine holds after a gradient pass — the parent's pre-order partial, the sibling's and the
// child's post-order partials — and four small matrices, so a whole (query x candidate) table is four stages:
//   k_pendantTables   G[m][c][a][x] = sum_b Mpend_c[a][b] codeTable[x][b], once per distinct pendant matrix of the list: tiny.
//   k_placementTable  T_k[p][x] = log(N_p,x / D_p) for a chunk of candidates.  A workgroup takes one candidate and one block of
//                     patterns (64; fewer where the state count leaves no LDS for 64).  Per category it sweeps the block's consecutive
//                     doubles of each of the three partials — neighbouring lanes read neighbouring doubles in either layout, as in
//                     k_nodePosterior — into LDS as [pattern][state], brings ONE matrix of ONE category into LDS at a time (four 61 x 61
//                     matrices of four categories do not fit together) and runs the mat-vecs with a wave's lanes on different patterns
//                     of the same row, so the matrix entry is a broadcast and the vector reads meet no bank twice (rows padded to an
//                     odd length).  N and D are added up over the categories in LDS; the logarithms leave element by element.
//   k_placementTable4 the same table at 4 states: a thread per pattern, registers and wave-uniform matrix loads, no barrier.
//   k_placementCounts n[q][p][x] (int32) from the site -> pattern map and the queries' codes: integer atomics, exact in any order.
//   k_placementScores score[q][k] = sum_j n[q][j] T_k[j] over j = p X + x: per segment of PLACEMENT_SEGMENT entries ONE accumulator
//                     per (q, k), ascending from 0.0, a term with n = 0 skipped; k_placementScoreSum adds the segments in ascending
//                     order from 0.0.  The order is a function of (P, codeCount) alone, whatever the chunking or the list.
// No atomics on values, nothing waits on another workgroup, plain stores only.
#include "kernels.h"

#include <algorithm>

namespace mi355 {

namespace {

constexpr int PL_THREADS = 256;
constexpr int PL_MATRIX_LDS_BYTES = 40 * 1024;       // a matrix (or pendant table) of one category is kept in LDS up to this size

struct PlShape { int P, S, C, X, PB, SP, XP, MW; };   // PB patterns per workgroup; SP, XP odd row lengths; MW = max(S, X)

// the block's PB patterns of category c of a partials buffer (or of a compact tip's states) into v [PB][SP]
template <bool TILED>
__device__ __forceinline__ void plLoadVector(double* v, const void* src, bool compact, int c, int p0, int nPat, const PlShape& g) {
    const int tid = threadIdx.x, S = g.S, P = g.P;
    const int nElem = g.PB * S;
    const int inMemory = TILED ? min(g.PB, ((P + 31) >> 5) * 32 - p0) : nPat;
    const int nLoad = inMemory * S;
    const size_t stride = TILED ? (size_t)((P + 31) >> 5) * 32 * S : (size_t)P * S;
    const double MI355_GLOBAL* x = gptr(reinterpret_cast<const double*>(src)) + (size_t)c * stride + (size_t)p0 * S;
    const uint8_t MI355_GLOBAL* states = gptr(reinterpret_cast<const uint8_t*>(src));
    for (int e = tid; e < nElem; e += PL_THREADS) {
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

// rows x cols doubles of global memory into LDS, as they are
__device__ __forceinline__ void plLoadMatrix(double* m, const double* src, int n) {
    const double MI355_GLOBAL* x = gptr(src);
    for (int e = threadIdx.x; e < n; e += PL_THREADS) m[e] = x[e];
}

template <bool TILED, bool MLDS>
__global__ __launch_bounds__(PL_THREADS) void k_placementTable(const PlacementCandidate* __restrict__ cands, const double* __restrict__ catWeights,
                                                               const double* __restrict__ pendant, PlShape g, double* __restrict__ table,
                                                               unsigned* __restrict__ fpError) {
    extern __shared__ double plLds[];              // A [PB][SP] | B [PB][SP] | N [PB][XP] | D [PB] | matrix [S][MW] (MLDS)
    const int tid = threadIdx.x, S = g.S, X = g.X, PB = g.PB, SP = g.SP, XP = g.XP;
    double* A = plLds; double* B = A + PB * SP; double* N = B + PB * SP; double* D = N + PB * XP; double* ML = D + PB;
    const PlacementCandidate cand = cands[blockIdx.y];
    const int p0 = (int)blockIdx.x * PB, nPat = min(PB, g.P - p0);
    const size_t SS = (size_t)S * S;

    for (int e = tid; e < PB * XP; e += PL_THREADS) N[e] = 0.0;
    if (tid < PB) D[tid] = 0.0;

    for (int c = 0; c < g.C; c++) {
        double* t = A; double* other = B;
        // u = pre * (Msib post_sib)
        __syncthreads();                                                           // (the last category's readers are done)
        plLoadVector<TILED>(A, cand.pre, false, c, p0, nPat, g);
        if (cand.sib) {
            plLoadVector<TILED>(B, cand.sib, cand.sibStates != 0, c, p0, nPat, g);
            const double* Mg = cand.mSib + c * SS;
            if (MLDS) plLoadMatrix(ML, Mg, (int)SS);
            __syncthreads();
            const double MI355_GLOBAL* Mx = gptr(Mg);
            for (int e = tid; e < PB * S; e += PL_THREADS) {
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
            if (MLDS) { plLoadMatrix(ML, Mg, (int)SS); __syncthreads(); }
            const double MI355_GLOBAL* Mx = gptr(Mg);
            for (int e = tid; e < PB * S; e += PL_THREADS) {
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
            plLoadVector<TILED>(other, cand.child, cand.childStates != 0, c, p0, nPat, g);
            const double* Mg = cand.mLow + c * SS;
            if (MLDS) plLoadMatrix(ML, Mg, (int)SS);
            __syncthreads();
            const double MI355_GLOBAL* Mx = gptr(Mg);
            for (int e = tid; e < PB * S; e += PL_THREADS) {
                const int pl = e % PB, a = e / PB;
                const double* v = other + pl * SP;
                double acc = 0.0;
                for (int b = 0; b < S; b++) acc += (MLDS ? ML[a * S + b] : Mx[a * S + b]) * v[b];
                t[pl * SP + a] *= acc;
            }
            __syncthreads();
        }
        // N += w_c e G_c, D += w_c sum e
        {
            const double w = catWeights[c];
            const double* Gg = pendant + ((size_t)cand.pendant * g.C + c) * S * X;
            if (MLDS) { plLoadMatrix(ML, Gg, S * X); __syncthreads(); }
            const double MI355_GLOBAL* Gx = gptr(Gg);
            for (int e = tid; e < PB * X; e += PL_THREADS) {
                const int pl = e % PB, x = e / PB;
                const double* v = t + pl * SP;
                double acc = 0.0;
                for (int a = 0; a < S; a++) acc += v[a] * (MLDS ? ML[a * X + x] : Gx[a * X + x]);
                N[pl * XP + x] += w * acc;
            }
            if (tid < PB) {
                const double* v = t + tid * SP;
                double acc = 0.0;
                for (int a = 0; a < S; a++) acc += v[a];
                D[tid] += w * acc;
            }
        }
    }
    __syncthreads();
    double* out = table + ((size_t)cand.slot * g.P + p0) * X;
    for (int e = tid; e < nPat * X; e += PL_THREADS) {
        const int pl = e / X, x = e - pl * X;
        const double d = D[pl];
        double v;
        if (!(d != 0.0 && isfinite(d))) { v = NAN; *fpError = 1u; }
        else v = log(N[pl * XP + x] / d);
        out[e] = v;
    }
}

// 4 states (the plain layout; up to P4_MAX_CATEGORIES categories): one thread per pattern, everything in registers.  A pattern's four
// doubles of a partial are one 32-byte run, so a wave reads 2 KiB in a row; the 4 x 4 matrices are wave-uniform loads; e_c(a) is kept in
// the thread's own LDS column ([c][a][thread]: no barrier anywhere) for the pass over the codes.  The same sums in the same order as
// k_placementTable.  The general kernel at 4 states moves one element per thread between barriers and reads 0.6-0.7 TB/s.
constexpr int P4_MAX_CATEGORIES = 16;
typedef double Pl4Vector __attribute__((ext_vector_type(4)));       // a pattern's four states: 32 bytes, 32-byte aligned in every buffer

__device__ __forceinline__ void pl4Load(double* y, const void* src, bool compact, int c, int P, int p) {
    if (compact) {
        const int st = (int)gptr(reinterpret_cast<const uint8_t*>(src))[p];
        for (int b = 0; b < 4; b++) y[b] = (st >= 4 || st == b) ? 1.0 : 0.0;
    } else {
        const Pl4Vector v = gptr(reinterpret_cast<const Pl4Vector*>(src))[(size_t)c * P + p];
        y[0] = v[0]; y[1] = v[1]; y[2] = v[2]; y[3] = v[3];
    }
}

__global__ __launch_bounds__(PL_THREADS) void k_placementTable4(const PlacementCandidate* __restrict__ cands, const double* __restrict__ catWeights,
                                                                const double* __restrict__ pendant, int P, int C, int X,
                                                                double* __restrict__ table, unsigned* __restrict__ fpError) {
    extern __shared__ double pl4Lds[];             // e [C][4][threads]
    const int tid = threadIdx.x, p = (int)blockIdx.x * PL_THREADS + tid;
    const bool live = p < P;
    const int pp = live ? p : P - 1;                                               // (threads past the end redo the last pattern and write nothing)
    const PlacementCandidate cand = cands[blockIdx.y];
    double D = 0.0;
    for (int c = 0; c < C; c++) {
        double u[4], t[4], y[4];
        pl4Load(u, cand.pre, false, c, P, pp);
        if (cand.sib) {
            pl4Load(y, cand.sib, cand.sibStates != 0, c, P, pp);
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
        pl4Load(y, cand.child, cand.childStates != 0, c, P, pp);
        const double MI355_GLOBAL* M = gptr(cand.mLow) + c * 16;
        double d = 0.0;
        for (int a = 0; a < 4; a++) {
            double acc = 0.0;
            for (int b = 0; b < 4; b++) acc += M[a * 4 + b] * y[b];
            const double e = t[a] * acc;
            pl4Lds[(c * 4 + a) * PL_THREADS + tid] = e;
            d += e;
        }
        D += catWeights[c] * d;
    }
    const bool bad = !(D != 0.0 && isfinite(D));
    if (!live) return;
    if (bad) *fpError = 1u;
    double* out = table + ((size_t)cand.slot * P + p) * X;
    const double MI355_GLOBAL* G = gptr(pendant) + (size_t)cand.pendant * C * 4 * X;
    for (int x = 0; x < X; x++) {
        double N = 0.0;
        for (int c = 0; c < C; c++) {
            double acc = 0.0;
            for (int a = 0; a < 4; a++) acc += pl4Lds[(c * 4 + a) * PL_THREADS + tid] * G[(size_t)(c * 4 + a) * X + x];
            N += catWeights[c] * acc;
        }
        out[x] = bad ? NAN : log(N / D);
    }
}

__global__ __launch_bounds__(PL_THREADS) void k_pendantTables(const double* __restrict__ matrices, const int* __restrict__ slots, int nSlots,
                                                              const double* __restrict__ codeTable, int S, int C, int X,
                                                              double* __restrict__ out) {
    const size_t n = (size_t)nSlots * C * S * X, i = (size_t)blockIdx.x * PL_THREADS + threadIdx.x;
    if (i >= n) return;
    const int x = (int)(i % X), a = (int)(i / X % S), c = (int)(i / X / S % C), m = (int)(i / X / S / C);
    const double* row = matrices + ((size_t)slots[m] * C + c) * S * S + (size_t)a * S;
    const double* code = codeTable + (size_t)x * S;
    double acc = 0.0;
    for (int b = 0; b < S; b++) acc += row[b] * code[b];
    out[i] = acc;
}

__global__ __launch_bounds__(PL_THREADS) void k_placementCounts(const int* __restrict__ sitePatterns, const uint8_t* __restrict__ codes,
                                                                int nQueries, int siteCount, int P, int X, int* __restrict__ counts) {
    const size_t n = (size_t)nQueries * siteCount, i = (size_t)blockIdx.x * PL_THREADS + threadIdx.x;
    if (i >= n) return;
    const int q = (int)(i / siteCount), site = (int)(i - (size_t)q * siteCount);
    const int p = sitePatterns[site], x = (int)codes[i];
    if (p < 0 || p >= P || x >= X) return;                                        // (a skipped site, a missing code; the host has refused everything else)
    atomicAdd(counts + ((size_t)q * P + p) * X + x, 1);
}

// A workgroup: 16 candidates x 64 queries, four queries a thread; J runs over 64 entries of (pattern, code) at a time
constexpr int PS_K = 16, PS_Q = 64, PS_J = 64, PS_QT = PS_Q / 16;

__global__ __launch_bounds__(PL_THREADS) void k_placementScores(const int* __restrict__ counts, const double* __restrict__ table, int nQueries,
                                                                int nCands, size_t J, double* __restrict__ partial) {
    __shared__ double ts[PS_K][PS_J + 1];
    __shared__ int ns[PS_Q][PS_J + 1];
    const int tid = threadIdx.x, kl = tid & 15, ql = tid >> 4;
    const int k0 = (int)blockIdx.x * PS_K, q0 = (int)blockIdx.y * PS_Q;
    double acc[PS_QT];
    for (int r = 0; r < PS_QT; r++) acc[r] = 0.0;
    const size_t jBegin = (size_t)blockIdx.z * PLACEMENT_SEGMENT, jEnd = min(J, jBegin + PLACEMENT_SEGMENT);
    for (size_t j0 = jBegin; j0 < jEnd; j0 += PS_J) {
        const int nj = (int)min((size_t)PS_J, jEnd - j0);
        __syncthreads();
        for (int e = tid; e < PS_K * PS_J; e += PL_THREADS) {
            const int k = e / PS_J, j = e - k * PS_J;
            ts[k][j] = (k0 + k < nCands && j < nj) ? table[(size_t)(k0 + k) * J + j0 + j] : 0.0;
        }
        for (int e = tid; e < PS_Q * PS_J; e += PL_THREADS) {
            const int q = e / PS_J, j = e - q * PS_J;
            ns[q][j] = (q0 + q < nQueries && j < nj) ? counts[(size_t)(q0 + q) * J + j0 + j] : 0;
        }
        __syncthreads();
        for (int j = 0; j < PS_J; j++) {
            const double t = ts[kl][j];
            for (int r = 0; r < PS_QT; r++) {
                const int n = ns[ql + 16 * r][j];
                if (n != 0) acc[r] += (double)n * t;                               // (an entry no site of the query uses never reaches its sum)
            }
        }
    }
    if (k0 + kl >= nCands) return;
    for (int r = 0; r < PS_QT; r++) {
        const int q = q0 + ql + 16 * r;
        if (q < nQueries) partial[((size_t)blockIdx.z * nQueries + q) * nCands + k0 + kl] = acc[r];
    }
}

__global__ __launch_bounds__(PL_THREADS) void k_placementScoreSum(const double* __restrict__ partial, int nSegments, size_t n, double* __restrict__ scores) {
    const size_t i = (size_t)blockIdx.x * PL_THREADS + threadIdx.x;
    if (i >= n) return;
    double acc = 0.0;
    for (int s = 0; s < nSegments; s++) acc += partial[(size_t)s * n + i];
    scores[i] = acc;
}

size_t plLdsBytes(int S, int X, int PB, bool mlds) {
    const size_t SP = (size_t)(S | 1), XP = (size_t)(X | 1);
    return ((size_t)PB * (2 * SP + XP + 1) + (mlds ? (size_t)S * std::max(S, X) : 0)) * sizeof(double);
}

}  // namespace

int placementPatternBlock(int S, int X) {
    const bool mlds = (size_t)S * std::max(S, X) * sizeof(double) <= (size_t)PL_MATRIX_LDS_BYTES;
    for (int pb = 64; pb >= 8; pb >>= 1) if (plLdsBytes(S, X, pb, mlds) <= 160 * 1024) return pb;
    return 0;
}

void launchPendantTables(hipStream_t stream, const double* matrices, const int* dSlots, int nSlots, const double* codeTable, int S, int C,
                         int X, double* out) {
    const size_t n = (size_t)nSlots * C * S * X;
    if (!n) return;
    hipLaunchKernelGGL(k_pendantTables, dim3((unsigned)((n + PL_THREADS - 1) / PL_THREADS)), dim3(PL_THREADS), 0, stream, matrices, dSlots, nSlots,
                       codeTable, S, C, X, out);
}

bool launchPlacementTable(hipStream_t stream, const PlacementCandidate* dCands, int nCands, const double* catWeights, const double* pendant,
                          int P, int S, int C, int X, bool tiled, double* table, unsigned* fpError) {
    if (nCands <= 0 || P <= 0) return true;
    if (S == 4 && !tiled && C <= P4_MAX_CATEGORIES && nCands <= PLACEMENT_MAX_CANDIDATES) {
        const size_t lds4 = (size_t)C * 4 * PL_THREADS * sizeof(double);
        if (!grantDynamicLds(reinterpret_cast<const void*>(k_placementTable4), 160 * 1024)) return false;
        hipLaunchKernelGGL(k_placementTable4, dim3((unsigned)((P + PL_THREADS - 1) / PL_THREADS), (unsigned)nCands), dim3(PL_THREADS), lds4, stream,
                           dCands, catWeights, pendant, P, C, X, table, fpError);
        return true;
    }
    const int PB = placementPatternBlock(S, X);
    if (nCands > PLACEMENT_MAX_CANDIDATES || PB == 0 || (tiled && PB < 32)) return false;
    const bool mlds = (size_t)S * std::max(S, X) * sizeof(double) <= (size_t)PL_MATRIX_LDS_BYTES;
    const PlShape g = {P, S, C, X, PB, S | 1, X | 1, std::max(S, X)};
    const size_t lds = plLdsBytes(S, X, PB, mlds);
    const dim3 grid((unsigned)((P + PB - 1) / PB), (unsigned)nCands), block(PL_THREADS);
#define PL_LAUNCH(T, M)                                                                                                          \
    do {                                                                                                                         \
        if (!grantDynamicLds(reinterpret_cast<const void*>(k_placementTable<T, M>), 160 * 1024)) return false;                   \
        hipLaunchKernelGGL((k_placementTable<T, M>), grid, block, lds, stream, dCands, catWeights, pendant, g, table, fpError);   \
    } while (0)
    if (tiled) { if (mlds) PL_LAUNCH(true, true); else PL_LAUNCH(true, false); }
    else { if (mlds) PL_LAUNCH(false, true); else PL_LAUNCH(false, false); }
#undef PL_LAUNCH
    return true;
}

void launchPlacementCounts(hipStream_t stream, const int* sitePatterns, const uint8_t* codes, int nQueries, int siteCount, int P, int X,
                           int* counts) {
    const size_t n = (size_t)nQueries * siteCount;
    if (!n) return;
    hipLaunchKernelGGL(k_placementCounts, dim3((unsigned)((n + PL_THREADS - 1) / PL_THREADS)), dim3(PL_THREADS), 0, stream, sitePatterns, codes,
                       nQueries, siteCount, P, X, counts);
}

int placementSegments(int P, int X) { return (int)(((size_t)P * X + PLACEMENT_SEGMENT - 1) / PLACEMENT_SEGMENT); }

void launchPlacementScores(hipStream_t stream, const int* counts, const double* table, int nQueries, int nCands, int P, int X, double* partial,
                           double* scores) {
    if (nQueries <= 0 || nCands <= 0) return;
    const int segments = placementSegments(P, X);
    const dim3 grid((unsigned)((nCands + PS_K - 1) / PS_K), (unsigned)((nQueries + PS_Q - 1) / PS_Q), (unsigned)segments), block(PL_THREADS);
    hipLaunchKernelGGL(k_placementScores, grid, block, 0, stream, counts, table, nQueries, nCands, (size_t)P * X, partial);
    const size_t n = (size_t)nQueries * nCands;
    hipLaunchKernelGGL(k_placementScoreSum, dim3((unsigned)((n + PL_THREADS - 1) / PL_THREADS)), block, 0, stream, partial, segments, n, scores);
}

}  // namespace mi355
