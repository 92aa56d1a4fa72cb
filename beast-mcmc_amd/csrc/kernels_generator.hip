// kernels_generator.hip — transition matrices straight from generators (beagleMi355UpdateTransitionMatricesFromGenerators,
// engine_generator.cpp): exp(Q d) by uniformization with scaling and squaring, no eigen system anywhere.  For generator g
//     mu = max_i -Q_ii (the host's scan),   B = Q / mu + I,   B^0 = I, B^1 = B, B^k = B^(k-1) B  (k = 2 .. 20),
// and for entry e and category c, with d = length_e * rate_c and x = mu d,
//     s = the smallest integer >= 0 with x 2^-s <= 1,   tau = x 2^-s,   w_0 = exp(-tau), w_k = w_(k-1) tau / k,
//     T = sum_{k = 0 .. 20} w_k B^k  (k upwards),   then s times T <- T T.
// B and every T are non-negative: nothing cancels, zeros of the structure stay zeros, d = 0 gives I to the bit.
//   k_generatorPowersSmall<S>  S <= 8: one generator per thread, B and the running power in registers (as k_eigenSmall)
//   k_generatorPowersBlock     9 <= S <= 64: one workgroup per generator (as k_uniformPowers, the grid over generators), B and the previous
//                              power in LDS, a 4 x 4 block of the next one per thread
//   k_generatorSmall<S>        S <= 8: one thread per (entry, category), T and its square in registers (as k_transition4)
//   k_generatorBlock<MFMA>     9 <= S <= 64: one workgroup per (entry, category); T and its square ping-pong in LDS, rows and columns
//                              padded with zeros to a multiple of 4 (zeros square to zeros) and the row stride 4 doubles longer than a
//                              row (a column of four rows then lies in sixteen different bank pairs).  The 21 table matrices stream
//                              from L2.  Squarings: from 16 states on v_mfma_f64_4x4x4_4b_f64 — a wave forms four 4 x 4 tiles of one
//                              tile row per instruction chain, the inner index four at a time in ascending tile order; below 16 states
//                              the 4 x 4 register blocking of k_transition with fused multiply-adds.
// The power tables are summed as k_uniformPowers sums: the inner index upwards from 0.0, every product rounded on its own (this file is
// compiled without FMA contraction; the fused operations of the combination and the squarings are written out).  Every sum has a fixed
// order; the only atomics are the two integer statistics words.  A matrix depends on (Q_g, length_e, rate_c) and on nothing else.
#pragma clang fp contract(off)

#include "kernels.h"

namespace mi355 {

namespace {

constexpr int GEN_BLOCK = 256;

// s and tau of x = mu d.  false: x is not finite or needs more than GENERATOR_MAX_SQUARINGS squarings — the matrix becomes NaN
__device__ __forceinline__ bool generatorScale(double x, int& s, double& tau) {
    s = 0; tau = x;
    if (!(x <= 1.79769313486231570815e308) || !(x >= -1.79769313486231570815e308)) return false;
    if (x <= 1.0) return true;
    int e;
    const double m = frexp(x, &e);                                  // x = m 2^e, 0.5 <= m < 1
    s = m == 0.5 ? e - 1 : e;
    if (s > GENERATOR_MAX_SQUARINGS) return false;
    tau = ldexp(x, -s);
    return true;
}

__device__ __forceinline__ void generatorWeights(double tau, double (&w)[GENERATOR_TERMS]) {
    w[0] = exp(-tau);
#pragma unroll
    for (int k = 1; k < GENERATOR_TERMS; k++) w[k] = w[k - 1] * tau / (double)k;
}

__device__ __forceinline__ void generatorCount(unsigned* __restrict__ stats, bool ok, int s) {
    if (!ok) atomicAdd(stats + 1, 1u);
    else if (s > 0) atomicMax(stats, (unsigned)s);
}

// ---- power tables --------------------------------------------------------------------------------------------------------------
template <int S>
__global__ __launch_bounds__(64) void k_generatorPowersSmall(double* __restrict__ tables, const double* __restrict__ Q,
                                                             const double* __restrict__ mu, int count) {
    const int g = blockIdx.x * 64 + threadIdx.x;
    if (g >= count) return;
    const double m = mu[g];
    const double* q = Q + (size_t)g * S * S;
    double* t = tables + (size_t)g * GENERATOR_TERMS * S * S;
    double B[S][S], P[S][S];
#pragma unroll
    for (int i = 0; i < S; i++)
#pragma unroll
        for (int j = 0; j < S; j++) {
            double b = q[i * S + j] / m;
            if (i == j) b += 1.0;
            B[i][j] = b; P[i][j] = b;
            t[i * S + j] = i == j ? 1.0 : 0.0;
            t[S * S + i * S + j] = b;
        }
    for (int k = 2; k < GENERATOR_TERMS; k++) {
        double N[S][S];
#pragma unroll
        for (int i = 0; i < S; i++)
#pragma unroll
            for (int j = 0; j < S; j++) {
                double sum = 0.0;
#pragma unroll
                for (int l = 0; l < S; l++) sum = sum + P[i][l] * B[l][j];
                N[i][j] = sum;
            }
#pragma unroll
        for (int i = 0; i < S; i++)
#pragma unroll
            for (int j = 0; j < S; j++) { P[i][j] = N[i][j]; t[(size_t)k * S * S + i * S + j] = N[i][j]; }
    }
}

// LDS of the block kernels, in doubles: two images [N][LD], N = S rounded up to a multiple of 4, LD = N + 4
__host__ __device__ inline int generatorPadded(int S) { return (S + 3) & ~3; }
__host__ __device__ inline size_t generatorLds(int S) { const size_t N = (size_t)generatorPadded(S); return 2 * N * (N + 4) * sizeof(double); }

// a[r][c] += sum_l L[i0 + r][l] R[l][j0 + c] on the padded images, l upwards, four steps' operands fetched together (rows of both images
// start on 32-byte boundaries, so a thread's four doubles of a row are one or two wide LDS reads).  The steps past S add 0 x 0: the same
// bits as stopping at S.  FUSED: fused multiply-adds; otherwise every product and every sum is rounded on its own.
template <bool FUSED>
__device__ __forceinline__ void generatorBlockProduct(double (&a)[4][4], const double* __restrict__ L, const double* __restrict__ R,
                                                      int N, int LD, int i0, int j0) {
    for (int l = 0; l < N; l += 4) {
        double w[4][4], v[4][4];
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const double* p = static_cast<const double*>(__builtin_assume_aligned(L + (size_t)(i0 + r) * LD + l, 32));
#pragma unroll
            for (int t = 0; t < 4; t++) w[r][t] = p[t];
        }
#pragma unroll
        for (int t = 0; t < 4; t++) {
            const double* p = static_cast<const double*>(__builtin_assume_aligned(R + (size_t)(l + t) * LD + j0, 32));
#pragma unroll
            for (int c = 0; c < 4; c++) v[t][c] = p[c];
        }
#pragma unroll
        for (int t = 0; t < 4; t++)
#pragma unroll
            for (int r = 0; r < 4; r++)
#pragma unroll
                for (int c = 0; c < 4; c++) a[r][c] = FUSED ? fma(w[r][t], v[t][c], a[r][c]) : a[r][c] + w[r][t] * v[t][c];
    }
}

__global__ __launch_bounds__(GEN_BLOCK) void k_generatorPowersBlock(double* __restrict__ tables, const double* __restrict__ Q,
                                                                    const double* __restrict__ mu, int S) {
    extern __shared__ __attribute__((aligned(32))) double sh[];
    const int N = generatorPadded(S), LD = N + 4, nb = N >> 2, tid = threadIdx.x;     // nb * nb <= 256: at most one block a thread
    double* B = sh;
    double* prev = sh + (size_t)N * LD;
    const int g = blockIdx.x;
    const double m = mu[g];
    const double* q = Q + (size_t)g * S * S;
    double* t = tables + (size_t)g * GENERATOR_TERMS * S * S;
    for (int e = tid; e < N * LD; e += GEN_BLOCK) {
        const int i = e / LD, j = e - i * LD;
        double b = 0.0;
        if (i < S && j < S) {
            b = q[i * S + j] / m;
            if (i == j) b += 1.0;
            t[i * S + j] = i == j ? 1.0 : 0.0;
            t[(size_t)S * S + i * S + j] = b;
        }
        B[e] = b; prev[e] = b;
    }
    __syncthreads();
    const int bi = tid / nb, bj = tid - bi * nb, i0 = 4 * bi, j0 = 4 * bj;
    const bool mine = tid < nb * nb;
    for (int k = 2; k < GENERATOR_TERMS; k++) {
        double a[4][4] = {{0.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0}};
        if (mine) generatorBlockProduct<false>(a, prev, B, N, LD, i0, j0);
        __syncthreads();                                           // (everyone has read the previous power)
        if (mine) {
            double* out = t + (size_t)k * S * S;
#pragma unroll
            for (int r = 0; r < 4; r++)
#pragma unroll
                for (int c = 0; c < 4; c++) {
                    prev[(i0 + r) * LD + j0 + c] = a[r][c];        // (rows and columns past S: sums of zeros)
                    if (i0 + r < S && j0 + c < S) out[(i0 + r) * S + j0 + c] = a[r][c];
                }
        }
        __syncthreads();
    }
}

// ---- matrices, S <= 8 ------------------------------------------------------------------------------------------------------------
template <int S>
__global__ __launch_bounds__(64) void k_generatorSmall(double* __restrict__ matrices, const double* __restrict__ rates,
                                                       const double* __restrict__ tables, const double* __restrict__ mu,
                                                       const int* __restrict__ dIdx, const double* __restrict__ dLen,
                                                       const int* __restrict__ dGen, const int* __restrict__ dRate,
                                                       unsigned* __restrict__ stats, int count, int C) {
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t >= count * C) return;
    const int u = t / C, c = t - u * C, g = dGen[u];
    const double dist = dLen[u] * rates[(size_t)dRate[u] * C + c];
    double* M = matrices + ((size_t)dIdx[u] * C + c) * S * S;
    int s; double tau;
    const bool ok = generatorScale(mu[g] * dist, s, tau);
    generatorCount(stats, ok, s);
    if (!ok) {
#pragma unroll
        for (int e = 0; e < S * S; e++) M[e] = NAN;
        return;
    }
    double w[GENERATOR_TERMS];
    generatorWeights(tau, w);
    const double* tab = tables + (size_t)g * GENERATOR_TERMS * S * S;
    double T[S][S];
#pragma unroll
    for (int i = 0; i < S; i++)
#pragma unroll
        for (int j = 0; j < S; j++) T[i][j] = w[0] * tab[i * S + j];
#pragma unroll
    for (int k = 1; k < GENERATOR_TERMS; k++)
#pragma unroll
        for (int i = 0; i < S; i++)
#pragma unroll
            for (int j = 0; j < S; j++) T[i][j] = fma(w[k], tab[k * S * S + i * S + j], T[i][j]);
    for (int q = 0; q < s; q++) {
        double N[S][S];
#pragma unroll
        for (int i = 0; i < S; i++)
#pragma unroll
            for (int j = 0; j < S; j++) {
                double sum = 0.0;
#pragma unroll
                for (int l = 0; l < S; l++) sum = fma(T[i][l], T[l][j], sum);
                N[i][j] = sum;
            }
#pragma unroll
        for (int i = 0; i < S; i++)
#pragma unroll
            for (int j = 0; j < S; j++) T[i][j] = N[i][j];
    }
#pragma unroll
    for (int i = 0; i < S; i++)
#pragma unroll
        for (int j = 0; j < S; j++) M[i * S + j] = T[i][j];
}

// ---- matrices, 9 <= S <= 64 -------------------------------------------------------------------------------------------------------
// out = in in on the padded images.  Lane map of v_mfma_f64_4x4x4_4b_f64 (kernels_mfma.hip): block b = (l >> 2) & 3,
// A_b[i = l & 3][k = l >> 4], B_b[k = l >> 4][j = l & 3], D_b[row = l >> 4][col = l & 3].  An item is (tile row it, four tile columns
// 4 jq + b): the four blocks share the A tile and take neighbouring B tiles.  A tile column past the last reads the last one's and is
// not stored.
__device__ __forceinline__ void generatorSquareMfma(double* __restrict__ out, const double* __restrict__ in, int N, int LD) {
    const int nt = N >> 2, nq = (nt + 3) >> 2, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = lane & 3, kk = lane >> 4, b = (lane >> 2) & 3;
    for (int item = wave; item < nt * nq; item += GEN_BLOCK / 64) {
        const int it = item / nq, jq = item - it * nq, jt = 4 * jq + b, jtc = jt < nt ? jt : nt - 1;
        const double* pa = in + (size_t)(4 * it + i) * LD + kk;                   // + 4 kt
        const double* pb = in + (size_t)kk * LD + 4 * jtc + i;                      // + 4 kt LD
        double acc = 0.0;
        for (int kt = 0; kt < nt; kt++) acc = __builtin_amdgcn_mfma_f64_4x4x4f64(pa[4 * kt], pb[(size_t)4 * kt * LD], acc, 0, 0, 0);
        if (jt < nt) out[(size_t)(4 * it + kk) * LD + 4 * jt + i] = acc;
    }
}

__device__ __forceinline__ void generatorSquareBlocked(double* __restrict__ out, const double* __restrict__ in, int N, int LD) {
    const int nb = N >> 2;
    for (int blk = threadIdx.x; blk < nb * nb; blk += blockDim.x) {
        const int bi = blk / nb, bj = blk - bi * nb, i0 = 4 * bi, j0 = 4 * bj;
        double a[4][4] = {{0.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0}};
        generatorBlockProduct<true>(a, in, in, N, LD, i0, j0);
#pragma unroll
        for (int r = 0; r < 4; r++)
#pragma unroll
            for (int c = 0; c < 4; c++) out[(i0 + r) * LD + j0 + c] = a[r][c];
    }
}

template <bool MFMA>
__global__ __launch_bounds__(MFMA ? GEN_BLOCK : 64) void k_generatorBlock(double* __restrict__ matrices, const double* __restrict__ rates,
                                                                          const double* __restrict__ tables, const double* __restrict__ mu,
                                                                          const int* __restrict__ dIdx, const double* __restrict__ dLen,
                                                                          const int* __restrict__ dGen, const int* __restrict__ dRate,
                                                                          unsigned* __restrict__ stats, int S, int C) {
    extern __shared__ __attribute__((aligned(32))) double sh[];
    const int N = generatorPadded(S), LD = N + 4, tid = threadIdx.x, nthreads = blockDim.x;
    const int u = blockIdx.x, c = blockIdx.y, g = dGen[u];
    const double dist = dLen[u] * rates[(size_t)dRate[u] * C + c];
    double* M = matrices + ((size_t)dIdx[u] * C + c) * S * S;
    int s; double tau;
    const bool ok = generatorScale(mu[g] * dist, s, tau);           // (the same in every thread)
    if (tid == 0) generatorCount(stats, ok, s);
    if (!ok) {
        for (int e = tid; e < S * S; e += nthreads) M[e] = NAN;
        return;
    }
    double w[GENERATOR_TERMS];
    generatorWeights(tau, w);
    const double* tab = tables + (size_t)g * GENERATOR_TERMS * S * S;
    double* cur = sh;
    double* nxt = sh + (size_t)N * LD;
    for (int e = tid; e < N * LD; e += nthreads) {
        const int i = e / LD, j = e - i * LD;
        double x = 0.0;
        if (i < S && j < S) {
            const double* p = tab + i * S + j;
            x = w[0] * p[0];
#pragma unroll
            for (int k = 1; k < GENERATOR_TERMS; k++) x = fma(w[k], p[(size_t)k * S * S], x);
        }
        cur[e] = x;
        nxt[e] = 0.0;                                               // (the padding of both images is zero from here on)
    }
    __syncthreads();
    for (int q = 0; q < s; q++) {
        if (MFMA) generatorSquareMfma(nxt, cur, N, LD); else generatorSquareBlocked(nxt, cur, N, LD);
        __syncthreads();
        double* swap = cur; cur = nxt; nxt = swap;
    }
    for (int e = tid; e < S * S; e += nthreads) { const int i = e / S, j = e - i * S; M[e] = cur[i * LD + j]; }
}

}  // namespace

bool launchGeneratorPowers(hipStream_t stream, double* tables, const double* Q, const double* mu, int count, int S) {
    if (count <= 0) return true;
    if (S < 1 || S > 64) return false;
    if (S <= 8) {
        const dim3 grid((unsigned)((count + 63) / 64)), block(64);
#define GENERATOR_SMALL(N) case N: hipLaunchKernelGGL((k_generatorPowersSmall<N>), grid, block, 0, stream, tables, Q, mu, count); break;
        switch (S) {
            GENERATOR_SMALL(1) GENERATOR_SMALL(2) GENERATOR_SMALL(3) GENERATOR_SMALL(4)
            GENERATOR_SMALL(5) GENERATOR_SMALL(6) GENERATOR_SMALL(7) GENERATOR_SMALL(8)
        }
#undef GENERATOR_SMALL
        return true;
    }
    const size_t lds = generatorLds(S);
    if (lds > 65536 && !grantDynamicLds(reinterpret_cast<const void*>(k_generatorPowersBlock), lds)) return false;
    hipLaunchKernelGGL(k_generatorPowersBlock, dim3((unsigned)count), dim3(GEN_BLOCK), lds, stream, tables, Q, mu, S);
    return true;
}

bool launchGeneratorMatrices(hipStream_t stream, double* matrices, const double* rates, const double* tables, const double* mu,
                             const int* dIdx, const double* dLen, const int* dGen, const int* dRate, unsigned* stats, int count, int S, int C) {
    if (count <= 0) return true;
    if (S < 1 || S > 64) return false;
    if (S <= 8) {
        const dim3 grid((unsigned)(((size_t)count * C + 63) / 64)), block(64);
#define GENERATOR_SMALL(N) case N: hipLaunchKernelGGL((k_generatorSmall<N>), grid, block, 0, stream, matrices, rates, tables, mu, dIdx, dLen, dGen, dRate, stats, count, C); break;
        switch (S) {
            GENERATOR_SMALL(1) GENERATOR_SMALL(2) GENERATOR_SMALL(3) GENERATOR_SMALL(4)
            GENERATOR_SMALL(5) GENERATOR_SMALL(6) GENERATOR_SMALL(7) GENERATOR_SMALL(8)
        }
#undef GENERATOR_SMALL
        return true;
    }
    const size_t lds = generatorLds(S);
    const dim3 grid((unsigned)count, (unsigned)C);
    if (S >= 16) {
        if (lds > 65536 && !grantDynamicLds(reinterpret_cast<const void*>(k_generatorBlock<true>), lds)) return false;
        hipLaunchKernelGGL(k_generatorBlock<true>, grid, dim3(GEN_BLOCK), lds, stream, matrices, rates, tables, mu, dIdx, dLen, dGen, dRate, stats, S, C);
    } else {
        hipLaunchKernelGGL(k_generatorBlock<false>, grid, dim3(64), lds, stream, matrices, rates, tables, mu, dIdx, dLen, dGen, dRate, stats, S, C);
    }
    return true;
}

}  // namespace mi355
