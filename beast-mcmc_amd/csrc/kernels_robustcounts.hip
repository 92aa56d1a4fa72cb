// kernels_robustcounts.hip — codon robust counting (beagleMi355RobustCounts, beagleMi355SimulateUnconditionedCounts).
//
// What it restates (reference = /root/reference): CodonPartitionedRobustCounting.computeExpectedCountsForBranch / the per-site
// gather (src/dr/evomodel/substmodel/CodonPartitionedRobustCounting.java:216-307) over MarkovJumpsCore
// .computeCondStatMarkovJumpsPrecompute (src/dr/inference/markovjumps/MarkovJumpsCore.java:84-103, 198-221) on the 64-state product
// chain of three nucleotide models, whose transition probabilities are BaseSubstitutionModel.getTransitionProbabilities' own
// (src/dr/evomodel/substmodel/BaseSubstitutionModel.java:206-240); and StateHistory.simulateUnconditionalOnEndingState
// (src/dr/inference/markovjumps/StateHistory.java:324-354) as fillInUnconditionalTraitValues uses it (:619-647).
//
// Four stages for the counts: the registers (k_robustRegisters: rateReg_k = Q o R_k from the SUPPLIED Q, M_k = U^-1 (rateReg_k U)),
// the conditional tables Cond[k][r][64][64] = (U ((A o M_k) U^-1)) / |U (diag(e^(lambda tau)) U^-1)| (k_robustTables: one
// workgroup per (register, row), three 64 x 64 operands in 96 KiB of LDS), the per-site gather over three state arrays
// (k_robustSites: one thread per site walks the rows; per-row totals through a fixed reduction tree) and k_blockTotals
// (kernels_markovjumps.hip) over the workgroups in ascending order.  No float atomics: two identical calls give identical bits.
//
// Every product is rounded on its own (no FMA contraction in this file) and every sum runs over its index in ascending order
// from 0.0, as the host restatement (tests/robust_counting_reference.py) forms it: the two differ only where exp() does.
#pragma clang fp contract(off)

#include "kernels.h"
#include "ancestral_draw.h"
#include "jump_aux.h"

namespace mi355 {

namespace {

constexpr int S64 = ROBUST_STATES;
constexpr int SS64 = S64 * S64;

// One workgroup per register: rr = Q o R_k (diagonal 0), tmp = rr U, M = U^-1 tmp (all [K][64][64] in global scratch; the phases
// of one workgroup meet at barriers) — k_jumpRegisters with the caller's Q.
__global__ __launch_bounds__(256) void k_robustRegisters(const double* __restrict__ eigen, const double* __restrict__ Q,
                                                         const double* __restrict__ registers, double* __restrict__ rr,
                                                         double* __restrict__ tmp, double* __restrict__ M) {
    const int k = blockIdx.x;
    const double* U = eigen;
    const double* Ui = U + SS64;
    const double* R = registers + (size_t)k * SS64;
    double* rk = rr + (size_t)k * SS64;
    double* tk = tmp + (size_t)k * SS64;
    double* mk = M + (size_t)k * SS64;
    for (int e = threadIdx.x; e < SS64; e += blockDim.x) {
        const int i = e / S64, j = e - i * S64;
        rk[e] = Q[e] * (i == j ? 0.0 : R[e]);
    }
    __syncthreads();
    for (int e = threadIdx.x; e < SS64; e += blockDim.x) {
        const int i = e / S64, j = e - i * S64;
        double s = 0.0;
        for (int b = 0; b < S64; b++) s = s + rk[i * S64 + b] * U[b * S64 + j];
        tk[e] = s;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < SS64; e += blockDim.x) {
        const int i = e / S64, j = e - i * S64;
        double s = 0.0;
        for (int a = 0; a < S64; a++) s = s + Ui[i * S64 + a] * tk[a * S64 + j];
        mk[e] = s;
    }
}

// One workgroup of 256 threads per (register k, row r >= 1).  LDS: T = A o M_k, Y = diag(e^(lambda tau)) U^-1, X = T U^-1, each
// 64 x 64 doubles.  A thread forms one 4 x 4 block of X, then the same block of J = U X and of U Y from one pass over U's rows
// (eight loads of U per thirty-two products); every entry sums over its inner index in ascending order.
__global__ __launch_bounds__(256) void k_robustTables(const RobustRow* __restrict__ rows, int nRows, const double* __restrict__ eigen,
                                                      const double* __restrict__ M, double* __restrict__ cond) {
    __shared__ double T[SS64];
    __shared__ double X[SS64];
    __shared__ double Y[SS64];
    __shared__ double ex[S64];
    const int r = 1 + blockIdx.x, k = blockIdx.y;
    const double tau = rows[r].tau;
    const double* U = eigen;
    const double* Ui = U + SS64;
    const double* lam = Ui + SS64;
    const double* Mk = M + (size_t)k * SS64;
    double* out = cond + ((size_t)k * nRows + r) * SS64;
    if (threadIdx.x < S64) ex[threadIdx.x] = exp(lam[threadIdx.x] * tau);
    __syncthreads();
    for (int e = threadIdx.x; e < SS64; e += 256) {
        const int a = e >> 6, b = e & 63;
        T[e] = auxInt(lam[a], lam[b], ex[a], ex[b], tau) * Mk[e];
        Y[e] = ex[a] * Ui[e];
    }
    __syncthreads();
    const int i0 = 4 * (threadIdx.x >> 4), j0 = 4 * (threadIdx.x & 15);
    {
        double acc[4][4] = {{0.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0}};
        for (int q = 0; q < S64; q++) {
            double w[4], v[4];
#pragma unroll
            for (int c = 0; c < 4; c++) { w[c] = T[(i0 + c) * S64 + q]; v[c] = Ui[q * S64 + j0 + c]; }
#pragma unroll
            for (int a = 0; a < 4; a++)
#pragma unroll
                for (int c = 0; c < 4; c++) acc[a][c] = acc[a][c] + w[a] * v[c];
        }
#pragma unroll
        for (int a = 0; a < 4; a++)
#pragma unroll
            for (int c = 0; c < 4; c++) X[(i0 + a) * S64 + j0 + c] = acc[a][c];
    }
    __syncthreads();
    double J[4][4] = {{0.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0}};
    double Pm[4][4] = {{0.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0}};
    for (int q = 0; q < S64; q++) {
        double w[4], x[4], y[4];
#pragma unroll
        for (int c = 0; c < 4; c++) { w[c] = U[(i0 + c) * S64 + q]; x[c] = X[q * S64 + j0 + c]; y[c] = Y[q * S64 + j0 + c]; }
#pragma unroll
        for (int a = 0; a < 4; a++)
#pragma unroll
            for (int c = 0; c < 4; c++) {
                J[a][c] = J[a][c] + w[a] * x[c];
                Pm[a][c] = Pm[a][c] + w[a] * y[c];
            }
    }
#pragma unroll
    for (int a = 0; a < 4; a++)
#pragma unroll
        for (int c = 0; c < 4; c++) out[(i0 + a) * S64 + j0 + c] = J[a][c] / fabs(Pm[a][c]);
}

constexpr int SITE_ROWS = 32;      // rows whose per-wave totals wait in LDS between two combines

// One thread per site walks rows [r0, r1): value = Cond[k][r][codon(parent)][codon(r)], codon = s0 * 16 + s1 * 4 + s2.  `counts`
// (may be nullptr): [K][r1 - r0][P]; `siteTotals` [K][P] carries the running sums over the INCLUDED rows from one chunk of rows to
// the next (r0 == 0: start from 0); `blockPartials` [block][K][nRows]: the workgroup's sum per row, included or not — wave sums
// by a fixed xor-shuffle tree, the four waves added in wave order (k_jumpSites' shape).
__global__ __launch_bounds__(256) void k_robustSites(const RobustRow* __restrict__ rows, int nRows, int r0, int r1,
                                                     const uint8_t* __restrict__ s0, const uint8_t* __restrict__ s1,
                                                     const uint8_t* __restrict__ s2, const double* __restrict__ cond, int K, int P,
                                                     double* __restrict__ counts, double* __restrict__ siteTotals,
                                                     double* __restrict__ blockPartials, unsigned* __restrict__ fpError) {
    __shared__ double part[4][MAX_JUMP_REGISTERS][SITE_ROWS];
    const int p = blockIdx.x * 256 + threadIdx.x;
    const bool live = p < P;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double tot[MAX_JUMP_REGISTERS];
#pragma unroll
    for (int k = 0; k < MAX_JUMP_REGISTERS; k++) tot[k] = (k < K && live && r0 > 0) ? siteTotals[(size_t)k * P + p] : 0.0;
    bool bad = false;
    for (int rb = r0; rb < r1; rb += SITE_ROWS) {
        const int re = rb + SITE_ROWS < r1 ? rb + SITE_ROWS : r1;
        for (int r = rb; r < re; r++) {
            double v[MAX_JUMP_REGISTERS];
            bool include = false;
            if (r == 0 || !live) {
#pragma unroll
                for (int k = 0; k < MAX_JUMP_REGISTERS; k++) v[k] = 0.0;
            } else {
                const RobustRow row = rows[r];
                include = row.include != 0;
                const size_t a = (size_t)row.parent * P + p, b = (size_t)r * P + p;
                const int i = ((s0[a] & 3) << 4) | ((s1[a] & 3) << 2) | (s2[a] & 3);
                const int j = ((s0[b] & 3) << 4) | ((s1[b] & 3) << 2) | (s2[b] & 3);
                const size_t off = (size_t)r * SS64 + (size_t)i * S64 + j;
#pragma unroll
                for (int k = 0; k < MAX_JUMP_REGISTERS; k++) {
                    v[k] = k < K ? cond[(size_t)k * nRows * SS64 + off] : 0.0;
                    if (k < K && !isfinite(v[k])) bad = true;
                }
            }
#pragma unroll
            for (int k = 0; k < MAX_JUMP_REGISTERS; k++) {
                if (k >= K) break;
                if (live) {
                    if (include) tot[k] = tot[k] + v[k];
                    if (counts) counts[((size_t)k * (r1 - r0) + (r - r0)) * P + p] = v[k];
                }
                double w = v[k];
#pragma unroll
                for (int d = 32; d >= 1; d >>= 1) w = w + __shfl_xor(w, d, 64);
                if (lane == 0) part[wave][k][r - rb] = w;
            }
        }
        __syncthreads();
        for (int e = threadIdx.x; e < K * (re - rb); e += 256) {
            const int k = e / (re - rb), q = e - k * (re - rb);
            const double s = ((part[0][k][q] + part[1][k][q]) + part[2][k][q]) + part[3][k][q];
            blockPartials[((size_t)blockIdx.x * K + k) * nRows + rb + q] = s;
        }
        __syncthreads();
    }
    if (live) {
#pragma unroll
        for (int k = 0; k < MAX_JUMP_REGISTERS; k++)
            if (k < K) siteTotals[(size_t)k * P + p] = tot[k];
    }
    if (bad) atomicOr(fpError, 2u);
}

// One thread per (length row l = l0 + blockIdx.y, site); `values` (may be nullptr) holds rows lBase .. lBase + lRows - 1: StateHistory.simulateUnconditionalOnEndingState from a start state drawn
// from `freqs`.  Q sits in LDS; the registers are read where a jump lands.  u_0: start state; u_(2m+1): waiting time m;
// u_(2m+2): the state after it.
__global__ __launch_bounds__(256) void k_unconditioned(const double* __restrict__ Q, const double* __restrict__ freqs,
                                                       const double* __restrict__ lengths, int lengthCount, int lBase, int lRows,
                                                       int l0, int siteCount,
                                                       const double* __restrict__ registers, int K, int S, unsigned long long seed,
                                                       double* __restrict__ values, double* __restrict__ blockPartials,
                                                       unsigned* __restrict__ fpError) {
    __shared__ double q[SS64];
    __shared__ double part[4][MAX_JUMP_REGISTERS];
    const int SS = S * S;
    for (int e = threadIdx.x; e < SS; e += 256) q[e] = Q[e];
    __syncthreads();
    const int l = l0 + blockIdx.y, s = blockIdx.x * 256 + threadIdx.x;
    const bool live = s < siteCount;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double v[MAX_JUMP_REGISTERS];
#pragma unroll
    for (int k = 0; k < MAX_JUMP_REGISTERS; k++) v[k] = 0.0;
    unsigned flag = 0;
    if (live) {
        const double length = lengths[l];
        const unsigned long long z = draw::mix64(seed ^ 0xBB67AE8584CAA73Bull, (unsigned long long)l * (unsigned long long)siteCount + s);
        bool bad = false;
        int cur = draw::drawChoice([&](int i) { return freqs[i]; }, S, draw::ancestralUniform(z, 0), false, bad);
        if (bad) flag |= 1u;
        double t = 0.0;
        unsigned long long n = 1;
        int jumps = 0;
        while (!bad && t < length) {
            const double rate = -q[cur * S + cur];
            if (!(rate > 0.0)) break;
            t = t + (-1.0 * log(1.0 - draw::ancestralUniform(z, n))) / rate;
            if (t < length) {
                if (jumps == ROBUST_MAX_JUMPS) { flag |= 4u; break; }
                bool none = false;
                const int next = draw::drawChoice([&](int i) { return i == cur ? 0.0 : q[cur * S + i]; }, S,
                                                  draw::ancestralUniform(z, n + 1), false, none);
                if (none) { flag |= 1u; break; }     // (a row whose off-diagonal total is not finite and > 0)
#pragma unroll
                for (int k = 0; k < MAX_JUMP_REGISTERS; k++)
                    if (k < K) v[k] = v[k] + registers[(size_t)k * SS + cur * S + next];
                cur = next;
                jumps++;
            }
            n += 2;
        }
    }
#pragma unroll
    for (int k = 0; k < MAX_JUMP_REGISTERS; k++) {
        if (k >= K) break;
        if (live && values) values[((size_t)k * lRows + (l - lBase)) * siteCount + s] = v[k];
        double w = v[k];
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) w = w + __shfl_xor(w, d, 64);
        if (lane == 0) part[wave][k] = w;
    }
    __syncthreads();
    if (threadIdx.x < K) {
        const int k = threadIdx.x;
        blockPartials[((size_t)blockIdx.x * K + k) * lengthCount + l] = ((part[0][k] + part[1][k]) + part[2][k]) + part[3][k];
    }
    if (flag) atomicOr(fpError, flag);
}

}  // namespace

void launchRobustRegisters(hipStream_t stream, const double* eigen, const double* Q, const double* registers, int K, double* rr,
                           double* tmp, double* M) {
    hipLaunchKernelGGL(k_robustRegisters, dim3(K), dim3(256), 0, stream, eigen, Q, registers, rr, tmp, M);
}

void launchRobustTables(hipStream_t stream, const RobustRow* dRows, int nRows, const double* eigen, const double* M, int K,
                        double* cond) {
    if (nRows < 2) return;
    hipLaunchKernelGGL(k_robustTables, dim3((unsigned)(nRows - 1), (unsigned)K), dim3(256), 0, stream, dRows, nRows, eigen, M, cond);
}

void launchRobustSites(hipStream_t stream, const RobustRow* dRows, int nRows, int r0, int r1, const uint8_t* s0, const uint8_t* s1,
                       const uint8_t* s2, const double* cond, int K, int P, double* counts, double* siteTotals,
                       double* blockPartials, unsigned* fpError) {
    hipLaunchKernelGGL(k_robustSites, dim3((unsigned)jumpSiteBlocks(P)), dim3(256), 0, stream, dRows, nRows, r0, r1, s0, s1, s2, cond,
                       K, P, counts, siteTotals, blockPartials, fpError);
}

int unconditionedBlocks(int siteCount) { return (siteCount + 255) / 256; }

void launchUnconditioned(hipStream_t stream, const double* Q, const double* freqs, const double* lengths, int lengthCount, int l0,
                         int l1, int siteCount, const double* registers, int K, int S, unsigned long long seed, double* values,
                         double* blockPartials, unsigned* fpError) {
    for (int l = l0; l < l1; l += 65535) {           // (a grid's y extent)
        const int n = l1 - l < 65535 ? l1 - l : 65535;
        hipLaunchKernelGGL(k_unconditioned, dim3((unsigned)unconditionedBlocks(siteCount), (unsigned)n), dim3(256), 0, stream, Q, freqs,
                           lengths, lengthCount, l0, l1 - l0, l, siteCount, registers, K, S, seed, values, blockPartials, fpError);
    }
}

}  // namespace mi355
