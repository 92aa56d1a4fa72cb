// kernels_markovjumps.hip — expected Markov-jump counts and rewards per branch and site (beagleMi355SampleMarkovJumps).
//
// What it restates (reference = /root/reference): MarkovJumpsBeagleTreeLikelihood.computeIntegratedMarkovJumpsForBranch
// (src/dr/evomodel/treelikelihood/MarkovJumpsBeagleTreeLikelihood.java:510-567) over MarkovJumpsCore
// .computeCondStatMarkovJumpsPrecompute (src/dr/inference/markovjumps/MarkovJumpsCore.java:84-103, 118-127, 198-221) and
// MarkovJumpsSubstitutionModel.setRegistration / makeRateRegistrationMatrix (src/dr/evomodel/substmodel/
// MarkovJumpsSubstitutionModel.java) with PRECOMPUTE.
//
// Three stages: the registers (k_jumpRegisters: Q, rateReg_k, M_k = U^-1 rateReg_k U), the conditional tables
// Cond[k][r][c][S][S] = (U ((A o M_k) U^-1)) / P_r[c] (k_jumpMatrices*: one per (register, row, category)), and the per-site
// gather (k_jumpSites: one thread per pattern walks the rows; per-row totals through a fixed reduction tree, then
// k_blockTotals over the workgroups in ascending order).  No float atomics: two identical calls give identical bits.
//
// Every product is rounded on its own (no FMA contraction in this file) and every sum runs over its index in ascending order
// from 0.0, as the host restatement (tests/markov_jumps_reference.py) forms it: the two differ only where exp() does.
#pragma clang fp contract(off)

#include "kernels.h"
#include "jump_aux.h"

namespace mi355 {

namespace {

// Q[i][j] = sum_a (U[i][a] lambda[a]) Uinv[a][j]
__device__ __forceinline__ double qEntry(const double* __restrict__ U, const double* __restrict__ Ui,
                                         const double* __restrict__ lam, int S, int i, int j) {
    double s = 0.0;
    for (int a = 0; a < S; a++) s = s + (U[(size_t)i * S + a] * lam[a]) * Ui[(size_t)a * S + j];
    return s;
}

// One workgroup per register: rr = rateReg_k, tmp = rateReg_k U, M = U^-1 tmp (all [K][S][S] in global scratch; the phases of
// one workgroup meet at barriers).
__global__ __launch_bounds__(256) void k_jumpRegisters(const double* __restrict__ eigen, const double* __restrict__ registers,
                                                       const int* __restrict__ regFlags, int S, double* __restrict__ rr,
                                                       double* __restrict__ tmp, double* __restrict__ M) {
    const int k = blockIdx.x;
    const size_t SS = (size_t)S * S;
    const double* U = eigen;
    const double* Ui = U + SS;
    const double* lam = Ui + SS;
    const double* R = registers + k * SS;
    const bool reward = (regFlags[k] & 1) != 0;
    double* rk = rr + k * SS;
    double* tk = tmp + k * SS;
    double* mk = M + k * SS;
    for (int e = threadIdx.x; e < (int)SS; e += blockDim.x) {
        const int i = e / S, j = e - i * S;
        if (reward) rk[e] = i == j ? R[e] : 0.0;
        else rk[e] = qEntry(U, Ui, lam, S, i, j) * (i == j ? 0.0 : R[e]);
    }
    __syncthreads();
    for (int e = threadIdx.x; e < (int)SS; e += blockDim.x) {
        const int i = e / S, j = e - i * S;
        double s = 0.0;
        for (int b = 0; b < S; b++) s = s + rk[(size_t)i * S + b] * U[(size_t)b * S + j];
        tk[e] = s;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < (int)SS; e += blockDim.x) {
        const int i = e / S, j = e - i * S;
        double s = 0.0;
        for (int a = 0; a < S; a++) s = s + Ui[(size_t)i * S + a] * tk[(size_t)a * S + j];
        mk[e] = s;
    }
}

// What a (k, r, c) shares: tau, the scale divisor, the zero-rate rule.  Returns false when rate_c <= 0 (the table is then 0, or
// branchTimes[r] on the diagonal for a reward register that scales by time).
struct JumpCell {
    double tau, scale;
    bool live, rewardTime;
    double time;
};
__device__ __forceinline__ JumpCell jumpCell(const JumpRow& row, double rateC, int flags) {
    JumpCell z;
    z.time = row.time;
    z.live = rateC > 0.0;
    z.tau = (row.time * row.rate) * rateC;
    z.scale = (flags & 2) ? row.rate * rateC : 0.0;
    z.rewardTime = (flags & 1) && (flags & 2);
    return z;
}
__device__ __forceinline__ double finishEntry(double J, double P, const JumpCell& z) {
    double v = J / P;
    if (z.scale != 0.0) v = v / z.scale;
    return v;
}
__device__ __forceinline__ double deadEntry(int i, int j, const JumpCell& z) { return z.rewardTime && i == j ? z.time : 0.0; }

// 4 states: one thread per (k, r, c), everything in registers (as k_transition4)
__global__ __launch_bounds__(256) void k_jumpMatrices4(const JumpRow* __restrict__ rows, int nRows, const double* __restrict__ eigen,
                                                       const double* __restrict__ rates, const double* __restrict__ M,
                                                       const int* __restrict__ regFlags, int K, int C, double* __restrict__ cond) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= K * (nRows - 1) * C) return;
    const int c = t % C, kr = t / C, r = 1 + kr % (nRows - 1), k = kr / (nRows - 1);
    const JumpRow row = rows[r];
    const JumpCell z = jumpCell(row, rates[c], regFlags[k]);
    double* out = cond + (((size_t)k * nRows + r) * C + c) * 16;
    if (!z.live) {
        for (int e = 0; e < 16; e++) out[e] = deadEntry(e >> 2, e & 3, z);
        return;
    }
    const double* U = eigen;
    const double* Ui = U + 16;
    const double* lam = U + 32;
    const double* Mk = M + (size_t)k * 16;
    const double* P = row.matrix + (size_t)c * 16;
    double ex[4], T[16], X[16];
    for (int a = 0; a < 4; a++) ex[a] = exp(lam[a] * z.tau);
    for (int a = 0; a < 4; a++)
        for (int b = 0; b < 4; b++) T[a * 4 + b] = auxInt(lam[a], lam[b], ex[a], ex[b], z.tau) * Mk[a * 4 + b];
    for (int a = 0; a < 4; a++)
        for (int j = 0; j < 4; j++) {
            double s = 0.0;
            for (int b = 0; b < 4; b++) s = s + T[a * 4 + b] * Ui[b * 4 + j];
            X[a * 4 + j] = s;
        }
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) {
            double s = 0.0;
            for (int a = 0; a < 4; a++) s = s + U[i * 4 + a] * X[a * 4 + j];
            out[i * 4 + j] = finishEntry(s, P[i * 4 + j], z);
        }
}

// C = L R for S x S operands, a thread forming 4 x 4 blocks of C (as k_transition: eight loads per sixteen products); every
// entry sums over k in ascending order.  L(i, k), R(k, j) read an operand; out(i, j, v) stores an entry.
template <class Lf, class Rf, class Of>
__device__ __forceinline__ void blockedProduct(int S, const Lf& L, const Rf& R, const Of& out) {
    const int nb = (S + 3) >> 2;
    for (int b = threadIdx.x; b < nb * nb; b += blockDim.x) {
        const int bi = b / nb, bj = b - bi * nb, i0 = 4 * bi, j0 = 4 * bj;
        int ii[4], jj[4];
#pragma unroll
        for (int q = 0; q < 4; q++) { ii[q] = i0 + q < S ? i0 + q : S - 1; jj[q] = j0 + q < S ? j0 + q : S - 1; }
        double acc[4][4] = {{0.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0}};
        for (int k = 0; k < S; k++) {
            double w[4], v[4];
#pragma unroll
            for (int q = 0; q < 4; q++) { w[q] = L(ii[q], k); v[q] = R(k, jj[q]); }
#pragma unroll
            for (int r = 0; r < 4; r++)
#pragma unroll
                for (int q = 0; q < 4; q++) acc[r][q] = acc[r][q] + w[r] * v[q];
        }
#pragma unroll
        for (int r = 0; r < 4; r++)
#pragma unroll
            for (int q = 0; q < 4; q++)
                if (i0 + r < S && j0 + q < S) out(i0 + r, j0 + q, acc[r][q]);
    }
}

// Up to 63 states (two S x S tables in 64 KiB of LDS): one workgroup per (k, r, c).  T = A o M_k and X = T U^-1 in LDS, then
// J = U X straight to the table.
__global__ __launch_bounds__(256) void k_jumpMatrices(const JumpRow* __restrict__ rows, int nRows, const double* __restrict__ eigen,
                                                      const double* __restrict__ rates, const double* __restrict__ M,
                                                      const int* __restrict__ regFlags, int S, int C, double* __restrict__ cond) {
    extern __shared__ double sh[];            // T[S][S] | X[S][S] | exp(lambda tau)[S]
    const int c = blockIdx.x % C, r = 1 + blockIdx.x / C, k = blockIdx.y;
    const size_t SS = (size_t)S * S;
    const JumpRow row = rows[r];
    const JumpCell z = jumpCell(row, rates[c], regFlags[k]);
    double* out = cond + (((size_t)k * nRows + r) * C + c) * SS;
    if (!z.live) {
        for (int e = threadIdx.x; e < (int)SS; e += blockDim.x) out[e] = deadEntry(e / S, e % S, z);
        return;
    }
    const double* U = eigen;
    const double* Ui = U + SS;
    const double* lam = Ui + SS;
    const double* Mk = M + (size_t)k * SS;
    const double* P = row.matrix + (size_t)c * SS;
    double* T = sh;
    double* X = sh + SS;
    double* ex = sh + 2 * SS;
    for (int a = threadIdx.x; a < S; a += blockDim.x) ex[a] = exp(lam[a] * z.tau);
    __syncthreads();
    for (int e = threadIdx.x; e < (int)SS; e += blockDim.x) {
        const int a = e / S, b = e - a * S;
        T[e] = auxInt(lam[a], lam[b], ex[a], ex[b], z.tau) * Mk[e];
    }
    __syncthreads();
    blockedProduct(S, [&](int i, int q) { return T[i * S + q]; }, [&](int q, int j) { return Ui[(size_t)q * S + j]; },
                   [&](int i, int j, double v) { X[i * S + j] = v; });
    __syncthreads();
    blockedProduct(S, [&](int i, int q) { return U[(size_t)i * S + q]; }, [&](int q, int j) { return X[q * S + j]; },
                   [&](int i, int j, double v) { out[(size_t)i * S + j] = finishEntry(v, P[(size_t)i * S + j], z); });
}

// More than 63 states: one workgroup per (k, r, c), only exp(lambda tau) in LDS.  X = (A o M_k) U^-1 one entry per thread into
// the table itself; then column by column, X's column j goes to LDS and the table's column j is overwritten with J's — no
// later column reads it.
__global__ __launch_bounds__(256) void k_jumpMatricesBig(const JumpRow* __restrict__ rows, int nRows, const double* __restrict__ eigen,
                                                         const double* __restrict__ rates, const double* __restrict__ M,
                                                         const int* __restrict__ regFlags, int S, int C, double* __restrict__ cond) {
    extern __shared__ double sh[];            // exp(lambda tau)[S] | X[.][j] [S]
    const int c = blockIdx.x % C, r = 1 + blockIdx.x / C, k = blockIdx.y;
    const size_t SS = (size_t)S * S;
    const JumpRow row = rows[r];
    const JumpCell z = jumpCell(row, rates[c], regFlags[k]);
    double* out = cond + (((size_t)k * nRows + r) * C + c) * SS;
    if (!z.live) {
        for (int e = threadIdx.x; e < (int)SS; e += blockDim.x) out[e] = deadEntry(e / S, e % S, z);
        return;
    }
    const double* U = eigen;
    const double* Ui = U + SS;
    const double* lam = Ui + SS;
    const double* Mk = M + (size_t)k * SS;
    const double* P = row.matrix + (size_t)c * SS;
    double* ex = sh;
    double* col = sh + S;
    for (int a = threadIdx.x; a < S; a += blockDim.x) ex[a] = exp(lam[a] * z.tau);
    __syncthreads();
    for (int e = threadIdx.x; e < (int)SS; e += blockDim.x) {
        const int a = e / S, j = e - a * S;
        double s = 0.0;
        for (int b = 0; b < S; b++) s = s + (auxInt(lam[a], lam[b], ex[a], ex[b], z.tau) * Mk[(size_t)a * S + b]) * Ui[(size_t)b * S + j];
        out[e] = s;
    }
    __syncthreads();
    for (int j = 0; j < S; j++) {
        for (int a = threadIdx.x; a < S; a += blockDim.x) col[a] = out[(size_t)a * S + j];
        __syncthreads();
        for (int i = threadIdx.x; i < S; i += blockDim.x) {
            double s = 0.0;
            for (int a = 0; a < S; a++) s = s + U[(size_t)i * S + a] * col[a];
            out[(size_t)i * S + j] = finishEntry(s, P[(size_t)i * S + j], z);
        }
        __syncthreads();
    }
}

constexpr int SITE_ROWS = 32;      // rows whose per-wave totals wait in LDS between two combines

// One thread per pattern walks rows [r0, r1): value = Cond[k][r][cat][state(parent)][state(r)].  `jumps` (may be nullptr):
// [K][r1 - r0][P]; `patternTotals` [K][P] carries the running sums from one chunk of rows to the next (r0 == 0: start from 0);
// `blockPartials` [block][K][nRows]: the workgroup's sum per row — wave sums by a fixed xor-shuffle tree, the four waves added
// in wave order.
__global__ __launch_bounds__(256) void k_jumpSites(const JumpRow* __restrict__ rows, int nRows, int r0, int r1,
                                                   const uint8_t* __restrict__ states, const int* __restrict__ cats,
                                                   const double* __restrict__ cond, int K, int S, int C, int P,
                                                   double* __restrict__ jumps, double* __restrict__ patternTotals,
                                                   double* __restrict__ blockPartials, unsigned* __restrict__ fpError) {
    __shared__ double part[4][MAX_JUMP_REGISTERS][SITE_ROWS];
    const int p = blockIdx.x * 256 + threadIdx.x;
    const bool live = p < P;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int cat = live ? cats[p] : 0;
    const size_t SS = (size_t)S * S;
    double tot[MAX_JUMP_REGISTERS];
#pragma unroll
    for (int k = 0; k < MAX_JUMP_REGISTERS; k++) tot[k] = (k < K && live && r0 > 0) ? patternTotals[(size_t)k * P + p] : 0.0;
    bool bad = false;
    for (int rb = r0; rb < r1; rb += SITE_ROWS) {
        const int re = rb + SITE_ROWS < r1 ? rb + SITE_ROWS : r1;
        for (int r = rb; r < re; r++) {
            double v[MAX_JUMP_REGISTERS];
            if (r == 0 || !live) {
#pragma unroll
                for (int k = 0; k < MAX_JUMP_REGISTERS; k++) v[k] = 0.0;
            } else {
                const int i = states[(size_t)rows[r].parent * P + p], j = states[(size_t)r * P + p];
                const size_t off = ((size_t)r * C + cat) * SS + (size_t)i * S + j;
#pragma unroll
                for (int k = 0; k < MAX_JUMP_REGISTERS; k++) {
                    v[k] = k < K ? cond[(size_t)k * nRows * C * SS + off] : 0.0;
                    if (k < K && !isfinite(v[k])) bad = true;
                }
            }
#pragma unroll
            for (int k = 0; k < MAX_JUMP_REGISTERS; k++) {
                if (k >= K) break;
                if (live) {
                    tot[k] = tot[k] + v[k];
                    if (jumps) jumps[((size_t)k * (r1 - r0) + (r - r0)) * P + p] = v[k];
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
            if (k < K) patternTotals[(size_t)k * P + p] = tot[k];
    }
    if (bad) atomicOr(fpError, 2u);
}

// out[k][r] = sum over the workgroups of a site kernel in ascending order (rows below firstRow: 0)
__global__ __launch_bounds__(256) void k_blockTotals(const double* __restrict__ blockPartials, int blocks, int K, int nRows,
                                                     int firstRow, double* __restrict__ out) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= K * nRows) return;
    const int k = t / nRows, r = t - k * nRows;
    double s = 0.0;
    if (r >= firstRow)
        for (int b = 0; b < blocks; b++) s = s + blockPartials[((size_t)b * K + k) * nRows + r];
    out[t] = s;
}

}  // namespace

void launchJumpRegisters(hipStream_t stream, const double* eigen, const double* registers, const int* regFlags, int K, int S,
                         double* rr, double* tmp, double* M) {
    hipLaunchKernelGGL(k_jumpRegisters, dim3(K), dim3(256), 0, stream, eigen, registers, regFlags, S, rr, tmp, M);
}

void launchJumpMatrices(hipStream_t stream, const JumpRow* dRows, int nRows, const double* eigen, const double* rates,
                        const double* M, const int* regFlags, int K, int S, int C, double* cond) {
    if (nRows < 2) return;
    if (S == 4) {
        const size_t n = (size_t)K * (nRows - 1) * C;
        hipLaunchKernelGGL(k_jumpMatrices4, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, dRows, nRows, eigen, rates, M,
                           regFlags, K, C, cond);
        return;
    }
    const dim3 grid((unsigned)((nRows - 1) * C), (unsigned)K);
    const size_t lds = (2 * (size_t)S * S + S) * sizeof(double);
    if (lds <= 64 * 1024) {
        hipLaunchKernelGGL(k_jumpMatrices, grid, dim3(S * S >= 256 ? 256 : 64), lds, stream, dRows, nRows, eigen, rates, M, regFlags,
                           S, C, cond);
        return;
    }
    hipLaunchKernelGGL(k_jumpMatricesBig, grid, dim3(256), 2 * (size_t)S * sizeof(double), stream, dRows, nRows, eigen, rates, M,
                       regFlags, S, C, cond);
}

int jumpSiteBlocks(int P) { return (P + 255) / 256; }

void launchJumpSites(hipStream_t stream, const JumpRow* dRows, int nRows, int r0, int r1, const uint8_t* states, const int* cats,
                     const double* cond, int K, int S, int C, int P, double* jumps, double* patternTotals, double* blockPartials,
                     unsigned* fpError) {
    hipLaunchKernelGGL(k_jumpSites, dim3((unsigned)jumpSiteBlocks(P)), dim3(256), 0, stream, dRows, nRows, r0, r1, states, cats, cond,
                       K, S, C, P, jumps, patternTotals, blockPartials, fpError);
}

void launchBlockTotals(hipStream_t stream, const double* blockPartials, int blocks, int K, int nRows, int firstRow, double* out) {
    const int n = K * nRows;
    hipLaunchKernelGGL(k_blockTotals, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, blockPartials, blocks, K, nRows,
                       firstRow, out);
}

}  // namespace mi355
