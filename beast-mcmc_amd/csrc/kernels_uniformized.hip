// kernels_uniformized.hip — sampled Markov-jump histories by uniformization (beagleMi355SampleMarkovJumpsUniformized).
//
// What it restates (reference = /root/reference): MarkovJumpsBeagleTreeLikelihood.computeSampledMarkovJumpsForBranch
// (src/dr/evomodel/treelikelihood/MarkovJumpsBeagleTreeLikelihood.java:473-509), UniformizedSubstitutionModel
// .computeCondStatMarkovJumps (src/dr/evomodel/substmodel/UniformizedSubstitutionModel.java, with RETURN_UNIFORMLY_DISTRIBUTED_EVENT),
// UniformizedStateHistory.simulateConditionalOnEndingState and SubordinatedProcess (src/dr/inference/markovjumps/), and
// MarkovJumpsSubstitutionModel.getProcessForSimulant.
//
// Four launches per call, and a fifth for the event list:
//   k_uniformPowers     one workgroup forms R^n = R^(n-1) R for n = 2 .. N-1 (MarkovJumpsCore.matrixMultiply order), the
//                       previous power and R in LDS when both fit;
//   k_uniformSites      one thread per (row, pattern) of a chunk of rows, lanes along patterns: every simulant's history, every
//                       register's value, the row's per-workgroup sums (fixed xor tree, then the four waves in order) and the
//                       number of real changes;
//   k_uniformPatternTotals  one thread per pattern adds the chunk's rows in row order onto the running totals;
//   k_eventRowOffsets + k_eventPatternScan  exclusive offsets of every (row, pattern)'s events in (pattern, row) order;
//   k_uniformSites<WRITE>   the same histories again (the draws are keyed, so nothing is stored in between), their events written.
// The row totals are launchBlockTotals' (kernels_markovjumps.hip) over the per-workgroup sums.
//
// A history never needs a per-thread array: the n + 1 exponential spacings whose running sums give the jump times are summed
// once for the total and recomputed from the keyed stream on the walk.  No float atomics; every product is rounded on its own (no
// FMA contraction in this file) and every sum runs in the order the host restatement (tests/uniformized_reference.py) uses.
#pragma clang fp contract(off)

#include "kernels.h"
#include "ancestral_draw.h"

namespace mi355 {

namespace {

using draw::ancestralUniform;
using draw::drawChoice;

// R^n for n = 2 .. N-1 into table[n] (table[0] = I and table[1] = R are the caller's).  LDS: R | previous power when they fit.
template <bool LDS>
__global__ __launch_bounds__(256) void k_uniformPowers(double* __restrict__ table, int S, int N) {
    extern __shared__ double sh[];
    const int SS = S * S;
    double* R = sh;
    double* prev = sh + SS;
    if (LDS)
        for (int e = threadIdx.x; e < SS; e += blockDim.x) { R[e] = table[SS + e]; prev[e] = table[SS + e]; }
    __syncthreads();
    for (int n = 2; n < N; n++) {
        const double* A = LDS ? prev : table + (size_t)(n - 1) * SS;
        const double* B = LDS ? R : table + SS;
        double* out = table + (size_t)n * SS;
        for (int e = threadIdx.x; e < SS; e += blockDim.x) {
            const int i = e / S, j = e - i * S;
            double s = 0.0;
            for (int k = 0; k < S; k++) s = s + A[i * S + k] * B[k * S + j];
            out[e] = s;
        }
        __syncthreads();
        if (LDS) {
            for (int e = threadIdx.x; e < SS; e += blockDim.x) prev[e] = out[e];
            __syncthreads();
        } else {
            __threadfence_block();
        }
    }
}

// The stream of one (simulant, row, pattern): SplitMix64's output for key, from seed ^ 0x6A09E667F3BCC909, as a 64-bit state
__device__ __forceinline__ unsigned long long historyStream(unsigned long long seed, unsigned long long key) {
    return draw::mix64(seed ^ 0x6A09E667F3BCC909ull, key);
}

__device__ __forceinline__ double spacing(unsigned long long z, int q) { return -log(1.0 - ancestralUniform(z, (unsigned long long)q)); }

// One endpoint-conditioned history from state i to state j over tau (simulateConditionalOnEndingState): emit(f, from, to) for every
// real change, in time order, f the change's time as a fraction of tau.  Returns n, the number of subordinated changes (N: the
// reference's fallback to one uniformly placed event).
template <class Emit>
__device__ __forceinline__ int uniformHistory(unsigned long long z, int i, int j, double tau, double pij, double mu,
                                              const double* __restrict__ table, int S, int N, bool& bad, const Emit& emit) {
    const size_t SS = (size_t)S * S, ij = (size_t)i * S + j;
    const double u0 = ancestralUniform(z, 0);
    const double eff = mu * tau, pre = exp(-eff);
    double cdf = 0.0, scale = 1.0;
    int n = -1;
    while (u0 >= cdf) {                                   // SubordinatedProcess.drawNumberOfChanges
        n++;
        if (n == N) break;
        if (n > 0) scale = scale * eff;
        if (n > 1) scale = scale / (double)n;
        cdf = cdf + ((pre * scale) * table[(size_t)n * SS + ij]) / pij;
    }
    if (n == 0) return 0;
    if (n == 1 || n == N) {
        if (i != j) emit(ancestralUniform(z, 1), i, j);
        return n;
    }
    double total = 0.0;
    for (int q = 1; q <= n + 1; q++) total = total + spacing(z, q);
    const double* R = table + SS;
    double run = 0.0;
    int cur = i;
    for (int m = 1; m < n; m++) {
        run = run + spacing(z, m);
        const double* Rm = table + (size_t)(n - m) * SS;
        auto w = [&](int k) { return R[(size_t)cur * S + k] * Rm[(size_t)k * S + j]; };
        const int next = drawChoice(w, S, ancestralUniform(z, (unsigned long long)(n + 1 + m)), false, bad);
        if (next != cur) {
            emit(run / total, cur, next);
            cur = next;
        }
    }
    if (cur != j) {
        run = run + spacing(z, n);
        emit(run / total, cur, j);
    }
    return n;
}

// WRITE = false: values [K][r1-r0][P] into `stage`, per-workgroup row sums into `blockPartials` [block][K][nRows], real changes of
// simulant 0 into `eventCounts` [nRows][P] (may be nullptr), fallbacks into *fallbacks.  WRITE = true: simulant 0's events at
// patternOffsets[p] + eventCounts[r][p] (the counts turned into offsets within the pattern).
template <bool WRITE>
__global__ __launch_bounds__(256) void k_uniformSites(UniformSiteArgs a, int r0) {
    __shared__ double part[4][MAX_JUMP_REGISTERS];
    const int p = blockIdx.x * 256 + threadIdx.x, r = r0 + blockIdx.y;
    const bool live = p < a.P;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t SS = (size_t)a.S * a.S;
    const UniformRow row = a.rows[r];
    double sum[MAX_JUMP_REGISTERS];
#pragma unroll
    for (int k = 0; k < MAX_JUMP_REGISTERS; k++) sum[k] = 0.0;
    bool bad = false;
    int changes = 0;
    unsigned long long fallbacks = 0;
    double rateC = 0.0;
    int i = 0, j = 0;
    if (live && r > 0) {
        const int cat = a.cats[p];
        rateC = a.rates[cat];
        i = a.states[(size_t)row.parent * a.P + p];
        j = a.states[(size_t)r * a.P + p];
        if (rateC > 0.0) {
            const double tau = (row.time * row.rate) * rateC;
            const double pij = row.matrix[(size_t)cat * SS + (size_t)i * a.S + j];
            if (!(pij > 0.0) || !(pij <= DBL_MAX)) bad = true;
            const unsigned long long gp = (unsigned long long)(a.pOffset + p);
            const int sims = WRITE ? 1 : a.simulants;
            long long at = 0, end = 0;                       // this (row, pattern)'s slice of the event list (writing)
            if (WRITE) {
                at = a.patternOffsets[p] + a.eventCounts[(size_t)r * a.P + p];
                end = r + 1 < a.nRows ? a.patternOffsets[p] + a.eventCounts[(size_t)(r + 1) * a.P + p] : a.patternOffsets[p + 1];
            }
            for (int s = 0; s < sims; s++) {
                const unsigned long long key = ((unsigned long long)s * a.nRows + r) * (unsigned long long)a.globalP + gp;
                const unsigned long long z = historyStream(a.seed, key);
                double acc[MAX_JUMP_REGISTERS];
#pragma unroll
                for (int k = 0; k < MAX_JUMP_REGISTERS; k++) acc[k] = 0.0;
                double prevT = 0.0;
                int last = i;
                auto emit = [&](double f, int from, int to) {
                    if (WRITE) {
                        if (at >= end) return;
                        a.eventHeights[at] = row.hParent + f * (row.hChild - row.hParent);
                        a.eventStates[2 * at] = (uint8_t)from;
                        a.eventStates[2 * at + 1] = (uint8_t)to;
                        at++;
                        return;
                    }
                    const double t = f * tau;
#pragma unroll
                    for (int k = 0; k < MAX_JUMP_REGISTERS; k++) {
                        if (k >= a.K) break;
                        const double* reg = a.registers + (size_t)k * SS;
                        if (a.regFlags[k] & 1) acc[k] = acc[k] + reg[(size_t)from * a.S + from] * (t - prevT);
                        else acc[k] = acc[k] + reg[(size_t)from * a.S + to];
                    }
                    prevT = t;
                    last = to;
                    if (s == 0) changes++;
                };
                const int n = uniformHistory(z, i, j, tau, pij, a.mu, a.table, a.S, a.N, bad, emit);
                if (WRITE) continue;
                if (n == a.N) fallbacks++;
#pragma unroll
                for (int k = 0; k < MAX_JUMP_REGISTERS; k++) {
                    if (k >= a.K) break;
                    if (a.regFlags[k] & 1) acc[k] = acc[k] + a.registers[(size_t)k * SS + (size_t)last * a.S + last] * (tau - prevT);
                    sum[k] = sum[k] + acc[k];
                }
            }
        }
    }
    if (WRITE) return;
    if (fallbacks) atomicAdd(a.fallbacks, fallbacks);
    if (a.eventCounts && live) a.eventCounts[(size_t)r * a.P + p] = changes;
#pragma unroll
    for (int k = 0; k < MAX_JUMP_REGISTERS; k++) {
        if (k >= a.K) break;
        double v = 0.0;
        if (live && r > 0) {
            if (rateC > 0.0) {
                v = sum[k] / (double)a.simulants;
                if (a.regFlags[k] & 2) v = v / (row.rate * rateC);
            } else if ((a.regFlags[k] & 3) == 3 && i == j) {
                v = row.time;                              // MarkovJumpsBeagleTreeLikelihood.java:553-559
            }
            if (!isfinite(v)) bad = true;
        }
        if (live) a.stage[((size_t)k * a.stageRows + (r - r0)) * a.P + p] = v;
        double w = v;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) w = w + __shfl_xor(w, d, 64);
        if (lane == 0) part[wave][k] = w;
    }
    __syncthreads();
    if (threadIdx.x < a.K)
        a.blockPartials[((size_t)blockIdx.x * a.K + threadIdx.x) * a.nRows + r] =
            ((part[0][threadIdx.x] + part[1][threadIdx.x]) + part[2][threadIdx.x]) + part[3][threadIdx.x];
    if (bad) atomicOr(a.fpError, 2u);
}

// patternTotals[k][p] (+)= stage rows [r0, r1) in row order (r0 == 0: from 0; row 0 adds nothing)
__global__ __launch_bounds__(256) void k_uniformPatternTotals(const double* __restrict__ stage, int stageRows, int r0, int r1, int K,
                                                              int P, double* __restrict__ patternTotals) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= P) return;
    for (int k = 0; k < K; k++) {
        double t = r0 > 0 ? patternTotals[(size_t)k * P + p] : 0.0;
        for (int r = r0 > 0 ? r0 : 1; r < r1; r++) t = t + stage[((size_t)k * stageRows + (r - r0)) * P + p];
        patternTotals[(size_t)k * P + p] = t;
    }
}

// counts [nRows][P] -> exclusive offsets within the pattern (in place), patternCounts[p] = the pattern's events
__global__ __launch_bounds__(256) void k_eventRowOffsets(int* __restrict__ counts, int nRows, int P, long long* __restrict__ patternCounts) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= P) return;
    int run = 0;
    for (int r = 0; r < nRows; r++) {
        const int c = counts[(size_t)r * P + p];
        counts[(size_t)r * P + p] = run;
        run += c;
    }
    patternCounts[p] = run;
}

// One workgroup: v[0..P) -> exclusive prefix sums in place, v[P] = the total (integers: any order gives the same)
__global__ __launch_bounds__(1024) void k_eventPatternScan(long long* __restrict__ v, int P) {
    __shared__ long long part[1024];
    const int t = threadIdx.x;
    const int per = (P + 1023) / 1024, b = t * per, e = b + per < P ? b + per : P;
    long long s = 0;
    for (int q = b; q < e; q++) s += v[q];
    part[t] = s;
    __syncthreads();
    if (t == 0) {
        long long run = 0;
        for (int q = 0; q < 1024; q++) { const long long x = part[q]; part[q] = run; run += x; }
        v[P] = run;
    }
    __syncthreads();
    long long run = part[t];
    for (int q = b; q < e; q++) { const long long x = v[q]; v[q] = run; run += x; }
}

}  // namespace

void launchUniformPowers(hipStream_t stream, double* table, int S, int N) {
    if (N < 3) return;
    const size_t lds = 2 * (size_t)S * S * sizeof(double);
    if (lds <= 64 * 1024)
        hipLaunchKernelGGL(k_uniformPowers<true>, dim3(1), dim3(256), lds, stream, table, S, N);
    else
        hipLaunchKernelGGL(k_uniformPowers<false>, dim3(1), dim3(256), 0, stream, table, S, N);
}

void launchUniformSites(hipStream_t stream, const UniformSiteArgs& a, int r0, int r1, bool write) {
    if (r1 <= r0) return;
    const dim3 grid((unsigned)jumpSiteBlocks(a.P), (unsigned)(r1 - r0));
    if (write)
        hipLaunchKernelGGL(k_uniformSites<true>, grid, dim3(256), 0, stream, a, r0);
    else
        hipLaunchKernelGGL(k_uniformSites<false>, grid, dim3(256), 0, stream, a, r0);
}

void launchUniformPatternTotals(hipStream_t stream, const double* stage, int stageRows, int r0, int r1, int K, int P, double* patternTotals) {
    hipLaunchKernelGGL(k_uniformPatternTotals, dim3((unsigned)jumpSiteBlocks(P)), dim3(256), 0, stream, stage, stageRows, r0, r1, K, P,
                       patternTotals);
}

void launchEventOffsets(hipStream_t stream, int* counts, int nRows, int P, long long* patternOffsets) {
    hipLaunchKernelGGL(k_eventRowOffsets, dim3((unsigned)jumpSiteBlocks(P)), dim3(256), 0, stream, counts, nRows, P, patternOffsets);
    hipLaunchKernelGGL(k_eventPatternScan, dim3(1), dim3(1024), 0, stream, patternOffsets, P);
}

}  // namespace mi355
