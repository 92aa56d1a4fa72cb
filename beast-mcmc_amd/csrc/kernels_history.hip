// kernels_history.hip — complete substitution histories simulated down the tree (beagleMi355SimulateCompleteHistories).
//
// What it restates (reference = dr.app.beagle.tools.CompleteHistorySimulator): simulate / traverse / simulateAlongBranch
// (src/dr/app/beagle/tools/CompleteHistorySimulator.java:384-496), which runs StateHistory.simulateUnconditionalOnEndingState
// (src/dr/inference/markovjumps/StateHistory.java:324-354) on every branch from the parent's realised state, takes the history's
// ending state as the child's, and keeps getTotalRegisteredCounts / getTotalReward of every registered jump process per (branch, site).
//
// Launches per chunk of sites:
//   k_historyTables     (once per call) one thread per (generator, state): the cumulative off-diagonal sums in index order — the
//                       bits of the sequential sum — their total, the largest positive index and the state's rate; two more lines
//                       for the state frequencies and the category weights;
//   k_historyWalk       lanes along sites, one wave a workgroup, every thread walks the whole pre-order row list with its site: a
//                       row's start state is what the thread stored for the parent row (program order makes it visible) or, where
//                       the parent is the row just before, what it still holds in a register.  The workgroup is on one row at a
//                       time, so the row's generator — its cumulative table, totals, last indices and rates — sits in LDS and is
//                       reloaded, behind a barrier, only where the next row names another generator.  The registers are read where
//                       a jump lands; a wave sums a count register over its sites only on rows where one of them jumped (the sum
//                       of 64 zeros is the zero it already holds).  A jump's draw is "the first i with u * total < cum_i" (up to 16 states: all entries are
//                       compared, without a branch; above: a binary search); no array is sized by S or by the number of jumps;
//   k_historyRowTotals  one thread per (register, row) adds the chunk's per-wave sums, four waves a block, blocks in ascending order,
//                       onto the running totals;
//   launchEventOffsets  (kernels_uniformized.hip) the exclusive offsets of every site's events;
//   k_historyWalk<WRITE>  the same histories again (the streams are keyed, so nothing is stored in between), their events written
//                       in (site, row, time) order — which is the order a thread meets them in.
// No float atomics.  No FMA contraction in this file; tests/complete_history_reference.py forms the same sums with numpy.
#pragma clang fp contract(off)

#include "kernels.h"
#include "ancestral_draw.h"

namespace mi355 {

namespace {

using draw::ancestralUniform;
using draw::mix64;                           // (the stream of one history)

constexpr unsigned long long HISTORY_SALT = 0x3C6EF372FE94F82Bull;

__global__ __launch_bounds__(256) void k_historyTables(const double* __restrict__ Q, int qCount, const double* __restrict__ catWeights,
                                                       const double* __restrict__ freqs, int S, int C, double* __restrict__ table,
                                                       double* __restrict__ total, double* __restrict__ rate, int* __restrict__ last) {
    const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t nGen = (size_t)qCount * S;
    if (g >= nGen + 2) return;
    const double* src;
    double* dst = table + g * S;                         // (the weights' line, the last one, follows the frequencies' S entries)
    int n = S, own = -1;
    if (g < nGen) { src = Q + g * S; own = (int)(g % (size_t)S); }
    else if (g == nGen) src = freqs;
    else { src = catWeights; n = C; }
    double cum = 0.0, top = 0.0;
    int lastPositive = 0;
    for (int i = 0; i < n; i++) {
        const double v = i == own ? 0.0 : src[i];
        cum = cum + v;
        if (v > 0.0) lastPositive = i;
        if (i == 0 || cum > top) top = cum;
        dst[i] = top;
    }
    const bool bad = !(cum > 0.0) || !(cum <= DBL_MAX);
    total[g] = cum;
    rate[g] = own >= 0 ? -src[own] : 0.0;
    last[g] = bad ? -1 : lastPositive;
}

// the first i with U < line[i] (line: non-decreasing), else `last`
template <class P>
__device__ __forceinline__ int historyPick(P line, int n, double U, int last) {
    int idx = 0;
    if (n <= 16) {
        for (int i = 0; i < n; i++) idx += (U < line[i]) ? 0 : 1;
    } else {
        int hi = n;
        while (idx < hi) {
            const int mid = (idx + hi) >> 1;
            if (U < line[mid]) hi = mid; else idx = mid + 1;
        }
    }
    return idx >= n ? last : idx;
}

template <bool WRITE>
__global__ __launch_bounds__(HISTORY_WAVE) void k_historyWalk(HistoryArgs a) {
    extern __shared__ double sh[];
    const int S = a.S, K = a.K, SS = S * S;
    double* cumL = sh;                                   // [S][S]
    double* totalL = sh + SS;                            // [S]
    double* rateL = totalL + S;                          // [S]
    int* lastL = (int*)(rateL + S);                      // [S]
    const int lane = threadIdx.x;
    const size_t s = (size_t)blockIdx.x * HISTORY_WAVE + lane;
    const bool live = s < (size_t)a.nSites;
    const unsigned long long gs = a.siteOffset + s, state0 = a.seed ^ HISTORY_SALT;
    const size_t nGen = (size_t)a.qCount * S;
    const double MI355_GLOBAL* table = gptr(a.table);
    const double MI355_GLOBAL* registers = gptr(a.registers);
    const HistoryRow* __restrict__ rows = a.rows;
    uint8_t MI355_GLOBAL* st = gptr(a.states) + s;
    unsigned flag = 0;

    // ---- the rate category and the root's state
    int cat = 0, prev = 0;
    if (live) {
        const unsigned long long z = mix64(state0, gs);
        if (a.haveCats) {
            cat = gptr(a.cats)[s];
        } else {
            if (a.C > 1) {
                const int l = gptr(a.last)[nGen + 1];
                if (l < 0) flag |= 1u;
                else cat = historyPick(table + nGen * S + S, a.C, ancestralUniform(z, 1) * gptr(a.total)[nGen + 1], l);
            }
            gptr(a.cats)[s] = cat;
        }
        if (a.haveRoot) {
            prev = st[(size_t)rows[0].slot * a.stride];
        } else {
            const int l = gptr(a.last)[nGen];
            if (l < 0) flag |= 1u;
            else prev = historyPick(table + nGen * S, S, ancestralUniform(z, 0) * gptr(a.total)[nGen], l);
            st[(size_t)rows[0].slot * a.stride] = (uint8_t)prev;
        }
    }
    const double rateC = live ? gptr(a.catRates)[cat] : 0.0;
    double siteTotal[MAX_JUMP_REGISTERS];
#pragma unroll
    for (int k = 0; k < MAX_JUMP_REGISTERS; k++) siteTotal[k] = 0.0;
    long long at = 0, end = 0;                           // this site's slice of the event list (writing)
    if (WRITE && live) {
        at = a.eventBase + gptr(a.siteOffsets)[s];
        end = a.eventBase + gptr(a.siteOffsets)[s + 1];
    }
    if (!WRITE && live) {                                // row 0 has no branch
        if (a.eventCounts) gptr(a.eventCounts)[s] = 0;
        if (a.stage)
            for (int k = 0; k < K; k++) gptr(a.stage)[(size_t)k * a.nRows * a.stride + s] = 0.0;
    }

    // ---- every other row, in list order
    int curQ = -1;
    for (int r = 1; r < a.nRows; r++) {
        const HistoryRow row = rows[r];
        if (row.q != curQ) {                             // (the same for every thread of the workgroup)
            __syncthreads();
            const size_t g0 = (size_t)row.q * S;
            for (int e = lane; e < SS; e += HISTORY_WAVE) cumL[e] = table[g0 * S + e];
            for (int e = lane; e < S; e += HISTORY_WAVE) {
                totalL[e] = gptr(a.total)[g0 + e];
                rateL[e] = gptr(a.rate)[g0 + e];
                lastL[e] = gptr(a.last)[g0 + e];
            }
            __syncthreads();
            curQ = row.q;
        }
        double v[MAX_JUMP_REGISTERS];
#pragma unroll
        for (int k = 0; k < MAX_JUMP_REGISTERS; k++) v[k] = 0.0;
        int jumps = 0;
        if (live) {
            int cur = row.parentIsPrev ? prev : (int)st[(size_t)row.parentSlot * a.stride];
            const double tau = rateC * row.length;
            const unsigned long long z = mix64(state0, (unsigned long long)r * a.siteCount + gs);
            double t = 0.0, tPrev = 0.0;
            unsigned long long n = 0;
            bool cut = false;
            while (t < tau) {
                const double rate = rateL[cur];
                if (!(rate > 0.0)) break;
                t = t + (-1.0 * log(1.0 - ancestralUniform(z, n))) / rate;
                if (t < tau) {
                    if (jumps == HISTORY_MAX_JUMPS) { flag |= 4u; cut = true; break; }
                    const int l = lastL[cur];
                    if (l < 0) { flag |= 1u; cut = true; break; }      // (a row whose off-diagonal total is not finite and > 0)
                    const int next = historyPick(cumL + cur * S, S, ancestralUniform(z, n + 1) * totalL[cur], l);
                    if (WRITE) {
                        if (at < end) {
                            gptr(a.eventHeights)[at] = row.hParent + (t / tau) * (row.hChild - row.hParent);
                            gptr(a.eventStates)[2 * at] = (uint8_t)cur;
                            gptr(a.eventStates)[2 * at + 1] = (uint8_t)next;
                            at++;
                        }
                    } else {
#pragma unroll
                        for (int k = 0; k < MAX_JUMP_REGISTERS; k++) {
                            if (k >= K) break;
                            const double MI355_GLOBAL* reg = registers + (size_t)k * SS + (size_t)cur * S;
                            if ((a.rewardMask >> k) & 1) v[k] = v[k] + reg[cur] * (t - tPrev);
                            else v[k] = v[k] + reg[next];
                        }
                    }
                    tPrev = t;
                    cur = next;
                    jumps++;
                }
                n += 2;
            }
            if (!WRITE && !cut && a.rewardMask) {
#pragma unroll
                for (int k = 0; k < MAX_JUMP_REGISTERS; k++) {
                    if (k >= K) break;
                    if ((a.rewardMask >> k) & 1) v[k] = v[k] + registers[(size_t)k * SS + (size_t)cur * S + cur] * (tau - tPrev);
                }
            }
            st[(size_t)row.slot * a.stride] = (uint8_t)cur;
            prev = cur;
        }
        if (WRITE) continue;
        if (live && a.eventCounts) gptr(a.eventCounts)[(size_t)r * a.nSites + s] = jumps;
        // a wave in which no lane jumped on this row holds +0.0 in every lane of a count register: its sum is lane 0's value
        const bool anyJump = a.wavePartials && __any(jumps > 0);
#pragma unroll
        for (int k = 0; k < MAX_JUMP_REGISTERS; k++) {
            if (k >= K) break;
            siteTotal[k] = siteTotal[k] + v[k];
            if (live && a.stage) gptr(a.stage)[((size_t)k * a.nRows + r) * a.stride + s] = v[k];
            if (a.wavePartials) {
                double w = v[k];
                if (anyJump || ((a.rewardMask >> k) & 1)) {
#pragma unroll
                    for (int d = 32; d >= 1; d >>= 1) w = w + __shfl_xor(w, d, 64);
                }
                if (lane == 0) gptr(a.wavePartials)[((size_t)blockIdx.x * K + k) * a.nRows + r] = w;
            }
        }
    }
    if (!WRITE && live) {
#pragma unroll
        for (int k = 0; k < MAX_JUMP_REGISTERS; k++) {
            if (k >= K) break;
            gptr(a.siteTotals)[(size_t)k * a.stride + s] = siteTotal[k];
        }
    }
    if (flag && !WRITE) atomicOr(a.fpError, flag);
}

__global__ __launch_bounds__(256) void k_historyRowTotals(const double* __restrict__ wavePartials, int waves, int K, int nRows, int first,
                                                          double* __restrict__ rowTotals) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= K * nRows) return;
    const int k = t / nRows, r = t - k * nRows;
    double sum = first ? 0.0 : rowTotals[t];
    if (r > 0) {
        for (int w0 = 0; w0 < waves; w0 += 4) {
            double p[4];
#pragma unroll
            for (int q = 0; q < 4; q++) p[q] = w0 + q < waves ? wavePartials[((size_t)(w0 + q) * K + k) * nRows + r] : 0.0;
            sum = sum + (((p[0] + p[1]) + p[2]) + p[3]);
        }
    } else {
        sum = 0.0;
    }
    rowTotals[t] = sum;
}

}  // namespace

void launchHistoryTables(hipStream_t stream, const double* Q, int qCount, const double* catWeights, const double* freqs, int S, int C,
                         double* table, double* total, double* rate, int* last) {
    const size_t lines = historyLines(qCount, S);
    hipLaunchKernelGGL(k_historyTables, dim3((unsigned)((lines + 255) / 256)), dim3(256), 0, stream, Q, qCount, catWeights, freqs, S, C,
                       table, total, rate, last);
}

void launchHistoryWalk(hipStream_t stream, const HistoryArgs& a, bool write) {
    if (a.nSites < 1) return;
    const dim3 grid((unsigned)(((size_t)a.nSites + HISTORY_WAVE - 1) / HISTORY_WAVE)), block(HISTORY_WAVE);
    const size_t lds = ((size_t)a.S * a.S + 2 * (size_t)a.S) * sizeof(double) + (size_t)a.S * sizeof(int);
    if (write)
        hipLaunchKernelGGL(k_historyWalk<true>, grid, block, lds, stream, a);
    else
        hipLaunchKernelGGL(k_historyWalk<false>, grid, block, lds, stream, a);
}

void launchHistoryRowTotals(hipStream_t stream, const double* wavePartials, int waves, int K, int nRows, bool first, double* rowTotals) {
    const int n = K * nRows;
    hipLaunchKernelGGL(k_historyRowTotals, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, wavePartials, waves, K, nRows,
                       first ? 1 : 0, rowTotals);
}

}  // namespace mi355
