// kernels_simulate.hip — an alignment drawn from the model, down the tree (beagleMi355SimulateSequences).
//
// What it restates (reference = dr.app.beagle.tools.Partition): traverse (src/dr/app/beagle/tools/Partition.java:292-387), which reads
// a branch matrix back per branch and then draws every site in Java with randomChoicePDF (:519-536): cumulative sums in index
// order, the first index whose sum is above u.
//
// Two launches.  k_simTables forms the cumulative sums ONCE per (row, category, parent state) — they do not depend on u — with one
// thread per matrix row adding its S terms in index order: the bits of the sequential sum.  k_simSites then gives every thread
// SIM_SITES_PER_THREAD consecutive sites and walks the row list with them: sites are independent and a row depends only on its
// parent's row, so a thread reads back what it stored itself (program order makes it visible) — or, where the parent is the row just
// before (a first child in pre-order: half the rows), keeps it in a register.  The walk is a chain of dependent loads per row
// (parent state -> table row), bound by their latency; four sites a thread are four such chains in flight, and a row's four states
// leave as one 32-bit store.  A draw compares u with the S table entries (up to 16 states: all of them, without a branch; above: a
// binary search) and touches nothing else; no array is sized by S, nothing spills.
//
// No FMA contraction in this file; tests/simulate_reference.py forms the same sums with numpy.
#pragma clang fp contract(off)

#include "kernels.h"
#include "ancestral_draw.h"

namespace mi355 {

namespace {

using draw::ancestralUniform;

constexpr int SIM_BLOCK = 64;                // one wave a workgroup: the walk is latency-bound, so the sites go to as many CUs as there are

__global__ __launch_bounds__(256) void k_simTables(const SimRow* __restrict__ rows, int nRows, const double* __restrict__ catWeights,
                                                   const double* __restrict__ freqs, int S, int C, double* __restrict__ table,
                                                   int* __restrict__ meta) {
    const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t perRow = (size_t)C * S, nMat = (size_t)(nRows - 1) * perRow;
    if (g >= nMat + 2) return;
    const double MI355_GLOBAL* src;
    double MI355_GLOBAL* dst = gptr(table) + g * S;      // (the weights' row, the last one, follows the frequencies' S entries)
    int n = S;
    if (g < nMat) src = gptr(rows[1 + g / perRow].matrix) + (g % perRow) * S;
    else if (g == nMat) src = gptr(freqs);
    else { src = gptr(catWeights); n = C; }
    double cum = 0.0, top = 0.0;
    int lastPositive = 0;
    for (int i = 0; i < n; i++) {
        const double v = src[i];
        cum = cum + v;
        if (v > 0.0) lastPositive = i;
        if (i == 0 || cum > top) top = cum;
        dst[i] = top;
    }
    const bool bad = !(cum > 0.0) || !(cum <= DBL_MAX);
    if (bad)
        for (int i = 0; i < n; i++) dst[i] = __builtin_nan("");
    gptr(meta)[g] = bad ? -1 : lastPositive;
}

// the first i with u < row[i] (row: non-decreasing, or all NaN), else what meta says.  SS > 0: n = SS
template <int SS>
__device__ __forceinline__ int simPick(const double MI355_GLOBAL* row, const int MI355_GLOBAL* meta, int n, double u, bool& bad) {
    int idx = 0;
    if (SS) {
#pragma unroll
        for (int i = 0; i < SS; i++) idx += (u < row[i]) ? 0 : 1;
        n = SS;
    } else if (n <= 16) {
        for (int i = 0; i < n; i++) idx += (u < row[i]) ? 0 : 1;
    } else {
        int hi = n;
        while (idx < hi) {
            const int mid = (idx + hi) >> 1;
            if (u < row[mid]) hi = mid; else idx = mid + 1;
        }
    }
    if (idx >= n) {
        const int m = *meta;
        bad = bad || m < 0;
        idx = m < 0 ? 0 : m;
    }
    return idx;
}

template <int SS>
__global__ __launch_bounds__(SIM_BLOCK) void k_simSites(const SimRow* __restrict__ rows, int nRows, const double* __restrict__ table,
                                                        const int* __restrict__ meta, int Sdyn, int C, int nSites, size_t stride,
                                                        unsigned long long siteCount, unsigned long long siteOffset,
                                                        unsigned long long seed, int haveRoot, int haveCats, uint8_t* states,
                                                        int* cats, unsigned* fpError) {
    constexpr int K = SIM_SITES_PER_THREAD;
    const int S = SS ? SS : Sdyn;
    const size_t s0 = ((size_t)blockIdx.x * SIM_BLOCK + threadIdx.x) * K;
    if (s0 >= (size_t)nSites) return;
    // the sites past the chunk's end (k >= liveSites: only in its last thread) are walked like the others — their bytes are padding
    // of the scratch rows and go nowhere — but take no input and report no error
    const int liveSites = (size_t)nSites - s0 < (size_t)K ? (int)((size_t)nSites - s0) : K;
    const unsigned long long g0 = siteOffset + s0;
    const size_t perRow = (size_t)C * S, nMat = (size_t)(nRows - 1) * perRow;
    const double MI355_GLOBAL* tab = gptr(table);
    const int MI355_GLOBAL* met = gptr(meta);
    uint8_t MI355_GLOBAL* st = gptr(states) + s0;
    bool bad[K];
    int cat[K];
#pragma unroll
    for (int k = 0; k < K; k++) { bad[k] = false; cat[k] = 0; }

    // ---- rate categories
    if (haveCats) {
#pragma unroll
        for (int k = 0; k < K; k++)
            if (k < liveSites) cat[k] = gptr(cats)[s0 + k];
    } else {
        if (C > 1) {
#pragma unroll
            for (int k = 0; k < K; k++)
                cat[k] = simPick<0>(tab + nMat * S + S, met + nMat + 1, C, ancestralUniform(seed, (g0 + k) * 2 + 1), bad[k]);
        }
#pragma unroll
        for (int k = 0; k < K; k++) gptr(cats)[s0 + k] = cat[k];
    }

    // ---- the root
    const SimRow root = rows[0];
    unsigned prev = 0;
    if (haveRoot) {
        const unsigned given = *(const unsigned MI355_GLOBAL*)(st + (size_t)root.slot * stride);
#pragma unroll
        for (int k = 0; k < K; k++)
            if (k < liveSites) prev |= given & (0xFFu << (8 * k));
    } else {
#pragma unroll
        for (int k = 0; k < K; k++)
            prev |= (unsigned)simPick<SS>(tab + nMat * S, met + nMat, S, ancestralUniform(seed, (g0 + k) * 2), bad[k]) << (8 * k);
    }
    *(unsigned MI355_GLOBAL*)(st + (size_t)root.slot * stride) = prev;

    // ---- every other row, in list order
    SimRow ahead = rows[nRows > 1 ? 1 : 0];                  // (the next row's descriptor is asked for a row early)
    for (int r = 1; r < nRows; r++) {
        const SimRow row = ahead;
        if (r + 1 < nRows) ahead = rows[r + 1];
        const unsigned parent = row.parentIsPrev ? prev : *(const unsigned MI355_GLOBAL*)(st + (size_t)row.parentSlot * stride);
        const size_t base = (size_t)(r - 1) * perRow;
        const unsigned long long ctr0 = (unsigned long long)r * siteCount + g0;
        unsigned packed = 0;
#pragma unroll
        for (int k = 0; k < K; k++) {
            const size_t line = base + (size_t)cat[k] * S + ((parent >> (8 * k)) & 0xFFu);
            packed |= (unsigned)simPick<SS>(tab + line * S, met + line, S, ancestralUniform(seed, (ctr0 + k) * 2), bad[k]) << (8 * k);
        }
        *(unsigned MI355_GLOBAL*)(st + (size_t)row.slot * stride) = packed;
        prev = packed;
    }
    bool anyBad = false;
#pragma unroll
    for (int k = 0; k < K; k++) anyBad = anyBad || (bad[k] && k < liveSites);
    if (anyBad) atomicOr(fpError, 1u);
}

}  // namespace

void launchSimTables(hipStream_t stream, const SimRow* dRows, int nRows, const double* catWeights, const double* freqs, int S, int C,
                     double* table, int* meta) {
    const size_t lines = simTableRows(nRows, S, C);
    hipLaunchKernelGGL(k_simTables, dim3((unsigned)((lines + 255) / 256)), dim3(256), 0, stream, dRows, nRows, catWeights, freqs, S, C,
                       table, meta);
}

void launchSimSites(hipStream_t stream, const SimRow* dRows, int nRows, const double* table, const int* meta, int S, int C,
                    int nSites, size_t stride, unsigned long long siteCount, unsigned long long siteOffset, unsigned long long seed,
                    bool haveRoot, bool haveCats, uint8_t* states, int* cats, unsigned* fpError) {
    const size_t threads = ((size_t)nSites + SIM_SITES_PER_THREAD - 1) / SIM_SITES_PER_THREAD;
    const dim3 grid((unsigned)((threads + SIM_BLOCK - 1) / SIM_BLOCK)), block(SIM_BLOCK);
    if (S == 4)
        hipLaunchKernelGGL(k_simSites<4>, grid, block, 0, stream, dRows, nRows, table, meta, S, C, nSites, stride, siteCount, siteOffset,
                           seed, haveRoot ? 1 : 0, haveCats ? 1 : 0, states, cats, fpError);
    else
        hipLaunchKernelGGL(k_simSites<0>, grid, block, 0, stream, dRows, nRows, table, meta, S, C, nSites, stride, siteCount, siteOffset,
                           seed, haveRoot ? 1 : 0, haveCats ? 1 : 0, states, cats, fpError);
}

}  // namespace mi355
