// kernels_basta.hip — the BASTA structured-coalescent likelihood (beagleBastaUpdatePartials / beagleBastaAccumulatePartials).
//
// What it restates: the reference's GenericBastaLikelihoodDelegate.peelPartials, reduceWithinInterval and
// reduceAcrossIntervals (src/dr/evomodel/coalescent/basta/GenericBastaLikelihoodDelegate.java:813-877, 970-1006, 935-968), the
// pure-Java twin of the native library BeagleBastaLikelihoodDelegate calls.  fp64 throughout.
//
// A BASTA "partial" is one vector of S doubles (one pattern, one category); an operation pushes a lineage's vector through its
// interval's S x S matrix, and a coalescence multiplies two such results.  One operation is far too small for a launch and a
// lineage's operations form a chain (interval k + 1 reads what interval k wrote), so k_bastaUpdate<true, .> runs the WHOLE list in
// one launch: one wave per chain.  The host (engine_basta.cpp) has found, for every operation, the one operation that reads its
// result (`next`) and how many of that operation's inputs are produced inside the list (`need`).  A wave starts at an operation
// that needs nothing, and walks next, next, ... keeping its vector in LDS.  Where two chains meet (need = 2) both publish their
// last vector (agent-scope release), add one to the meeting operation's ticket, and the wave that arrives SECOND carries on with
// it (agent-scope acquire, then plain vector loads of the other chain's vector); the first simply ends.  Nobody waits for
// anybody, so nothing has to be co-resident and the grid is just the number of starting operations.  Every value is computed by
// exactly one wave from operands that do not depend on which wave that was: the same bits whatever the schedule.
// k_bastaUpdate<false, .> runs the operations [first, first + gridDim.x) of ONE interval with no chaining: the path of lists whose
// dependencies are not a forest (engine_basta.cpp says which).
//
// Sums run in index order and nothing is contracted into an FMA: the device forms every product, sum and quotient exactly as
// the host restatement does (tests/basta_reference.py).
#pragma clang fp contract(off)

#include "kernels.h"
#include "basta_stage.h"

namespace mi355 {

namespace {

constexpr int BASTA_ROWS = 4;          // rows of the result per lane: up to 256 states

// row i of M (leading dimension ld) times v, in index order
template <class MatrixPtr>
__device__ __forceinline__ double bastaRow(MatrixPtr M, int ld, int i, const double* v, int S) {
    double sum = 0.0;
    for (int j = 0; j < S; j++) sum += M[(size_t)i * ld + j] * v[j];
    return sum;
}

// M p for the rows of this lane: from the staged copy (LDS) or, above BASTA_LDS_STATES, straight from memory
template <bool STAGED>
__device__ __forceinline__ void bastaProduct(const double* g, const double* stage, int ld, const double* v, int S, double* out) {
#pragma unroll
    for (int r = 0; r < BASTA_ROWS; r++) {
        const int i = threadIdx.x + 64 * r;
        if (STAGED) out[r] = i < S ? bastaRow(stage, ld, i, v, S) : 0.0;
        else out[r] = i < S ? bastaRow(g, ld, i, v, S) : 0.0;
    }
}

template <bool CHAIN, bool STAGED>
__global__ __launch_bounds__(64) void k_bastaUpdate(const int* __restrict__ ops, const int* __restrict__ link,
                                                    const int* __restrict__ leaves, unsigned* tickets, int first,
                                                    const double* __restrict__ matrices, double* partials,
                                                    const double* __restrict__ sizes, double* coalescent, int S) {
    extern __shared__ double lds[];
    double* vIn = lds;                 // an input read from memory
    double* vOut = lds + S;            // the last result of this wave: the next operation of the chain reads it here
    double* entry = lds + 2 * S;       // a coalescence's unnormalised entries
    double* stage = lds + 3 * S;       // the matrix (staged)
    const int ld = STAGED ? (S | 1) : S;
    const int lane = threadIdx.x;
    int k = __builtin_amdgcn_readfirstlane(CHAIN ? leaves[blockIdx.x] : first + (int)blockIdx.x);
    int carried = -1;                  // the buffer whose content vOut holds
    for (;;) {
        const int* op = ops + (size_t)k * 8;
        const int dest = op[0], in1 = op[1], m1 = op[2], in2 = op[3], m2 = op[4], acc1 = op[5], acc2 = op[6], number = op[7];
        double left[BASTA_ROWS], right[BASTA_ROWS];
        // left = M1 p_in1
        const double* src = vOut;
        if (in1 != carried) { for (int j = lane; j < S; j += 64) vIn[j] = partials[(size_t)in1 * S + j]; src = vIn; }
        if (STAGED) bastaStage(matrices + (size_t)m1 * S * S, stage, S, ld);
        __syncthreads();
        bastaProduct<STAGED>(matrices + (size_t)m1 * S * S, stage, ld, src, S, left);
        __syncthreads();
        if (in2 < 0) {
#pragma unroll
            for (int r = 0; r < BASTA_ROWS; r++) { const int i = lane + 64 * r; if (i < S) { vOut[i] = left[r]; partials[(size_t)dest * S + i] = left[r]; } }
        } else {
            src = vOut;
            if (in2 != carried) { for (int j = lane; j < S; j += 64) vIn[j] = partials[(size_t)in2 * S + j]; src = vIn; }
            if (STAGED && m2 != m1) bastaStage(matrices + (size_t)m2 * S * S, stage, S, ld);
            __syncthreads();
            bastaProduct<STAGED>(matrices + (size_t)m2 * S * S, stage, ld, src, S, right);
            double e[BASTA_ROWS];
#pragma unroll
            for (int r = 0; r < BASTA_ROWS; r++) {
                const int i = lane + 64 * r;
                e[r] = i < S ? left[r] * right[r] / sizes[i] : 0.0;
                if (i < S) entry[i] = e[r];
            }
            __syncthreads();
            double prob = 0.0;
            for (int i = 0; i < S; i++) prob += entry[i];
#pragma unroll
            for (int r = 0; r < BASTA_ROWS; r++) {
                const int i = lane + 64 * r;
                if (i < S) {
                    const double d = e[r] / prob;
                    vOut[i] = d;
                    partials[(size_t)dest * S + i] = d;
                    partials[(size_t)acc1 * S + i] = left[r];
                    partials[(size_t)acc2 * S + i] = right[r];
                }
            }
            if (lane == 0) coalescent[number] = prob;
        }
        if (!CHAIN) return;
        const int nxt = link[2 * k], need = link[2 * k + 1];
        if (nxt < 0) return;
        if (need == 2) {
            // publish this chain's last vector, then draw a ticket: the second to arrive runs the coalescence
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            unsigned before = 0;
            if (lane == 0) before = __hip_atomic_fetch_add(tickets + nxt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            before = __builtin_amdgcn_readfirstlane(before);
            if (before == 0) return;
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        __syncthreads();               // (vOut is complete before the next operation reads it)
        carried = dest;
        k = nxt;
    }
}

// One wave per interval: e, f, g, h over the interval's operations in list order, then the interval's term of the log-density.
// The interval's number (where e, f, g, h and its coalescent probability live) is that of its first operation.
__global__ __launch_bounds__(64) void k_bastaReduce(const int* __restrict__ ops, const int* __restrict__ intervals,
                                                    const double* __restrict__ lengths, const double* partials,
                                                    const double* __restrict__ sizes, const double* coalescent,
                                                    double* e, double* f, double* g, double* h, double* intervalLogL, int S) {
    extern __shared__ double lds[];
    const int lane = threadIdx.x, k = blockIdx.x;
    const int begin = intervals[k], end = intervals[k + 1];
    if (begin >= end) { if (lane == 0) intervalLogL[k] = 0.0; return; }
    const int number = ops[(size_t)begin * 8 + 7];
    double se[BASTA_ROWS] = {}, sf[BASTA_ROWS] = {}, sg[BASTA_ROWS] = {}, sh[BASTA_ROWS] = {};
#pragma unroll 4
    for (int o = begin; o < end; o++) {
        const int* op = ops + (size_t)o * 8;
        const int in1 = op[1], in2 = op[3], acc1 = op[5], acc2 = op[6];
#pragma unroll
        for (int r = 0; r < BASTA_ROWS; r++) {
            const int i = lane + 64 * r;
            if (i >= S) break;
            const double a = partials[(size_t)in1 * S + i], b = partials[(size_t)acc1 * S + i];
            se[r] += a; sf[r] += a * a; sg[r] += b; sh[r] += b * b;
            if (in2 >= 0) {
                const double c = partials[(size_t)in2 * S + i], d = partials[(size_t)acc2 * S + i];
                se[r] += c; sf[r] += c * c; sg[r] += d; sh[r] += d * d;
            }
        }
    }
#pragma unroll
    for (int r = 0; r < BASTA_ROWS; r++) {
        const int i = lane + 64 * r;
        if (i >= S) break;
        const size_t at = (size_t)number * S + i;
        e[at] = se[r]; f[at] = sf[r]; g[at] = sg[r]; h[at] = sh[r];
        lds[i] = (se[r] * se[r] - sf[r] + sg[r] * sg[r] - sh[r]) / sizes[i];
    }
    __syncthreads();
    if (lane == 0) {
        double sum = 0.0;
        for (int i = 0; i < S; i++) sum += lds[i];
        double logL = -lengths[k] * sum / 4;
        const double prob = coalescent[number];
        if (prob != 0.0) logL += log(prob);
        intervalLogL[k] = logL;
    }
}

// the intervals' terms in a fixed order: lane l adds terms l, l + 64, ..., lane 0 adds the 64 partial sums
__global__ __launch_bounds__(64) void k_bastaTotal(const double* __restrict__ intervalLogL, int n, double* out) {
    __shared__ double part[64];
    double s = 0.0;
    for (int k = threadIdx.x; k < n; k += 64) s += intervalLogL[k];
    part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int l = 0; l < 64; l++) t += part[l];
        out[0] = t;
    }
}

inline size_t bastaUpdateLds(int S) { return ((size_t)3 * S + (bastaStaged(S) ? (size_t)S * (S | 1) : 0)) * sizeof(double); }

}  // namespace

void launchBastaChains(hipStream_t stream, const int* ops, const int* link, const int* leaves, int nLeaves, unsigned* tickets,
                       const double* matrices, double* partials, const double* sizes, double* coalescent, int S) {
    if (nLeaves <= 0) return;
    if (bastaStaged(S))
        hipLaunchKernelGGL((k_bastaUpdate<true, true>), dim3(nLeaves), dim3(64), bastaUpdateLds(S), stream, ops, link, leaves, tickets, 0,
                           matrices, partials, sizes, coalescent, S);
    else
        hipLaunchKernelGGL((k_bastaUpdate<true, false>), dim3(nLeaves), dim3(64), bastaUpdateLds(S), stream, ops, link, leaves, tickets, 0,
                           matrices, partials, sizes, coalescent, S);
}

void launchBastaInterval(hipStream_t stream, const int* ops, int first, int count, const double* matrices, double* partials,
                         const double* sizes, double* coalescent, int S) {
    if (count <= 0) return;
    if (bastaStaged(S))
        hipLaunchKernelGGL((k_bastaUpdate<false, true>), dim3(count), dim3(64), bastaUpdateLds(S), stream, ops, (const int*)nullptr,
                           (const int*)nullptr, (unsigned*)nullptr, first, matrices, partials, sizes, coalescent, S);
    else
        hipLaunchKernelGGL((k_bastaUpdate<false, false>), dim3(count), dim3(64), bastaUpdateLds(S), stream, ops, (const int*)nullptr,
                           (const int*)nullptr, (unsigned*)nullptr, first, matrices, partials, sizes, coalescent, S);
}

void launchBastaReduce(hipStream_t stream, const int* ops, const int* intervals, int nIntervals, const double* lengths,
                       const double* partials, const double* sizes, const double* coalescent, double* e, double* f, double* g,
                       double* h, double* intervalLogL, double* out, int S) {
    if (nIntervals > 0)
        hipLaunchKernelGGL(k_bastaReduce, dim3(nIntervals), dim3(64), (size_t)S * sizeof(double), stream, ops, intervals, lengths,
                           partials, sizes, coalescent, e, f, g, h, intervalLogL, S);
    hipLaunchKernelGGL(k_bastaTotal, dim3(1), dim3(64), 0, stream, intervalLogL, nIntervals, out);
}

}  // namespace mi355
