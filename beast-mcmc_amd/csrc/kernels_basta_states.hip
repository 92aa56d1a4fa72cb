// kernels_basta_states.hip — BASTA lineage demes: a state for every vector of an operation list, drawn from the roots outwards
// (beagleBastaSampleStates; the rule is stated in include/beagle_mi355.h).
//
// What it restates: BastaLikelihood.traverseSampleByCoalescentIntervals (src/dr/evomodel/coalescent/basta/BastaLikelihood.java:
// 755-943): the root from p f (:889-909), then every branch-interval operation from the last interval to the first, each input from
// the row of the operation's matrix its `dest` state selects times the input's vector (:911-943), fixed tips without a draw (:846-867).
//
// A vector's state needs its reader's state and nothing else, so the work fans out from the roots and never meets.  The host
// (engine_basta.cpp planStates) cuts it into CHAINS — one input of a coalescence, then the one-input operations that produced it, down
// to a vector the list does not produce or to the `dest` of the next coalescence — and sorts them by the number of coalescences above
// them, each chain's draws laid out in order (kernels.h BastaStatesArgs: no pointer is chased on the device).  One launch runs the
// chains of ONE such level: a wave per (chain, 64 replicates), lane = replicate.  The wave walks its chain top to bottom; per step the
// matrix and the input's vector are in LDS (odd leading dimension) and each lane gathers the row its own state selects.  The state at
// the top of a chain was stored by the level before (a root's is drawn here, by both chains of a root coalescence alike), so nothing
// waits for another workgroup.
//
// A chain is a sequence of dependent small draws, so a step costs what its memory latencies cost:
//   k_bastaStatesAhead<REGS>   up to 32 states: the NEXT step's matrix and vector are asked for (into registers, REGS matrix entries a
//                              lane) before the current step is drawn and go into the other of two LDS buffers after it: no step waits
//                              for memory it could have asked for earlier
//   k_bastaStates<true>        33..64 states (two such buffers and the changes histogram do not fit 64 KB of LDS): one buffer, staged
//                              per step as k_bastaUpdate stages it
//   k_bastaStates<false>       above 64 states: the matrix is read from memory
//
// Counts are integers: a step's occupancy goes through a per-wave LDS histogram into 64-bit counters, a chain's changes through an
// [S][S] LDS histogram (up to 64 states; above that straight to the counters) flushed when the chain ends.
//
// Nothing is contracted into an FMA: weights, totals and the walk of the draw are the host restatement's bit for bit
// (tests/basta_states_reference.py).
#pragma clang fp contract(off)

#include "kernels.h"
#include "basta_stage.h"
#include "ancestral_draw.h"

namespace mi355 {

namespace {

constexpr int BASTA_AHEAD_STATES = 32;   // up to here k_bastaStatesAhead

// what a wave knows of its chain and its lanes of their replicates
struct ChainWalk {
    int nSteps, l; bool live, map, bad; unsigned long long stream; int s; const int4* steps;
};

// the chain of this workgroup; the state at its top: drawn from p f (a root) or what the level above stored
__device__ __forceinline__ ChainWalk bastaChainStart(const BastaStatesArgs& a, int first) {
    const int S = a.S;
    const int4 chain = a.chains[first + (int)blockIdx.x];
    const int dest = __builtin_amdgcn_readfirstlane(chain.z);
    ChainWalk c;
    c.nSteps = __builtin_amdgcn_readfirstlane(chain.y);
    c.steps = a.steps + __builtin_amdgcn_readfirstlane(chain.x);
    c.l = (int)blockIdx.y * 64 + (int)threadIdx.x;                           // column of the chunk
    c.live = c.l < a.count;
    c.stream = draw::mix64(a.seed, (unsigned long long)a.r0 + (unsigned long long)c.l);
    c.map = a.map != 0; c.bad = false; c.s = 0;
    if (chain.w & BASTA_CHAIN_ROOT) {
        const double* p = a.partials + (size_t)dest * S;
        const double* f = a.freqs;
        c.s = draw::drawChoice([&](int i) { return p[i] * f[i]; }, S, draw::ancestralUniform(c.stream, (unsigned long long)dest), c.map, c.bad);
        if (c.live && (chain.w & BASTA_CHAIN_STORES_ROOT)) a.states[(size_t)dest * a.stride + c.l] = (uint8_t)c.s;
    } else if (c.live) {
        c.s = a.states[(size_t)dest * a.stride + c.l];
        if (c.s >= S) c.s = 0;                                               // (never: the level above stored it; keeps the gather inside the matrix)
    }
    return c;
}

// state t drawn for the input of `step` under dest state c.s: stored, counted; then it is the state the next step starts from
template <bool LDS_CHANGES>
__device__ __forceinline__ void bastaStepDone(const BastaStatesArgs& a, ChainWalk& c, const int4& step, int t, unsigned* occ, unsigned* chg) {
    const int S = a.S, lane = threadIdx.x;
    if (c.live) {
        a.states[(size_t)step.x * a.stride + c.l] = (uint8_t)t;
        if (step.z >= 0) a.states[(size_t)step.z * a.stride + c.l] = (uint8_t)t;
    }
    if (a.occupancy) {
        if (c.live) atomicAdd(&occ[t], 1u);
        __syncthreads();
        unsigned long long* out = a.occupancy + (size_t)step.w * S;
        for (int j = lane; j < S; j += 64) {
            const unsigned n = occ[j];
            if (n) { __hip_atomic_fetch_add(out + j, (unsigned long long)n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); occ[j] = 0u; }
        }
        __syncthreads();
    }
    if (a.changes && c.live) {
        if (LDS_CHANGES) atomicAdd(&chg[c.s * S + t], 1u);
        else __hip_atomic_fetch_add(a.changes + (size_t)c.s * S + t, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    c.s = t;
}

template <bool LDS_CHANGES>
__device__ __forceinline__ void bastaChainEnd(const BastaStatesArgs& a, const ChainWalk& c, const unsigned* chg) {
    const int S = a.S;
    if (LDS_CHANGES && a.changes) {
        __syncthreads();
        for (int i = threadIdx.x; i < S * S; i += 64) {
            const unsigned n = chg[i];
            if (n) __hip_atomic_fetch_add(a.changes + i, (unsigned long long)n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    if (c.live && c.bad) atomicOr(a.error, 1u);
}

// is v (S entries at a wave-uniform address, LDS or memory) a vector with exactly one positive entry, and which
__device__ __forceinline__ bool bastaFixed(const double* v, int S, int* at) {
    int positives = 0, last = 0;
    for (int base = 0; base < S; base += 64) {
        const int j = base + (int)threadIdx.x;
        const unsigned long long mask = __ballot(j < S && v[j < S ? j : 0] > 0.0);
        positives += __popcll(mask);
        if (mask) last = base + 63 - __clzll(mask);
    }
    *at = last;
    return positives == 1;
}

template <bool STAGED>
__global__ __launch_bounds__(64) void k_bastaStates(BastaStatesArgs a, int first) {
    extern __shared__ double lds[];
    const int S = a.S, lane = threadIdx.x;
    const int ld = STAGED ? (S | 1) : S;
    double* stage = lds;                                                     // STAGED: the operation's matrix
    unsigned* occ = reinterpret_cast<unsigned*>(lds + (STAGED ? S * ld : 0));   // [S]: the step's inputs by state
    unsigned* chg = occ + S;                                                 // STAGED: [S][S], the chain's (dest state, input state) pairs
    for (int i = lane; i < S + (STAGED && a.changes ? S * S : 0); i += 64) occ[i] = 0u;
    __syncthreads();
    ChainWalk c = bastaChainStart(a, first);
    int4 cur = c.steps[0];
    for (int i = 0; i < c.nSteps; i++) {
        const int4 next = c.steps[i + 1 < c.nSteps ? i + 1 : i];             // asked for now, used after this step's draw
        const double* p = a.partials + (size_t)cur.x * S;
        int t;
        if (!bastaFixed(p, S, &t)) {
            const double* M = a.matrices + (size_t)cur.y * S * S;
            const double u = draw::ancestralUniform(c.stream, (unsigned long long)cur.x);
            if (STAGED) {
                __syncthreads();                                             // (the lanes are done with the matrix before)
                bastaStage(M, stage, S, ld);
                __syncthreads();
                const double* row = a.asWritten ? stage + c.s : stage + c.s * ld;
                const int step = a.asWritten ? ld : 1;
                t = draw::drawChoice([&](int j) { return row[j * step] * p[j]; }, S, u, c.map, c.bad);
            } else {
                const double* row = a.asWritten ? M + c.s : M + (size_t)c.s * S;
                const int step = a.asWritten ? S : 1;
                t = draw::drawChoice([&](int j) { return row[(size_t)j * step] * p[j]; }, S, u, c.map, c.bad);
            }
        }
        bastaStepDone<STAGED>(a, c, cur, t, occ, chg);
        cur = next;
    }
    bastaChainEnd<STAGED>(a, c, chg);
}

// a step's matrix (REGS entries a lane) and vector from memory into registers ...
template <int REGS>
__device__ __forceinline__ void bastaAheadLoad(const BastaStatesArgs& a, const int4& step, double (&m)[REGS], double& v) {
    const int S = a.S, n = S * S, lane = threadIdx.x;
    const double* M = a.matrices + (size_t)step.y * n;
#pragma unroll
    for (int u = 0; u < REGS; u++) { const int at = lane + 64 * u; m[u] = at < n ? M[at] : 0.0; }
    v = lane < S ? a.partials[(size_t)step.x * S + lane] : 0.0;
}
// ... and from there into an LDS buffer [S][ld] | [S] (the row of entry `at`: basta_stage.h)
template <int REGS>
__device__ __forceinline__ void bastaAheadStore(double* buf, int S, int ld, const double (&m)[REGS], double v) {
    const int n = S * S, pad = ld - S, lane = threadIdx.x;
    const unsigned magic = (1u << 18) / (unsigned)S + 1u;
#pragma unroll
    for (int u = 0; u < REGS; u++) {
        const int at = lane + 64 * u;
        if (at < n) buf[at + (int)(((unsigned)at * magic) >> 18) * pad] = m[u];
    }
    if (lane < S) buf[S * ld + lane] = v;
}

template <int REGS>
__global__ __launch_bounds__(64) void k_bastaStatesAhead(BastaStatesArgs a, int first) {
    extern __shared__ double lds[];
    const int S = a.S, lane = threadIdx.x, ld = S | 1, bufDoubles = S * ld + S;
    unsigned* occ = reinterpret_cast<unsigned*>(lds + 2 * bufDoubles);
    unsigned* chg = occ + S;
    for (int i = lane; i < S + (a.changes ? S * S : 0); i += 64) occ[i] = 0u;
    ChainWalk c = bastaChainStart(a, first);
    double m[REGS], v;
    int4 cur = c.steps[0];
    int4 next = c.steps[c.nSteps > 1 ? 1 : 0];
    bastaAheadLoad<REGS>(a, cur, m, v);
    bastaAheadStore<REGS>(lds, S, ld, m, v);
    __syncthreads();
    for (int i = 0; i < c.nSteps; i++) {
        const double* buf = lds + (i & 1) * bufDoubles;
        const double* p = buf + S * ld;
        const bool more = i + 1 < c.nSteps;
        const int4 after = c.steps[i + 2 < c.nSteps ? i + 2 : i];            // the step after the next: its record, asked for now
        if (more) bastaAheadLoad<REGS>(a, next, m, v);                       // the next step's data: asked for now, stored after the draw
        int t;
        if (!bastaFixed(p, S, &t)) {
            const double* row = a.asWritten ? buf + c.s : buf + c.s * ld;
            const int step = a.asWritten ? ld : 1;
            t = draw::drawChoice([&](int j) { return row[j * step] * p[j]; }, S, draw::ancestralUniform(c.stream, (unsigned long long)cur.x),
                                 c.map, c.bad);
        }
        bastaStepDone<true>(a, c, cur, t, occ, chg);
        if (more) bastaAheadStore<REGS>(lds + ((i + 1) & 1) * bufDoubles, S, ld, m, v);
        __syncthreads();                                                     // (the other buffer is complete; this one is free)
        cur = next; next = after;
    }
    bastaChainEnd<true>(a, c, chg);
}

// out[l][v] = states[v][l]: 64 x 64 tiles through LDS, both sides coalesced
__global__ __launch_bounds__(256) void k_bastaStatesTranspose(const uint8_t* __restrict__ states, int vectors, int stride, int count,
                                                              uint8_t* __restrict__ out) {
    __shared__ uint8_t tile[64][65];
    const int v0 = (int)blockIdx.x * 64, l0 = (int)blockIdx.y * 64;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    for (int i = ty; i < 64; i += 4) {
        const int v = v0 + i, l = l0 + tx;
        if (v < vectors && l < count) tile[i][tx] = states[(size_t)v * stride + l];
    }
    __syncthreads();
    for (int i = ty; i < 64; i += 4) {
        const int l = l0 + i, v = v0 + tx;
        if (l < count && v < vectors) out[(size_t)l * vectors + v] = tile[tx][i];
    }
}

inline size_t bastaStatesLds(int S) {
    const size_t counts = ((size_t)S + (size_t)S * S) * sizeof(unsigned);
    if (S <= BASTA_AHEAD_STATES) return 2 * ((size_t)S * (S | 1) + S) * sizeof(double) + counts;
    return bastaStaged(S) ? (size_t)S * (S | 1) * sizeof(double) + counts : (size_t)S * sizeof(unsigned);
}

}  // namespace

void launchBastaStates(hipStream_t stream, const BastaStatesArgs& a, int first, int n) {
    if (n <= 0 || a.count <= 0) return;
    const dim3 grid(n, (a.count + 63) / 64);
    const size_t lds = bastaStatesLds(a.S);
    const int entries = (a.S * a.S + 63) / 64;               // matrix entries a lane
    if (a.S > BASTA_AHEAD_STATES) {
        if (bastaStaged(a.S)) hipLaunchKernelGGL(k_bastaStates<true>, grid, dim3(64), lds, stream, a, first);
        else hipLaunchKernelGGL(k_bastaStates<false>, grid, dim3(64), lds, stream, a, first);
    }
    else if (entries <= 1) hipLaunchKernelGGL(k_bastaStatesAhead<1>, grid, dim3(64), lds, stream, a, first);
    else if (entries <= 4) hipLaunchKernelGGL(k_bastaStatesAhead<4>, grid, dim3(64), lds, stream, a, first);
    else hipLaunchKernelGGL(k_bastaStatesAhead<16>, grid, dim3(64), lds, stream, a, first);
}

void launchBastaStatesTranspose(hipStream_t stream, const uint8_t* states, int vectors, int stride, int count, uint8_t* out) {
    if (vectors <= 0 || count <= 0) return;
    hipLaunchKernelGGL(k_bastaStatesTranspose, dim3((vectors + 63) / 64, (count + 63) / 64), dim3(256), 0, stream, states, vectors,
                       stride, count, out);
}

}  // namespace mi355
