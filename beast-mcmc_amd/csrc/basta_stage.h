// basta_stage.h — an operation's S x S matrix staged in LDS by one wave, shared by the BASTA kernels (kernels_basta.hip,
// kernels_basta_states.hip).  Device code only.
#pragma once

namespace mi355 {
namespace {

constexpr int BASTA_LDS_STATES = 64;   // up to here an operation's matrix is staged in LDS (33 KB at 64 states)

// S <= BASTA_LDS_STATES: the operation's matrix is staged in LDS with coalesced reads (odd leading dimension: a lane reads its own
// row): all 64 lanes over the S * S entries, sixteen loads in flight per lane before the first is waited for (a loop that stores
// each value as it arrives is a chain of 58 L2 latencies at 61 states: 19 us an operation).  The row of entry `at` is
// at / S by a multiply and a shift: exact for at < 4096 and S <= 64 (magic = 2^18 / S + 1 overshoots at / S by less than 1 / 64).
__device__ __forceinline__ void bastaStage(const double* g, double* stage, int S, int ld) {
    const int n = S * S, pad = ld - S;
    const unsigned magic = (1u << 18) / (unsigned)S + 1u;
    if (n <= 64) {                                        // (up to 8 states: one load)
        const int at = threadIdx.x;
        if (at < n) stage[at + (int)(((unsigned)at * magic) >> 18) * pad] = g[at];
        return;
    }
    for (int base = threadIdx.x; base < n; base += 64 * 16) {
        double r[16];
#pragma unroll
        for (int u = 0; u < 16; u++) { const int at = base + 64 * u; r[u] = at < n ? g[at] : 0.0; }
#pragma unroll
        for (int u = 0; u < 16; u++) {
            const int at = base + 64 * u;
            if (at < n) stage[at + (int)(((unsigned)at * magic) >> 18) * pad] = r[u];
        }
    }
}

inline bool bastaStaged(int S) { return S <= BASTA_LDS_STATES; }

}  // namespace
}  // namespace mi355
