// kernels_tipemission.hip — tip error models (beagleMi355SetTipEmission, engine_tipemission.cpp).  A tip whose partials are a lookup
// E[code][state] is a compact tip whose branch matrix is M E^T: k_foldTipEmission writes those products into the shadow matrix slots
// in front of an operation list; k_expandTipEmission writes the lookup out as a partials buffer for the callers that need one.
#include "kernels.h"

namespace mi355 {

// shadow[c][i][k] = sum_j M[c][i][j] E[k][j], the products added with j ascending and never fused (what a host statement of the
// same sum gives, bit for bit); columns k >= K are zero.  One workgroup per (job, category).
__global__ void __launch_bounds__(256) k_foldTipEmission(double* __restrict__ matrices, const TipFoldJob* __restrict__ jobs, int S, int C) {
#pragma clang fp contract(off)
    const TipFoldJob job = jobs[blockIdx.x];
    const int c = blockIdx.y;
    const size_t per = (size_t)C * S * S;
    const double* __restrict__ M = matrices + per * (size_t)job.src + (size_t)c * S * S;
    double* __restrict__ out = matrices + per * (size_t)job.dst + (size_t)c * S * S;
    const double* __restrict__ E = job.emission;
    for (int e = threadIdx.x; e < S * S; e += 256) {
        const int i = e / S, k = e - i * S;
        double sum = 0.0;
        if (k < job.K) {
            const double* row = M + (size_t)i * S;
            const double* col = E + (size_t)k * S;
            for (int j = 0; j < S; j++) { const double t = row[j] * col[j]; sum = sum + t; }
        }
        out[e] = sum;
    }
}

void launchFoldTipEmission(hipStream_t stream, double* matrices, const TipFoldJob* dJobs, int nJobs, int S, int C) {
    if (nJobs <= 0) return;
    hipLaunchKernelGGL(k_foldTipEmission, dim3((unsigned)nJobs, (unsigned)C), dim3(256), 0, stream, matrices, dJobs, S, C);
}

// partials[c][p][i] = E[code_p][i], all ones for a code >= K; T32 layout: the padded patterns of the last tile are zero
template <bool TILED>
__global__ void __launch_bounds__(256) k_expandTipEmission(double* __restrict__ dest, const uint8_t* __restrict__ codes,
                                                            const double* __restrict__ E, int K, int P, int S, int C) {
    const int p = blockIdx.x * 256 + threadIdx.x, ntile = (P + 31) >> 5;
    const int slots = TILED ? ntile * 32 : P;
    if (p >= slots) return;
    const bool pad = p >= P;
    const int code = pad ? 255 : codes[p];
    const bool known = code < K;
    for (int i = 0; i < S; i++) {
        const double v = pad ? 0.0 : known ? E[(size_t)code * S + i] : 1.0;
        for (int c = 0; c < C; c++) {
            const size_t at = TILED ? (((size_t)c * ntile + (p >> 5)) * S + i) * 32 + (p & 31) : ((size_t)c * P + p) * S + i;
            dest[at] = v;
        }
    }
}

void launchExpandTipEmission(hipStream_t stream, double* dest, const uint8_t* codes, const double* emission, int K, int P, int S, int C,
                             bool tiled) {
    const int slots = tiled ? ((P + 31) / 32) * 32 : P;
    dim3 grid((slots + 255) / 256), block(256);
    if (tiled) hipLaunchKernelGGL(k_expandTipEmission<true>, grid, block, 0, stream, dest, codes, emission, K, P, S, C);
    else hipLaunchKernelGGL(k_expandTipEmission<false>, grid, block, 0, stream, dest, codes, emission, K, P, S, C);
}

}  // namespace mi355
