// kernels_epoch.hip — branch matrices of epoch models (beagleMi355UpdateTransitionMatricesWithEpochs, engine_epoch.cpp): a branch that
// crosses epoch boundaries gets the product of its segments' transition matrices, root end first, without a matrix slot per segment and
// without a launch per product.  For entry e with segments j = 0 .. n - 1 and category c
//     M_j = U_j exp(Lambda_j length_j rate_c) U_j^-1, negative entries clamped to 0 — transition_body.h, the arithmetic and summation
//           order of k_transition / k_transition4 (this file is compiled with the same contraction as kernels.hip: no pragma here),
//     slot = ((M_0 M_1) M_2) ... M_(n-1),   each product sum_k a_ik b_kj with k upwards from 0.0 and NOT clamped (as k_convolve).
//   k_epochSmall<S>     S <= 8: one thread per (entry, category); the running product and the current segment matrix in registers, the
//                       eigen systems read through L2.  A product is one fused multiply-add per k, k = 0 .. S - 1; a row of the product
//                       is formed before it replaces the row it was formed from.
//   k_epochBlock<MFMA>  9 <= S <= 64: one workgroup per (entry, category).  Three LDS images [N][LD], N = S rounded up to a multiple of 4,
//                       LD = N + 4 (kernels_generator.hip's padding; the padding is zero and stays zero): the running product, the next
//                       one, the segment.  The segment's U^-1 exp staging (S x S + S doubles) lives in the free product image.  From 16
//                       states the product runs on v_mfma_f64_4x4x4_4b_f64: k four at a time in ascending tile order, each instruction
//                       accumulating its four k into the running sum (generatorSquareMfma's lane map with two operands); below 16 states
//                       the 4 x 4 register blocking with one fused multiply-add per k, k upwards.  The steps past S add 0 x 0.
// Every sum has a fixed order and nothing is accumulated with atomics: a slot's bits depend on its own segments, rate set and category.
#include "kernels.h"
#include "transition_body.h"

namespace mi355 {

namespace {

constexpr int EPOCH_BLOCK = 256;

// (CX: the instance's eigen systems are complex — an instantiation of its own, so that the real one carries none of that path's registers
// and scratch)
template <int S, bool CX>
__global__ __launch_bounds__(64) void k_epochSmall(double* __restrict__ matrices, const double* __restrict__ eigen,
                                                   const double* __restrict__ rates, const int* __restrict__ dSlot,
                                                   const int* __restrict__ dRate, const int* __restrict__ dOff,
                                                   const int* __restrict__ dSegEig, const double* __restrict__ dSegLen,
                                                   int count, int C) {
    constexpr int complexEigen = CX ? 1 : 0;
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t >= count * C) return;
    const int u = t / C, c = t - u * C;
    const size_t eigStride = (size_t)2 * S * S + (complexEigen ? 2 : 1) * S;
    const double rate = rates[(size_t)dRate[u] * C + c];
    const int end = dOff[u + 1];
    int j = dOff[u];
    double P[S * S];
    transitionMatrixThread<S>(P, eigen + eigStride * dSegEig[j], dSegLen[j] * rate, complexEigen);
    for (j++; j < end; j++) {
        double M[S * S];
        transitionMatrixThread<S>(M, eigen + eigStride * dSegEig[j], dSegLen[j] * rate, complexEigen);
#pragma unroll
        for (int i = 0; i < S; i++) {
            double row[S];
#pragma unroll
            for (int q = 0; q < S; q++) {
                double s = 0.0;
#pragma unroll
                for (int k = 0; k < S; k++) s = fma(P[i * S + k], M[k * S + q], s);
                row[q] = s;
            }
#pragma unroll
            for (int q = 0; q < S; q++) P[i * S + q] = row[q];
        }
    }
    double* out = matrices + ((size_t)dSlot[u] * C + c) * S * S;
#pragma unroll
    for (int e = 0; e < S * S; e++) out[e] = P[e];
}

__host__ __device__ inline int epochPadded(int S) { return (S + 3) & ~3; }
__host__ __device__ inline size_t epochLds(int S) { const size_t N = (size_t)epochPadded(S); return 3 * N * (N + 4) * sizeof(double); }

// out = L R on the padded images.  Lane map of v_mfma_f64_4x4x4_4b_f64 (kernels_mfma.hip): block b = (l >> 2) & 3,
// A_b[i = l & 3][k = l >> 4], B_b[k = l >> 4][j = l & 3], D_b[row = l >> 4][col = l & 3].  An item is (tile row it, four tile columns
// 4 jq + b): the four blocks share the A tile and take neighbouring B tiles.  A tile column past the last reads the last one's and is
// not stored.
__device__ __forceinline__ void epochProductMfma(double* __restrict__ out, const double* __restrict__ L, const double* __restrict__ R, int N, int LD) {
    const int nt = N >> 2, nq = (nt + 3) >> 2, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = lane & 3, kk = lane >> 4, b = (lane >> 2) & 3;
    for (int item = wave; item < nt * nq; item += EPOCH_BLOCK / 64) {
        const int it = item / nq, jq = item - it * nq, jt = 4 * jq + b, jtc = jt < nt ? jt : nt - 1;
        const double* pa = L + (size_t)(4 * it + i) * LD + kk;                    // + 4 kt
        const double* pb = R + (size_t)kk * LD + 4 * jtc + i;                       // + 4 kt LD
        double acc = 0.0;
        for (int kt = 0; kt < nt; kt++) acc = __builtin_amdgcn_mfma_f64_4x4x4f64(pa[4 * kt], pb[(size_t)4 * kt * LD], acc, 0, 0, 0);
        if (jt < nt) out[(size_t)(4 * it + kk) * LD + 4 * jt + i] = acc;
    }
}

// ... and with the 4 x 4 register blocking: l upwards, four steps' operands fetched together (rows of the images start on 32-byte boundaries)
__device__ __forceinline__ void epochProductBlocked(double* __restrict__ out, const double* __restrict__ L, const double* __restrict__ R, int N, int LD) {
    const int nb = N >> 2;
    for (int blk = threadIdx.x; blk < nb * nb; blk += blockDim.x) {
        const int bi = blk / nb, bj = blk - bi * nb, i0 = 4 * bi, j0 = 4 * bj;
        double a[4][4] = {{0.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0}};
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
                for (int q = 0; q < 4; q++) v[t][q] = p[q];
            }
#pragma unroll
            for (int t = 0; t < 4; t++)
#pragma unroll
                for (int r = 0; r < 4; r++)
#pragma unroll
                    for (int q = 0; q < 4; q++) a[r][q] = fma(w[r][t], v[t][q], a[r][q]);
        }
#pragma unroll
        for (int r = 0; r < 4; r++)
#pragma unroll
            for (int q = 0; q < 4; q++) out[(i0 + r) * LD + j0 + q] = a[r][q];
    }
}

template <bool MFMA>
__global__ __launch_bounds__(MFMA ? EPOCH_BLOCK : 64) void k_epochBlock(double* __restrict__ matrices, const double* __restrict__ eigen,
                                                                        const double* __restrict__ rates, const int* __restrict__ dSlot,
                                                                        const int* __restrict__ dRate, const int* __restrict__ dOff,
                                                                        const int* __restrict__ dSegEig, const double* __restrict__ dSegLen,
                                                                        int S, int C, int complexEigen) {
    extern __shared__ __attribute__((aligned(32))) double sh[];
    const int N = epochPadded(S), LD = N + 4, tid = threadIdx.x, nthreads = blockDim.x;
    const size_t image = (size_t)N * LD;
    const int u = blockIdx.x, c = blockIdx.y;
    const size_t eigStride = (size_t)2 * S * S + (complexEigen ? 2 : 1) * S;
    const double rate = rates[(size_t)dRate[u] * C + c];
    const int begin = dOff[u], end = dOff[u + 1];                   // (the same in every thread: the barriers below are uniform)
    double* cur = sh;
    double* nxt = sh + image;
    double* seg = sh + 2 * image;
    for (size_t e = tid; e < 3 * image; e += nthreads) sh[e] = 0.0;   // (the padding of the images is zero from here on)
    __syncthreads();
    for (int j = begin; j < end; j++) {
        const double* U = eigen + eigStride * dSegEig[j];
        const double* Ui = U + (size_t)S * S;
        const double* lam = Ui + (size_t)S * S;
        double* dst = j == begin ? cur : seg;
        // (the staging goes where the next product will be written: nobody reads that image before the product has filled it)
        transitionMatrixBody(nxt, U, Ui, lam, S, dSegLen[j] * rate, complexEigen, [dst, LD](int i, int q, double v) { dst[(size_t)i * LD + q] = v; });
        __syncthreads();
        if (j == begin) continue;                                   // (what the staging left in nxt is overwritten by the first product)
        if (MFMA) epochProductMfma(nxt, cur, seg, N, LD); else epochProductBlocked(nxt, cur, seg, N, LD);
        __syncthreads();
        double* swap = cur; cur = nxt; nxt = swap;
    }
    double* M = matrices + ((size_t)dSlot[u] * C + c) * S * S;
    for (int e = tid; e < S * S; e += nthreads) { const int i = e / S, q = e - i * S; M[e] = cur[(size_t)i * LD + q]; }
}

}  // namespace

bool launchEpochMatrices(hipStream_t stream, double* matrices, const double* eigen, const double* rates, const int* dSlot, const int* dRate,
                         const int* dOff, const int* dSegEig, const double* dSegLen, int count, int S, int C, bool complexEigen) {
    if (count <= 0) return true;
    if (S < 1 || S > 64) return false;
    const int cx = complexEigen ? 1 : 0;
    if (S <= 8) {
        const dim3 grid((unsigned)(((size_t)count * C + 63) / 64)), block(64);
#define EPOCH_SMALL(N) case N: \
    if (complexEigen) hipLaunchKernelGGL((k_epochSmall<N, true>), grid, block, 0, stream, matrices, eigen, rates, dSlot, dRate, dOff, dSegEig, dSegLen, count, C); \
    else hipLaunchKernelGGL((k_epochSmall<N, false>), grid, block, 0, stream, matrices, eigen, rates, dSlot, dRate, dOff, dSegEig, dSegLen, count, C); \
    break;
        switch (S) {
            EPOCH_SMALL(1) EPOCH_SMALL(2) EPOCH_SMALL(3) EPOCH_SMALL(4)
            EPOCH_SMALL(5) EPOCH_SMALL(6) EPOCH_SMALL(7) EPOCH_SMALL(8)
        }
#undef EPOCH_SMALL
        return true;
    }
    const size_t lds = epochLds(S);
    const dim3 grid((unsigned)count, (unsigned)C);
    if (S >= 16) {
        if (lds > 65536 && !grantDynamicLds(reinterpret_cast<const void*>(k_epochBlock<true>), lds)) return false;
        hipLaunchKernelGGL(k_epochBlock<true>, grid, dim3(EPOCH_BLOCK), lds, stream, matrices, eigen, rates, dSlot, dRate, dOff, dSegEig, dSegLen, S, C, cx);
    } else {
        hipLaunchKernelGGL(k_epochBlock<false>, grid, dim3(64), lds, stream, matrices, eigen, rates, dSlot, dRate, dOff, dSegEig, dSegLen, S, C, cx);
    }
    return true;
}

}  // namespace mi355
