// kernels_differential.hip — substitution-parameter differential matrices (beagleMi355UpdateDifferentialMatrices, engine_differential.cpp):
// what DifferentiableSubstitutionModelUtil.getExactDifferentialMassMatrix forms per branch and category on the host
// (src/dr/evomodel/substmodel/DifferentiableSubstitutionModelUtil.java:57-171),
//     D = U (V o Phi(dist)) U^-1,   V = U^-1 dQ U with |V_ij| < 1e-10 set to 0,
// formed where the eigen systems, the category rates and the matrix pool already are.  dP / d theta = P D.
//   k_differentialRotate       V once per distinct (eigen system, differential) pair of a call — the reference rotates per branch and category
//   k_differentialSmall<S, complex>  S <= 8: one thread per (branch, category), everything in registers (as k_transition4)
//   k_differentialBlock        9 <= S <= 64: one workgroup per (branch, category); W = V o Phi and T = W U^-1 in LDS (2 S^2 doubles: 64 KiB
//                              at 64 states), both products with the 4 x 4 register blocking of k_transition
//   k_differentialFirstOrder   D = dist dQ
// Every dot product sums its index in ascending order and nothing depends on the position of a branch in the list: a slot receives
// the same bits whatever else the call holds.  The exponent of Phi is formed from the DIFFERENCE (lambda_j - lambda_i) dist, S^2
// exponentials per matrix: the ratio of S exponentials exp(-lambda_i dist) overflows on long branches where the difference does not.
#include "kernels.h"

namespace mi355 {

#define DIFFERENTIAL_THRESHOLD 1e-10      // DifferentiableSubstitutionModelUtil.java:284 (setZeros, and "equal" eigenvalues)

// ---- one entry of W = V o Phi --------------------------------------------------------------------------------------------
// real eigenvalues (lines 76-86): in the reference's order of operations, (V (1 - exp)) / gap, not expm1
__device__ __forceinline__ double differentialRealEntry(double v, double li, double lj, bool diagonal, double dist) {
    const double gap = li - lj;
    if (diagonal || fabs(gap) < DIFFERENTIAL_THRESHOLD) return v * dist;
    return v == 0.0 ? 0.0 : v * (1.0 - exp((lj - li) * dist)) / gap;
}

// integral over [0, t] of exp(a s) cos(b s) and of exp(a s) sin(b s) (lines 210-222)
__device__ __forceinline__ double expCosineIntegral(double t, double a, double b) {
    const double den = a * a + b * b, e = exp(a * t);
    return (b * e * sin(b * t) + a * e * cos(b * t) - a) / den;
}
__device__ __forceinline__ double expSineIntegral(double t, double a, double b) {
    const double den = a * a + b * b, e = exp(a * t);
    return (a * e * sin(b * t) - b * e * cos(b * t) + b) / den;
}

// the first row of the conjugate pair row k belongs to (k itself for a real eigenvalue): as iexpEntry finds it
__device__ __forceinline__ int pairFirstRow(const double* __restrict__ lam, int S, int k) {
    if (lam[S + k] == 0.0) return k;
    int run = 0;
    for (int q = k - 1; q >= 0 && lam[S + q] != 0.0; q--) run++;
    return (run & 1) ? k - 1 : k;
}

// EIGEN_COMPLEX (lines 88-160): an entry that lies in a row or column of a conjugate pair is one component of a 1 x 2, 2 x 1 or 2 x 2
// block; the entry's thread forms the block's integrals and takes its own component.  V is only read (the reference updates in place,
// but no block reads what another wrote).  Kept out of line: the real path of the callers stays small.
__device__ __noinline__ double differentialComplexEntry(const double* __restrict__ V, const double* __restrict__ lam, int S, int i, int j, double dist) {
    const int I = pairFirstRow(lam, S, i), J = pairFirstRow(lam, S, j);
    const bool realI = lam[S + i] == 0.0, realJ = lam[S + j] == 0.0;
    if (realI && realJ) return differentialRealEntry(V[i * S + j], lam[i], lam[j], i == j, dist);
    if (realI) {                                                       // real - complex
        const double a = lam[J] - lam[i], b = lam[S + J];
        const double v0 = V[i * S + J], v1 = V[i * S + J + 1];
        const double ci = expCosineIntegral(dist, a, b), si = expSineIntegral(dist, a, b);
        return j == J ? v0 * ci - v1 * si : v0 * si + v1 * ci;
    }
    if (realJ) {                                                       // complex - real
        const double a = lam[j] - lam[I], b = lam[S + I];
        const double v0 = V[I * S + j], v1 = V[(I + 1) * S + j];
        const double ci = expCosineIntegral(dist, a, b), si = expSineIntegral(dist, a, b);
        return i == I ? v0 * ci - v1 * si : v0 * si + v1 * ci;
    }
    // complex - complex
    const double aI = lam[I], bI = lam[S + I], aJ = lam[J], bJ = lam[S + J];
    const double vij = V[I * S + J], vijp1 = V[I * S + J + 1], vip1j = V[(I + 1) * S + J], vip1jp1 = V[(I + 1) * S + J + 1];
    const bool special = fabs(aI - aJ) < DIFFERENTIAL_THRESHOLD && fabs(bI - bJ) < DIFFERENTIAL_THRESHOLD;
    const double cPlus = special ? sin(2 * bI * dist) / 2 / bI : expCosineIntegral(dist, aJ - aI, bI + bJ);
    const double cMinus = special ? dist : expCosineIntegral(dist, aJ - aI, bI - bJ);
    const double sPlus = special ? (1 - cos(2 * bI * dist)) / 2 / bI : expSineIntegral(dist, aJ - aI, bI + bJ);
    const double sMinus = special ? 0.0 : expSineIntegral(dist, aJ - aI, bI - bJ);
    if (i == I && j == J) return 0.5 * ((vij - vip1jp1) * cPlus + (vij + vip1jp1) * cMinus - (vip1j + vijp1) * sPlus + (vijp1 - vip1j) * sMinus);
    if (i == I) return 0.5 * ((vijp1 + vip1j) * cPlus + (vijp1 - vip1j) * cMinus + (vij - vip1jp1) * sPlus - (vij + vip1jp1) * sMinus);
    if (j == J) return 0.5 * ((vijp1 + vip1j) * cPlus + (vip1j - vijp1) * cMinus + (vij - vip1jp1) * sPlus + (vij + vip1jp1) * sMinus);
    return 0.5 * ((vip1jp1 - vij) * cPlus + (vij + vip1jp1) * cMinus + (vip1j + vijp1) * sPlus + (vijp1 - vip1j) * sMinus);
}

// out[i][j] = sum_k L[i][k] R[k][j] for a 4 x 4 block of entries per thread, k ascending (k_transition's blocking: eight loads per
// sixteen multiply-adds); rows and columns past S are clamped to S - 1 and not stored.  ZERO_SMALL: entries under the threshold become 0.
template <bool ZERO_SMALL>
__device__ __forceinline__ void differentialProduct(double* __restrict__ out, const double* __restrict__ L, const double* __restrict__ R, int S) {
    const int nb = (S + 3) >> 2;
    for (int b = threadIdx.x; b < nb * nb; b += blockDim.x) {
        const int bi = b / nb, bj = b - bi * nb, i0 = 4 * bi, j0 = 4 * bj;
        const double* l0 = L + (size_t)(i0 < S ? i0 : S - 1) * S;
        const double* l1 = L + (size_t)(i0 + 1 < S ? i0 + 1 : S - 1) * S;
        const double* l2 = L + (size_t)(i0 + 2 < S ? i0 + 2 : S - 1) * S;
        const double* l3 = L + (size_t)(i0 + 3 < S ? i0 + 3 : S - 1) * S;
        const int c0 = j0 < S ? j0 : S - 1, c1 = j0 + 1 < S ? j0 + 1 : S - 1, c2 = j0 + 2 < S ? j0 + 2 : S - 1, c3 = j0 + 3 < S ? j0 + 3 : S - 1;
        double a[4][4] = {{0.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0}};
        for (int k = 0; k < S; k++) {
            const double* row = R + (size_t)k * S;
            const double v[4] = {row[c0], row[c1], row[c2], row[c3]};
            const double w[4] = {l0[k], l1[k], l2[k], l3[k]};
#pragma unroll
            for (int r = 0; r < 4; r++)
#pragma unroll
                for (int q = 0; q < 4; q++) a[r][q] += w[r] * v[q];
        }
#pragma unroll
        for (int r = 0; r < 4; r++)
#pragma unroll
            for (int q = 0; q < 4; q++)
                if (i0 + r < S && j0 + q < S)
                    out[(size_t)(i0 + r) * S + j0 + q] = ZERO_SMALL && fabs(a[r][q]) < DIFFERENTIAL_THRESHOLD ? 0.0 : a[r][q];
    }
}

// ---- V = U^-1 (dQ U), thresholded: one workgroup per (eigen system, differential) pair -----------------------------------------
// (both products blocked as above: entry by entry, a thread's S-long chains of dependent loads made the one workgroup of a one-model
// call the longest kernel of the call at 61 states)
__global__ __launch_bounds__(256) void k_differentialRotate(double* __restrict__ Vout, const double* __restrict__ eigen,
                                                            const double* __restrict__ dQ, const int* __restrict__ dPairs, int S,
                                                            int complexEigen) {
    extern __shared__ double sh[];            // dQ U [S][S]
    const int pair = blockIdx.x;
    const size_t eigStride = (size_t)2 * S * S + (complexEigen ? 2 : 1) * S;
    const double* U = eigen + eigStride * dPairs[2 * pair];
    const double* Ui = U + (size_t)S * S;
    differentialProduct<false>(sh, dQ + (size_t)dPairs[2 * pair + 1] * S * S, U, S);
    __syncthreads();
    differentialProduct<true>(Vout + (size_t)pair * S * S, Ui, sh, S);
}

void launchDifferentialRotate(hipStream_t stream, double* V, const double* eigen, const double* dQ, const int* dPairs, int pairCount,
                              int S, bool complexEigen) {
    if (pairCount <= 0) return;
    hipLaunchKernelGGL(k_differentialRotate, dim3((unsigned)pairCount), dim3(S * S >= 256 ? 256 : 64), (size_t)S * S * sizeof(double), stream,
                       V, eigen, dQ, dPairs, S, complexEigen ? 1 : 0);
}

// ---- S <= 8: one thread per (branch, category) -------------------------------------------------------------------------
// (out of line here: with the exponential inlined S^2 times the compiler forms them side by side, and their temporaries next to T spill
// at 7 and 8 states)
__device__ __noinline__ double differentialRealEntryCall(double v, double li, double lj, bool diagonal, double dist) {
    return differentialRealEntry(v, li, lj, diagonal, dist);
}

// T = W U^-1 stays in registers (S^2 doubles: 128 VGPRs at 8 states), W is formed a row at a time; then D = U T.
template <int S, bool COMPLEX>
__global__ __launch_bounds__(256) void k_differentialSmall(double* __restrict__ matrices, const double* __restrict__ eigen,
                                                           const double* __restrict__ rates, const double* __restrict__ Vall,
                                                           const int* __restrict__ dIdx, const double* __restrict__ dLen,
                                                           const int* __restrict__ dEig, const int* __restrict__ dRate,
                                                           const int* __restrict__ dPair, int count, int C) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= count * C) return;
    const int u = t / C, c = t - u * C;
    const double* U = eigen + (size_t)(2 * S * S + (COMPLEX ? 2 : 1) * S) * dEig[u];
    const double* Ui = U + S * S;
    const double* lam = U + 2 * S * S;
    const double* V = Vall + (size_t)dPair[u] * S * S;
    const double dist = dLen[u] * rates[(size_t)dRate[u] * C + c];
    double T[S * S];
#pragma unroll
    for (int i = 0; i < S; i++) {
        double w[S];
#pragma unroll
        for (int k = 0; k < S; k++)
            w[k] = COMPLEX ? differentialComplexEntry(V, lam, S, i, k, dist) : differentialRealEntryCall(V[i * S + k], lam[i], lam[k], i == k, dist);
#pragma unroll
        for (int j = 0; j < S; j++) {
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < S; k++) s += w[k] * Ui[k * S + j];
            T[i * S + j] = s;
        }
    }
    double* M = matrices + ((size_t)dIdx[u] * C + c) * S * S;
#pragma unroll
    for (int i = 0; i < S; i++)
#pragma unroll
        for (int j = 0; j < S; j++) {
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < S; k++) s += U[i * S + k] * T[k * S + j];
            M[i * S + j] = s;
        }
}

// ---- 9 <= S <= 64: one workgroup per (branch, category) ----------------------------------------------------------------
__global__ __launch_bounds__(256) void k_differentialBlock(double* __restrict__ matrices, const double* __restrict__ eigen,
                                                           const double* __restrict__ rates, const double* __restrict__ Vall,
                                                           const int* __restrict__ dIdx, const double* __restrict__ dLen,
                                                           const int* __restrict__ dEig, const int* __restrict__ dRate,
                                                           const int* __restrict__ dPair, int S, int C, int complexEigen) {
    extern __shared__ double sh[];            // W [S][S] | T [S][S]
    double* W = sh;
    double* T = sh + (size_t)S * S;
    const int u = blockIdx.x, c = blockIdx.y;
    const size_t eigStride = (size_t)2 * S * S + (complexEigen ? 2 : 1) * S;
    const double* U = eigen + eigStride * dEig[u];
    const double* Ui = U + (size_t)S * S;
    const double* lam = Ui + (size_t)S * S;
    const double* V = Vall + (size_t)dPair[u] * S * S;
    const double dist = dLen[u] * rates[(size_t)dRate[u] * C + c];
    for (int e = threadIdx.x; e < S * S; e += blockDim.x) {
        const int i = e / S, j = e - i * S;
        W[e] = complexEigen ? differentialComplexEntry(V, lam, S, i, j, dist) : differentialRealEntry(V[e], lam[i], lam[j], i == j, dist);
    }
    __syncthreads();
    differentialProduct<false>(T, W, Ui, S);        // U^-1 streams from L2: the whole grid shares it
    __syncthreads();
    differentialProduct<false>(matrices + ((size_t)dIdx[u] * C + c) * S * S, U, T, S);
}

void launchDifferentialExact(hipStream_t stream, double* matrices, const double* eigen, const double* rates, const double* V,
                             const int* dIdx, const double* dLen, const int* dEig, const int* dRate, const int* dPair,
                             int count, int S, int C, bool complexEigen) {
    if (count <= 0) return;
    const int cx = complexEigen ? 1 : 0;
    if (S <= 8) {
        const dim3 grid((unsigned)(((size_t)count * C + 255) / 256)), block(256);
#define DIFFERENTIAL_SMALL(N) case N: \
            if (complexEigen) hipLaunchKernelGGL((k_differentialSmall<N, true>), grid, block, 0, stream, matrices, eigen, rates, V, dIdx, dLen, dEig, dRate, dPair, count, C); \
            else hipLaunchKernelGGL((k_differentialSmall<N, false>), grid, block, 0, stream, matrices, eigen, rates, V, dIdx, dLen, dEig, dRate, dPair, count, C); \
            break;
        switch (S) {
            DIFFERENTIAL_SMALL(1) DIFFERENTIAL_SMALL(2) DIFFERENTIAL_SMALL(3) DIFFERENTIAL_SMALL(4)
            DIFFERENTIAL_SMALL(5) DIFFERENTIAL_SMALL(6) DIFFERENTIAL_SMALL(7) DIFFERENTIAL_SMALL(8)
        }
#undef DIFFERENTIAL_SMALL
        return;
    }
    hipLaunchKernelGGL(k_differentialBlock, dim3((unsigned)count, (unsigned)C), dim3(S * S >= 256 ? 256 : 64),
                       (size_t)2 * S * S * sizeof(double), stream, matrices, eigen, rates, V, dIdx, dLen, dEig, dRate, dPair, S, C, cx);
}

// ---- D = dist dQ: a thread per entry ------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_differentialFirstOrder(double* __restrict__ matrices, const double* __restrict__ rates,
                                                                const double* __restrict__ dQ, const int* __restrict__ dIdx,
                                                                const double* __restrict__ dLen, const int* __restrict__ dRate,
                                                                const int* __restrict__ dDiff, size_t total, int S, int C) {
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const int per = S * S;
    const size_t m = t / per;
    const int e = (int)(t - m * per), u = (int)(m / C), c = (int)(m - (size_t)u * C);
    const double dist = dLen[u] * rates[(size_t)dRate[u] * C + c];
    matrices[((size_t)dIdx[u] * C + c) * per + e] = dist * dQ[(size_t)dDiff[u] * per + e];
}

void launchDifferentialFirstOrder(hipStream_t stream, double* matrices, const double* rates, const double* dQ, const int* dIdx,
                                  const double* dLen, const int* dRate, const int* dDiff, int count, int S, int C) {
    if (count <= 0) return;
    const size_t total = (size_t)count * C * S * S;
    hipLaunchKernelGGL(k_differentialFirstOrder, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, matrices, rates, dQ, dIdx,
                       dLen, dRate, dDiff, total, S, C);
}

}  // namespace mi355
