// transition_body.h — the arithmetic of ONE transition matrix U exp(Lambda d) U^-1, shared by the kernels that form one: k_transition,
// k_transition4 and k_transition4Fused (kernels.hip) and the epoch kernels (kernels_epoch.hip), which need the same bits without a
// round trip through a matrix slot.  A file that includes this must be compiled with the contraction kernels.hip is compiled with
// (the compiler's default: no "#pragma clang fp contract(off)"), or the sums below round differently.
#pragma once
#include <hip/hip_runtime.h>

namespace mi355 {

// complexEigen (an EIGEN_COMPLEX instance: BeagleTreeLikelihood.java:353-355, the asymmetric discrete-trait models): the
// eigenvalue array holds S real parts, then S imaginary parts, and U / U^-1 are the REAL block form — a conjugate pair
// a +/- b i sits in rows i, i+1 (imaginary parts b, -b) and contributes exp(a t) [cos b t, sin b t; -sin b t, cos b t] on those
// two rows of U^-1 (ComplexSubstitutionModel.java:121-173).  Row k of a pair is its FIRST row iff an even number of rows
// with a nonzero imaginary part precede it without a gap (the reference walks the rows in order and skips the second).
__device__ __forceinline__ double iexpEntry(const double* __restrict__ Ui, const double* __restrict__ lam, int S, int k, int j, double dist, int complexEigen) {
    const double im = complexEigen ? lam[S + k] : 0.0;
    if (im == 0.0) return Ui[k * S + j] * exp(dist * lam[k]);
    int run = 0;
    for (int q = k - 1; q >= 0 && lam[S + q] != 0.0; q--) run++;
    const int first = (run & 1) ? k - 1 : k;
    const double b = lam[S + first];
    const double expat = exp(dist * lam[first]), c = expat * cos(dist * b), sn = expat * sin(dist * b);
    return first == k ? c * Ui[k * S + j] + sn * Ui[(k + 1) * S + j] : c * Ui[k * S + j] - sn * Ui[(k - 1) * S + j];
}

// A workgroup forms one matrix.  sh: S * S + S doubles of LDS (iexp[S][S] | exp(dist lambda_k)[S]); put(i, j, value) receives every entry
// i, j < S once, negative sums already clamped to 0.  Every thread of the workgroup must call it (it holds barriers); what put wrote is
// the caller's to publish.
template <class Put>
__device__ __forceinline__ void transitionMatrixBody(double* __restrict__ sh, const double* __restrict__ U, const double* __restrict__ Ui,
                                                     const double* __restrict__ lam, int S, double dist, int complexEigen, Put put) {
    // (one exponential per eigenvalue, not per entry: S instead of S x S of them — 3 721 at 61 states — the same values)
    double* ek = sh + (size_t)S * S;
    if (!complexEigen) {
        for (int k = threadIdx.x; k < S; k += blockDim.x) ek[k] = exp(dist * lam[k]);
        __syncthreads();
    }
    for (int e = threadIdx.x; e < S * S; e += blockDim.x) {
        const int k = e / S;
        sh[e] = complexEigen ? iexpEntry(Ui, lam, S, k, e - k * S, dist, 1) : Ui[e] * ek[k];
    }
    __syncthreads();
    // a thread forms a 4 x 4 block of entries: eight loads per sixteen multiply-adds instead of two per one (round 6: the 1 592 matrices
    // of a 61-state evaluation 127 -> ~40 us); every entry still sums over k in ascending order — the same bits as entry by entry
    const int nb = (S + 3) >> 2;
    for (int b = threadIdx.x; b < nb * nb; b += blockDim.x) {
        const int bi = b / nb, bj = b - bi * nb, i0 = 4 * bi, j0 = 4 * bj;
        const double* u0 = U + (size_t)(i0 < S ? i0 : S - 1) * S;
        const double* u1 = U + (size_t)(i0 + 1 < S ? i0 + 1 : S - 1) * S;
        const double* u2 = U + (size_t)(i0 + 2 < S ? i0 + 2 : S - 1) * S;
        const double* u3 = U + (size_t)(i0 + 3 < S ? i0 + 3 : S - 1) * S;
        const int c0 = j0 < S ? j0 : S - 1, c1 = j0 + 1 < S ? j0 + 1 : S - 1, c2 = j0 + 2 < S ? j0 + 2 : S - 1, c3 = j0 + 3 < S ? j0 + 3 : S - 1;
        double a[4][4] = {{0.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0}};
        for (int k = 0; k < S; k++) {
            const double* row = sh + (size_t)k * S;
            const double v[4] = {row[c0], row[c1], row[c2], row[c3]};
            const double w[4] = {u0[k], u1[k], u2[k], u3[k]};
#pragma unroll
            for (int r = 0; r < 4; r++)
#pragma unroll
                for (int q = 0; q < 4; q++) a[r][q] += w[r] * v[q];
        }
#pragma unroll
        for (int r = 0; r < 4; r++)
#pragma unroll
            for (int q = 0; q < 4; q++)
                if (i0 + r < S && j0 + q < S) put(i0 + r, j0 + q, a[r][q] > 0.0 ? a[r][q] : 0.0);
    }
}

// A thread forms one matrix of S states into M[S * S] (row-major), the same arithmetic and summation order: what k_transition4 runs at S = 4.
// U: the eigen system [U | U^-1 | lambda] of S states.
template <int S>
__device__ __forceinline__ void transitionMatrixThread(double (&M)[S * S], const double* __restrict__ U, double dist, int complexEigen) {
    const double* Ui = U + S * S;
    const double* lam = U + 2 * S * S;
    double ie[S * S];
    if (complexEigen) {
        for (int e = 0; e < S * S; e++) ie[e] = iexpEntry(Ui, lam, S, e / S, e % S, dist, 1);
    } else {
#pragma unroll
        for (int k = 0; k < S; k++) {
            const double ex = exp(dist * lam[k]);
#pragma unroll
            for (int j = 0; j < S; j++) ie[k * S + j] = Ui[k * S + j] * ex;
        }
    }
#pragma unroll
    for (int i = 0; i < S; i++)
#pragma unroll
        for (int j = 0; j < S; j++) {
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < S; k++) s += U[i * S + k] * ie[k * S + j];
            M[i * S + j] = s > 0.0 ? s : 0.0;
        }
}

}  // namespace mi355
