// kernels_mds.hip — multidimensional scaling on gfx950: the sum of increments over all pairs, its change when one location
// moves, and the gradient with respect to every location (include/mds_mi355.h states the arithmetic; kernels_mds.h the layout).
//
// Every sum is made in an order that depends on the sizes alone: a lane adds its own pairs in index order, a wave adds its 64
// lanes by a butterfly of shuffles, a workgroup adds its waves in wave order, the grid's partial sums are stored and added by
// one workgroup in index order.  No floating-point atomics anywhere, so the same inputs give the same bits on every run.
//
// Bounds: a thread reads obs[i * ld + j] (two doubles) only with i < n and even j < n, and ld is even and >= n; loc[j * D + c]
// only with j < n; it writes grad[i * D + c] only with i < n, slab[2 * block + {0, 1}] with block < gridDim.x <=
// MAX_SUM_BLOCKS, out[0..1], saved[0..D) and loc[k * D + c] with k < n checked by the host.
#include "kernels_mds.h"

namespace mds {
namespace {

constexpr double INV_SQRT2 = 0.70710678118654752440;
constexpr double INV_SQRT_2PI = 0.39894228040143267794;

// log Phi(z) for z >= 0 (a distance times sqrt(tau)): Phi = 1 - erfc(z / sqrt 2) / 2 lies in [1/2, 1), so log1p of the small
// negative number keeps full relative accuracy of log Phi as z grows.
__device__ inline double logPhi(double z) { return log1p(-0.5 * erfc(z * INV_SQRT2)); }
// phi(z) / Phi(z), z >= 0
__device__ inline double hazard(double z) { return INV_SQRT_2PI * exp(-0.5 * z * z) / (1.0 - 0.5 * erfc(z * INV_SQRT2)); }

__device__ inline double waveSum(double v) {
#pragma unroll
    for (int offset = 32; offset > 0; offset >>= 1) v += __shfl_xor(v, offset, 64);
    return v;
}

template <int D>
__device__ inline double distance(const double* a, const double (&b)[D]) {
    double s = 0.0;
#pragma unroll
    for (int c = 0; c < D; ++c) {
        const double t = a[c] - b[c];
        s += t * t;
    }
    return sqrt(s);
}

template <int D>
__device__ inline void loadPoint(const double* loc, int64_t j, int n, double (&x)[D]) {
#pragma unroll
    for (int c = 0; c < D; ++c) x[c] = j < n ? loc[j * D + c] : 0.0;
}

// ---------------------------------------------------------------------------------------------------------------------------
// Full evaluation.  The table is cut into TILE x TILE tiles; a workgroup walks the tiles of the upper triangle (bj >= bi) with
// the grid's stride.  The tile's TILE row locations sit in LDS (read as a broadcast: a wave works on one row at a time), each
// lane keeps the two column locations of its pair (j, j + 1) in registers and reads y as one 16-byte load, 1 KiB per wave and
// row.  A wave takes rows wave, wave + 4, ...
template <int D, bool TRUNCATED>
__global__ __launch_bounds__(SUM_BLOCK) void mdsSumKernel(int n, int64_t ld, const double* __restrict__ obs,
                                                          const double* __restrict__ loc, double sqrtTau, int tilesPerSide,
                                                          double* __restrict__ slab) {
    __shared__ double rows[TILE * D];
    __shared__ double waveSums[2 * SUM_BLOCK / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t tiles = (int64_t)tilesPerSide * tilesPerSide;
    double ssq = 0.0, tr = 0.0;
    for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int bi = (int)(t / tilesPerSide), bj = (int)(t % tilesPerSide);
        if (bj < bi) continue;                                   // the same for the whole workgroup
        const int64_t i0 = (int64_t)bi * TILE, j = (int64_t)bj * TILE + 2 * lane;
        __syncthreads();                                         // the previous tile's rows have been read
        for (int e = tid; e < TILE * D; e += SUM_BLOCK) rows[e] = i0 * D + e < (int64_t)n * D ? loc[i0 * D + e] : 0.0;
        __syncthreads();
        if (j >= n) continue;                                    // no barrier below this line in the loop body
        double x0[D], x1[D];
        loadPoint<D>(loc, j, n, x0);
        loadPoint<D>(loc, j + 1, n, x1);
        const bool second = j + 1 < n;
        // rows of this tile that exist; on a diagonal tile the pairs on or below the diagonal are read and masked out (one tile
        // in tilesPerSide), so that the loop has no exit and its loads can be issued ahead
        const int rowCount = (int)(n - i0 < TILE ? n - i0 : TILE);
#pragma unroll 4
        for (int r = wave; r < rowCount; r += SUM_BLOCK / 64) {
            const int64_t i = i0 + r;
            const double2 y = *reinterpret_cast<const double2*>(obs + i * ld + j);
            const bool use0 = j > i && y.x == y.x, use1 = second && j + 1 > i && y.y == y.y;
            const double d0 = distance<D>(rows + r * D, x0), d1 = distance<D>(rows + r * D, x1);
            const double r0 = d0 - y.x, r1 = d1 - y.y;
            ssq += use0 ? r0 * r0 : 0.0;
            ssq += use1 ? r1 * r1 : 0.0;
            if (TRUNCATED) {
                if (use0) tr += logPhi(d0 * sqrtTau);
                if (use1) tr += logPhi(d1 * sqrtTau);
            }
        }
    }
    ssq = waveSum(ssq);
    tr = waveSum(tr);
    __syncthreads();
    if (lane == 0) {
        waveSums[2 * wave] = ssq;
        waveSums[2 * wave + 1] = tr;
    }
    __syncthreads();
    if (tid == 0) {
        double a = 0.0, b = 0.0;
        for (int w = 0; w < SUM_BLOCK / 64; ++w) {
            a += waveSums[2 * w];
            b += waveSums[2 * w + 1];
        }
        slab[2 * blockIdx.x] = a;
        slab[2 * blockIdx.x + 1] = b;
    }
}

// second stage: thread t adds partial sums t, t + 256, ... in that order, the workgroup adds its threads as above
__global__ __launch_bounds__(SUM_BLOCK) void mdsFinishKernel(const double* __restrict__ slab, int count, double* __restrict__ out) {
    __shared__ double waveSums[2 * SUM_BLOCK / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double a = 0.0, b = 0.0;
    for (int k = tid; k < count; k += SUM_BLOCK) {
        a += slab[2 * k];
        b += slab[2 * k + 1];
    }
    a = waveSum(a);
    b = waveSum(b);
    if (lane == 0) {
        waveSums[2 * wave] = a;
        waveSums[2 * wave + 1] = b;
    }
    __syncthreads();
    if (tid == 0) {
        a = b = 0.0;
        for (int w = 0; w < SUM_BLOCK / 64; ++w) {
            a += waveSums[2 * w];
            b += waveSums[2 * w + 1];
        }
        out[0] = a;
        out[1] = b;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// Row update: one workgroup of ROW_BLOCK threads over row k of the table.  The old location is read from loc[k] by every thread
// before the barrier and replaced after it; no other thread reads loc[k] (pair (k, k) is skipped).
template <int D>
__global__ __launch_bounds__(ROW_BLOCK) void mdsRowKernel(int n, int64_t ld, const double* __restrict__ obs, double* loc, int k,
                                                          Point moved, double sqrtTau, int truncated, double ssqOld, double trOld,
                                                          double* __restrict__ saved, double* __restrict__ out) {
    __shared__ double waveSums[2 * ROW_BLOCK / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double was[D], now[D];
#pragma unroll
    for (int c = 0; c < D; ++c) {
        was[c] = loc[(int64_t)k * D + c];
        now[c] = moved.v[c];
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < D; ++c)
        if (tid == c) {
            saved[c] = was[c];
            loc[(int64_t)k * D + c] = now[c];
        }
    double ssq = 0.0, tr = 0.0;
    const double* row = obs + (int64_t)k * ld;
    for (int64_t j = 2 * tid; j < n; j += 2 * ROW_BLOCK) {
        const double2 y = *reinterpret_cast<const double2*>(row + j);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int64_t jj = j + h;
            const double yy = h ? y.y : y.x;
            if (jj >= n || jj == k || yy != yy) continue;
            double x[D];
            loadPoint<D>(loc, jj, n, x);
            const double dNew = distance<D>(now, x), dOld = distance<D>(was, x);
            const double rNew = dNew - yy, rOld = dOld - yy;
            ssq += rNew * rNew - rOld * rOld;
            if (truncated) tr += logPhi(dNew * sqrtTau) - logPhi(dOld * sqrtTau);
        }
    }
    ssq = waveSum(ssq);
    tr = waveSum(tr);
    if (lane == 0) {
        waveSums[2 * wave] = ssq;
        waveSums[2 * wave + 1] = tr;
    }
    __syncthreads();
    if (tid == 0) {
        double a = 0.0, b = 0.0;
        for (int w = 0; w < ROW_BLOCK / 64; ++w) {
            a += waveSums[2 * w];
            b += waveSums[2 * w + 1];
        }
        out[0] = ssqOld + a;
        out[1] = trOld + b;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// Gradient: a wave owns GRAD_ROWS_PER_WAVE rows and walks the whole table row, 128 columns at a time; a lane's two column
// locations are loaded once and used for all of the wave's rows.  Nothing is scattered to x_j: the table is symmetric, every row
// is read, 8 n^2 bytes.
template <int D, bool TRUNCATED>
__global__ __launch_bounds__(GRAD_BLOCK) void mdsGradientKernel(int n, int64_t ld, const double* __restrict__ obs,
                                                                const double* __restrict__ loc, double tau, double sqrtTau,
                                                                double* __restrict__ grad) {
    constexpr int R = GRAD_ROWS_PER_WAVE;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t strips = ((int64_t)n + GRAD_ROWS - 1) / GRAD_ROWS;
    for (int64_t strip = blockIdx.x; strip < strips; strip += gridDim.x) {
        const int64_t i0 = strip * GRAD_ROWS + wave * R;
        if (i0 >= n) continue;                                   // no barrier in this kernel
        double xi[R][D], acc[R][D];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            loadPoint<D>(loc, i0 + r, n, xi[r]);
#pragma unroll
            for (int c = 0; c < D; ++c) acc[r][c] = 0.0;
        }
        for (int64_t j = 2 * lane; j < n; j += 128) {
            double xj[2][D];
            loadPoint<D>(loc, j, n, xj[0]);
            loadPoint<D>(loc, j + 1, n, xj[1]);
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int64_t i = i0 + r;
                if (i >= n) continue;
                const double2 y = *reinterpret_cast<const double2*>(obs + i * ld + j);
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int64_t jj = j + h;
                    const double yy = h ? y.y : y.x;
                    if (jj >= n || jj == i || yy != yy) continue;
                    const double d = distance<D>(xi[r], xj[h]);
                    if (!(d > 0.0)) continue;                    // coincident locations: no direction, no contribution
                    double coef = tau * (d - yy);
                    if (TRUNCATED) coef += sqrtTau * hazard(d * sqrtTau);
                    coef /= d;
#pragma unroll
                    for (int c = 0; c < D; ++c) acc[r][c] -= coef * (xi[r][c] - xj[h][c]);
                }
            }
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
#pragma unroll
            for (int c = 0; c < D; ++c) {
                const double total = waveSum(acc[r][c]);
                if (lane == 0 && i0 + r < n) grad[(i0 + r) * D + c] = total;
            }
        }
    }
}

template <int D>
hipError_t sumD(hipStream_t stream, int n, const double* obs, const double* loc, double tau, int truncated, double* slab, double* out) {
    const int side = (n + TILE - 1) / TILE;
    const int64_t tiles = (int64_t)side * side;
    const int blocks = (int)(tiles < MAX_SUM_BLOCKS ? tiles : MAX_SUM_BLOCKS);
    if (truncated)
        hipLaunchKernelGGL((mdsSumKernel<D, true>), dim3(blocks), dim3(SUM_BLOCK), 0, stream, n, leadingDimension(n), obs, loc, sqrt(tau), side,
                           slab);
    else
        hipLaunchKernelGGL((mdsSumKernel<D, false>), dim3(blocks), dim3(SUM_BLOCK), 0, stream, n, leadingDimension(n), obs, loc, sqrt(tau), side,
                           slab);
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return err;
    hipLaunchKernelGGL(mdsFinishKernel, dim3(1), dim3(SUM_BLOCK), 0, stream, slab, blocks, out);
    return hipGetLastError();
}

template <int D>
hipError_t rowD(hipStream_t stream, int n, const double* obs, double* loc, int k, const Point& x, double tau, int truncated, double ssq,
                double tr, double* saved, double* out) {
    hipLaunchKernelGGL(mdsRowKernel<D>, dim3(1), dim3(ROW_BLOCK), 0, stream, n, leadingDimension(n), obs, loc, k, x, sqrt(tau), truncated,
                       ssq, tr, saved, out);
    return hipGetLastError();
}

template <int D>
hipError_t gradientD(hipStream_t stream, int n, const double* obs, const double* loc, double tau, int truncated, double* grad) {
    const int64_t strips = ((int64_t)n + GRAD_ROWS - 1) / GRAD_ROWS;
    const int blocks = (int)(strips < MAX_GRAD_BLOCKS ? strips : MAX_GRAD_BLOCKS);
    if (truncated)
        hipLaunchKernelGGL((mdsGradientKernel<D, true>), dim3(blocks), dim3(GRAD_BLOCK), 0, stream, n, leadingDimension(n), obs, loc, tau,
                           sqrt(tau), grad);
    else
        hipLaunchKernelGGL((mdsGradientKernel<D, false>), dim3(blocks), dim3(GRAD_BLOCK), 0, stream, n, leadingDimension(n), obs, loc, tau,
                           sqrt(tau), grad);
    return hipGetLastError();
}

}  // namespace

hipError_t launchSum(hipStream_t stream, int dim, int n, const double* obs, const double* loc, double tau, int truncated, double* slab,
                     double* out) {
#define MDS_ARGS (stream, n, obs, loc, tau, truncated, slab, out)
    switch (dim) {
        case 1: return sumD<1> MDS_ARGS;
        case 2: return sumD<2> MDS_ARGS;
        case 3: return sumD<3> MDS_ARGS;
        case 4: return sumD<4> MDS_ARGS;
        case 5: return sumD<5> MDS_ARGS;
        case 6: return sumD<6> MDS_ARGS;
        case 7: return sumD<7> MDS_ARGS;
        case 8: return sumD<8> MDS_ARGS;
        default: return hipErrorInvalidValue;
    }
#undef MDS_ARGS
}

hipError_t launchRow(hipStream_t stream, int dim, int n, const double* obs, double* loc, int k, const Point& x, double tau, int truncated,
                     double ssq, double tr, double* saved, double* out) {
#define MDS_ARGS (stream, n, obs, loc, k, x, tau, truncated, ssq, tr, saved, out)
    switch (dim) {
        case 1: return rowD<1> MDS_ARGS;
        case 2: return rowD<2> MDS_ARGS;
        case 3: return rowD<3> MDS_ARGS;
        case 4: return rowD<4> MDS_ARGS;
        case 5: return rowD<5> MDS_ARGS;
        case 6: return rowD<6> MDS_ARGS;
        case 7: return rowD<7> MDS_ARGS;
        case 8: return rowD<8> MDS_ARGS;
        default: return hipErrorInvalidValue;
    }
#undef MDS_ARGS
}

hipError_t launchGradient(hipStream_t stream, int dim, int n, const double* obs, const double* loc, double tau, int truncated,
                          double* grad) {
#define MDS_ARGS (stream, n, obs, loc, tau, truncated, grad)
    switch (dim) {
        case 1: return gradientD<1> MDS_ARGS;
        case 2: return gradientD<2> MDS_ARGS;
        case 3: return gradientD<3> MDS_ARGS;
        case 4: return gradientD<4> MDS_ARGS;
        case 5: return gradientD<5> MDS_ARGS;
        case 6: return gradientD<6> MDS_ARGS;
        case 7: return gradientD<7> MDS_ARGS;
        case 8: return gradientD<8> MDS_ARGS;
        default: return hipErrorInvalidValue;
    }
#undef MDS_ARGS
}

}  // namespace mds
