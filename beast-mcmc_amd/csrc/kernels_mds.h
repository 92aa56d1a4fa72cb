// kernels_mds.h — launchers of csrc/kernels_mds.hip, the three kernels of libmds2_jni.so (include/mds_mi355.h).
//
// Device layout, the same for the three:
//   obs  [n][ld]   the caller's symmetric table, row-major, ld = n rounded up to 16 doubles so that every row starts on a
//                  128-byte line and a pair (j, j + 1), j even, is one aligned 16-byte load; the pad columns are never read
//                  beyond j + 1 with j < n
//   loc  [n][D]    locations, location-major as the caller hands them
// All of it fp64.  D is a template parameter (1..MAX_DIM): a location lives in registers with static indices.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mds {

constexpr int MAX_DIM = 8;
constexpr int TILE = 128;              // full evaluation: a workgroup takes TILE x TILE pairs at a time
constexpr int SUM_BLOCK = 256;
constexpr int MAX_SUM_BLOCKS = 2048;   // grid cap of the full evaluation = length of the partial-sum slab (x 2 doubles)
constexpr int ROW_BLOCK = 1024;        // row update: ONE workgroup (one launch, its reduction needs no second stage)
constexpr int GRAD_BLOCK = 256;
constexpr int GRAD_ROWS_PER_WAVE = 4;
constexpr int GRAD_ROWS = GRAD_ROWS_PER_WAVE * GRAD_BLOCK / 64;
constexpr int MAX_GRAD_BLOCKS = 4096;

struct Point { double v[MAX_DIM]; };   // a location passed by value in the kernel arguments: the row update uploads nothing

inline int64_t leadingDimension(int n) { return ((int64_t)n + 15) & ~(int64_t)15; }

// out[0] = sum over i < j, y_ij not NaN, of (d_ij - y_ij)^2; out[1] = the same sum of log Phi(d_ij sqrt(tau)) when `truncated`,
// else 0.  Two launches: per-workgroup partial sums into slab[2 * MAX_SUM_BLOCKS], then one workgroup adds them in index order.
hipError_t launchSum(hipStream_t stream, int dim, int n, const double* obs, const double* loc, double tau, int truncated,
                     double* slab, double* out);

// Location k moves to `x`: out[0] = ssq + sum_j [(d'_kj - y_kj)^2 - (d_kj - y_kj)^2], out[1] = tr + the same difference of the
// truncation terms, d from loc[k] as it is, d' from x.  Then saved[0..D) = the old loc[k] and loc[k] = x.  One launch.
hipError_t launchRow(hipStream_t stream, int dim, int n, const double* obs, double* loc, int k, const Point& x, double tau,
                     int truncated, double ssq, double tr, double* saved, double* out);

// grad[i][c] = - sum_{j != i, y_ij not NaN, d_ij > 0} [tau (d_ij - y_ij) + truncated sqrt(tau) phi(z)/Phi(z)] (x_ic - x_jc) / d_ij,
// z = d_ij sqrt(tau); each row's sum by one wave in a fixed order.  One launch.
hipError_t launchGradient(hipStream_t stream, int dim, int n, const double* obs, const double* loc, double tau, int truncated,
                          double* grad);

}  // namespace mds
