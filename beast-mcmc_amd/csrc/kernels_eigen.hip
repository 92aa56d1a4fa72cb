// kernels_eigen.hip — eigen systems of time-reversible substitution models (beagleMi355SetReversibleModels, engine_eigen.cpp): what the
// caller of setEigenDecomposition computes per model on the host (BaseSubstitutionModel.java:256-289, 314-319), formed where the eigen
// slots are.  With A = Pi^1/2 Q Pi^-1/2 symmetric,
//     A = V diag(mu) V^T,   U = Pi^-1/2 V,   U^-1 = V^T Pi^1/2,   lambda = mu / n,   n = -sum_i pi_i Q_ii,
// by cyclic Jacobi in the round-robin tournament order: n' - 1 rounds of n' / 2 disjoint pairs per sweep, n' = S rounded up to even
// (odd S: player S idles).  Pair 0 of round r is (r, n' - 1), pair k is ((r + k) mod (n' - 1), (r - k) mod (n' - 1)).
//   k_eigenSmall<S>   S <= 8: one model per thread, A (upper triangle) and V in registers, every index a compile-time constant
//   k_eigenBlock<players>  9 <= S <= 64: one workgroup of 256 threads per model, A and V in LDS with an odd row stride (a column access
//                     walks the banks); a round = the angles of its pairs, a barrier, then the 2 x 2 blocks (row pair, column pair) of the
//                     upper block triangle, each rotated by its row pair first and its column pair second and written with its mirror
//                     image — A stays symmetric to the bit — next to the column pairs of V, a barrier.  What a thread updates is fixed for
//                     the model and held in registers; the three instantiations size those register arrays (22, 44, 64 players)
// The angle is t = sign(theta) / (|theta| + sqrt(theta^2 + 1)), theta = (a_qq - a_pp) / 2 a_pq; a pair with a_pq == 0 is not rotated.
// sqrt and / are the IEEE ones (the library is built without fast-math).  A sweep starts with the test off(A) <= eps ||A||_F, ||A||_F
// taken once; EIGEN_SWEEP_CAP sweeps without passing it leave NaN eigenvalues.  Eigenvalues leave in ascending order (ties by index).
// A model's output depends on its own rates and frequencies only: no sum runs over anything but the model's own entries in a fixed order.
#include "kernels.h"

namespace mi355 {

#define EIGEN_EPS 2.220446049250313e-16

struct EigenAngle { double c, s, t; };

__device__ __forceinline__ EigenAngle eigenAngle(double app, double aqq, double apq) {
    EigenAngle r;
    if (apq == 0.0) { r.c = 1.0; r.s = 0.0; r.t = 0.0; return r; }
    const double theta = (aqq - app) / (2.0 * apq);
    const double mag = fabs(theta);
    double t;
    if (mag > 1e150) t = 1.0 / (2.0 * theta);                       // theta^2 would overflow
    else { t = 1.0 / (mag + sqrt(theta * theta + 1.0)); if (theta < 0.0) t = -t; }
    r.t = t;
    r.c = 1.0 / sqrt(t * t + 1.0);
    r.s = t * r.c;
    return r;
}

// ---- S <= 8: a model per thread ---------------------------------------------------------------------------------------------
template <int S>
__global__ __launch_bounds__(64) void k_eigenSmall(double* __restrict__ eigen, const double* __restrict__ models,
                                                   const int* __restrict__ slots, int* __restrict__ sweepsOut, int count, int nLambda) {
    constexpr int N = S + (S & 1), M = N / 2, R = S * (S - 1) / 2;
    const int model = blockIdx.x * 64 + threadIdx.x;
    if (model >= count) return;
    const double* rates = models + (size_t)model * (R + S);
    const double* pi = rates + R;
    double sq[S], a[S][S], v[S][S];          // a: entries i <= j only
#pragma unroll
    for (int i = 0; i < S; i++) sq[i] = sqrt(pi[i]);
    double diag[S];
#pragma unroll
    for (int i = 0; i < S; i++) diag[i] = 0.0;
#pragma unroll
    for (int i = 0; i < S; i++)
#pragma unroll
        for (int j = 0; j < S; j++) {
            if (i == j) continue;
            const int lo = i < j ? i : j, hi = i < j ? j : i;
            const double r = rates[lo * S - lo * (lo + 1) / 2 + (hi - lo - 1)];
            diag[i] -= r * pi[j];
            if (i < j) a[i][j] = (sq[i] * r) * sq[j];
        }
    double norm = 0.0, norm2 = 0.0;
#pragma unroll
    for (int i = 0; i < S; i++) {
        a[i][i] = diag[i];
        norm -= pi[i] * diag[i];
        norm2 += diag[i] * diag[i];
#pragma unroll
        for (int j = 0; j < S; j++) v[i][j] = i == j ? 1.0 : 0.0;
    }
    double upper2 = 0.0;
#pragma unroll
    for (int i = 0; i < S; i++)
#pragma unroll
        for (int j = i + 1; j < S; j++) upper2 += a[i][j] * a[i][j];
    norm2 += 2.0 * upper2;
    int sweeps = 0;
    bool capped = false;
    for (;;) {
        double off2 = 0.0;
#pragma unroll
        for (int i = 0; i < S; i++)
#pragma unroll
            for (int j = i + 1; j < S; j++) off2 += a[i][j] * a[i][j];
        off2 *= 2.0;
        if (off2 <= EIGEN_EPS * EIGEN_EPS * norm2) break;
        if (sweeps == EIGEN_SWEEP_CAP || !(norm2 < INFINITY)) { capped = true; break; }
#pragma unroll
        for (int r = 0; r < N - 1; r++)
#pragma unroll
            for (int k = 0; k < M; k++) {
                const int x = (r + k) % (N - 1), y = k == 0 ? N - 1 : (r - k + (N - 1)) % (N - 1);
                const int p = x < y ? x : y, q = x < y ? y : x;
                if (q >= S) continue;                               // the idle player
                const EigenAngle g = eigenAngle(a[p][p], a[q][q], a[p][q]);
                if (g.s == 0.0 && g.c == 1.0) continue;
#pragma unroll
                for (int j = 0; j < S; j++) {
                    if (j == p || j == q) continue;
                    // a(j, p) and a(j, q) where they are kept
                    double& ap = j < p ? a[j][p] : a[p][j];
                    double& aq = j < q ? a[j][q] : a[q][j];
                    const double u = ap, w = aq;
                    ap = g.c * u - g.s * w;
                    aq = g.s * u + g.c * w;
                }
                const double apq = a[p][q];
                a[p][p] -= g.t * apq;
                a[q][q] += g.t * apq;
                a[p][q] = 0.0;
#pragma unroll
                for (int i = 0; i < S; i++) {
                    const double u = v[i][p], w = v[i][q];
                    v[i][p] = u * g.c - w * g.s;
                    v[i][q] = u * g.s + w * g.c;
                }
            }
        sweeps++;
    }
    double* U = eigen + (size_t)(2 * S * S + nLambda) * slots[model];
    double* Ui = U + S * S;
    double* lam = Ui + S * S;
#pragma unroll
    for (int j = 0; j < S; j++) {
        int rank = 0;
#pragma unroll
        for (int i = 0; i < S; i++) rank += (a[i][i] < a[j][j] || (a[i][i] == a[j][j] && i < j)) ? 1 : 0;
        lam[rank] = capped ? NAN : a[j][j] / norm;
        if (nLambda > S) lam[S + rank] = 0.0;
#pragma unroll
        for (int i = 0; i < S; i++) {
            U[i * S + rank] = v[i][j] / sq[i];
            Ui[rank * S + i] = v[i][j] * sq[i];
        }
    }
    sweepsOut[model] = capped ? -sweeps : sweeps;
}

// ---- 9 <= S <= 64: a workgroup per model --------------------------------------------------------------------------------------
constexpr int EIGEN_BLOCK = 256;
// Per thread and round at most EIGEN_TB blocks of the upper block triangle and EIGEN_TV (row of V, column pair) items, compile-time
// sizes of the register arrays that hold them: up to 22 players 66 blocks and 242 items (one of each a thread), up to 44 players 253
// and 968 (1 and 4), up to 64 players 528 and 2 048 (3 and 8).  The smaller sizes keep the registers, and with them the workgroups a CU
// holds, where a model's LDS image would allow many.
constexpr int eigenBlocksPerThread(int maxPlayers) { return ((maxPlayers / 2) * (maxPlayers / 2 + 1) / 2 + EIGEN_BLOCK - 1) / EIGEN_BLOCK; }
constexpr int eigenItemsPerThread(int maxPlayers) { return (maxPlayers * (maxPlayers / 2) + EIGEN_BLOCK - 1) / EIGEN_BLOCK; }
static_assert(eigenBlocksPerThread(22) == 1 && eigenItemsPerThread(22) == 1 && eigenBlocksPerThread(44) == 1 && eigenItemsPerThread(44) == 4 &&
              eigenBlocksPerThread(64) == 3 && eigenItemsPerThread(64) == 8, "items a thread holds");

// pair k of round r among n1 + 1 players, p < q (0 <= r < n1, 0 <= k <= n1 / 2)
__device__ __forceinline__ void eigenPair(int r, int k, int n1, int& p, int& q) {
    int x = r + k; if (x >= n1) x -= n1;
    int y = r - k; if (y < 0) y += n1;
    if (k == 0) y = n1;
    p = x < y ? x : y; q = x < y ? y : x;
}

// the sum of every thread's x, the same bits in every thread: partial sums in thread order, then a fixed tree
__device__ __forceinline__ double eigenBlockSum(double x, double* red) {
    __syncthreads();                                               // (red may still be read from the previous sum)
    red[threadIdx.x] = x;
    __syncthreads();
    for (int h = EIGEN_BLOCK / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
        __syncthreads();
    }
    return red[0];
}

// LDS image, in doubles: A [N][LD] | V [N][LD] | sqrt(pi) [N] | c, s, t [M] each | red [256] | then ints: order [N]
__host__ __device__ inline size_t eigenBlockLds(int S) {
    const size_t N = (size_t)S + (S & 1), M = N / 2, LD = N + 1;
    return (2 * N * LD + N + 3 * M + EIGEN_BLOCK) * sizeof(double) + N * sizeof(int);
}

template <int MAX_PLAYERS>
__global__ __launch_bounds__(EIGEN_BLOCK) void k_eigenBlock(double* __restrict__ eigen, const double* __restrict__ models,
                                                            const int* __restrict__ slots, int* __restrict__ sweepsOut, int S, int nLambda) {
    extern __shared__ double sh[];
    constexpr int EIGEN_TB = eigenBlocksPerThread(MAX_PLAYERS), EIGEN_TV = eigenItemsPerThread(MAX_PLAYERS);
    const int N = S + (S & 1), M = N / 2, LD = N + 1, R = S * (S - 1) / 2, nBlocks = M * (M + 1) / 2;      // N <= MAX_PLAYERS
    double* A = sh;
    double* V = A + (size_t)N * LD;
    double* sq = V + (size_t)N * LD;
    double* rc = sq + N;
    double* rs = rc + M;
    double* rt = rs + M;
    double* red = rt + M;
    int* order = (int*)(red + EIGEN_BLOCK);
    const int tid = threadIdx.x, model = blockIdx.x;
    const double* rates = models + (size_t)model * (R + S);
    const double* pi = rates + R;

    for (int i = tid; i < N; i += EIGEN_BLOCK) sq[i] = i < S ? sqrt(pi[i]) : 1.0;
    // what this thread updates in every round, in registers: blocks (row pair k, column pair l), k <= l, of the upper block triangle
    // numbered row by row, and (row of V, column pair) items; the pairs of a round are arithmetic in (round, pair), so the addresses
    // of an update wait for no load
    int bk[EIGEN_TB], bl[EIGEN_TB], vi[EIGEN_TV], vl[EIGEN_TV];
#pragma unroll
    for (int j = 0; j < EIGEN_TB; j++) {
        int k = 0, rest = tid + j * EIGEN_BLOCK;
        const bool mine = rest < nBlocks;
        while (mine && rest >= M - k) { rest -= M - k; k++; }
        bk[j] = mine ? k : -1; bl[j] = mine ? k + rest : -1;
    }
#pragma unroll
    for (int j = 0; j < EIGEN_TV; j++) {
        const int e = tid + j * EIGEN_BLOCK;
        vi[j] = e < S * M ? e / M : 0; vl[j] = e < S * M ? e - (e / M) * M : -1;
    }
    __syncthreads();
    for (int e = tid; e < N * N; e += EIGEN_BLOCK) {
        const int i = e / N, j = e - i * N;
        double x = 0.0;
        if (i != j && i < S && j < S) {
            const int lo = i < j ? i : j, hi = i < j ? j : i;
            x = (sq[lo] * rates[lo * S - lo * (lo + 1) / 2 + (hi - lo - 1)]) * sq[hi];
        }
        A[i * LD + j] = x;
        V[i * LD + j] = i == j ? 1.0 : 0.0;
    }
    __syncthreads();
    for (int i = tid; i < S; i += EIGEN_BLOCK) {                   // Q_ii = -sum_j r_ij pi_j, j ascending
        double d = 0.0;
        for (int j = 0; j < S; j++) {
            if (j == i) continue;
            const int lo = i < j ? i : j, hi = i < j ? j : i;
            d -= rates[lo * S - lo * (lo + 1) / 2 + (hi - lo - 1)] * pi[j];
        }
        A[i * LD + i] = d;
    }
    __syncthreads();
    double norm = 0.0;                                             // (every thread forms it the same way: S loads, no hand-over)
    for (int i = 0; i < S; i++) norm -= pi[i] * A[i * LD + i];
    double part = 0.0;
    for (int e = tid; e < N * N; e += EIGEN_BLOCK) { const int i = e / N, j = e - i * N; const double x = A[i * LD + j]; part += x * x; }
    const double norm2 = eigenBlockSum(part, red);

    int sweeps = 0;
    bool capped = false;
    for (;;) {
        part = 0.0;
        for (int e = tid; e < N * N; e += EIGEN_BLOCK) {
            const int i = e / N, j = e - i * N;
            if (i < j) { const double x = A[i * LD + j]; part += x * x; }
        }
        const double off2 = 2.0 * eigenBlockSum(part, red);
        if (off2 <= EIGEN_EPS * EIGEN_EPS * norm2) break;
        if (sweeps == EIGEN_SWEEP_CAP || !(norm2 < INFINITY)) { capped = true; break; }
        for (int r = 0; r < N - 1; r++) {
            if (tid < M) {
                int p, q;
                eigenPair(r, tid, N - 1, p, q);
                // (the idle player's row and column are zeros: its pair is not rotated)
                const EigenAngle g = eigenAngle(A[p * LD + p], A[q * LD + q], A[p * LD + q]);
                rc[tid] = g.c; rs[tid] = g.s; rt[tid] = g.t;
            }
            __syncthreads();
            // every operand of the thread's items first (an item without work reads item 0's), then the arithmetic and the stores:
            // the items of a round touch disjoint entries, and the loads of one do not wait for another's
            int bp[EIGEN_TB][4];
            double be[EIGEN_TB][4], bc[EIGEN_TB][2], bs[EIGEN_TB][2], bt[EIGEN_TB];
#pragma unroll
            for (int j = 0; j < EIGEN_TB; j++) {
                const int k = bk[j] < 0 ? 0 : bk[j], l = bk[j] < 0 ? 0 : bl[j];
                eigenPair(r, k, N - 1, bp[j][0], bp[j][1]);
                eigenPair(r, l, N - 1, bp[j][2], bp[j][3]);
                bc[j][0] = rc[k]; bs[j][0] = rs[k]; bc[j][1] = rc[l]; bs[j][1] = rs[l]; bt[j] = rt[k];
                be[j][0] = A[bp[j][0] * LD + bp[j][2]]; be[j][1] = A[bp[j][0] * LD + bp[j][3]];
                be[j][2] = A[bp[j][1] * LD + bp[j][2]]; be[j][3] = A[bp[j][1] * LD + bp[j][3]];
            }
            int vp[EIGEN_TV][2];
            double ve[EIGEN_TV][2], vc[EIGEN_TV], vs[EIGEN_TV];
#pragma unroll
            for (int j = 0; j < EIGEN_TV; j++) {
                const int l = vl[j] < 0 ? 0 : vl[j], i = vl[j] < 0 ? 0 : vi[j];
                eigenPair(r, l, N - 1, vp[j][0], vp[j][1]);
                vc[j] = rc[l]; vs[j] = rs[l];
                ve[j][0] = V[i * LD + vp[j][0]]; ve[j][1] = V[i * LD + vp[j][1]];
            }
#pragma unroll
            for (int j = 0; j < EIGEN_TB; j++) {
                const double ck = bc[j][0], sk = bs[j][0], cl = bc[j][1], sl = bs[j][1];
                if (bk[j] < 0 || (sk == 0.0 && sl == 0.0 && ck == 1.0 && cl == 1.0)) continue;
                const int p = bp[j][0], q = bp[j][1], P = bp[j][2], Q = bp[j][3];
                if (bk[j] == bl[j]) {                               // (P = p, Q = q: the entries are a_pp, a_pq, a_qp, a_qq)
                    const double apq = be[j][1];
                    A[p * LD + p] = be[j][0] - bt[j] * apq;
                    A[q * LD + q] = be[j][3] + bt[j] * apq;
                    A[p * LD + q] = 0.0; A[q * LD + p] = 0.0;
                    continue;
                }
                const double b00 = be[j][0], b01 = be[j][1], b10 = be[j][2], b11 = be[j][3];
                const double r00 = ck * b00 - sk * b10, r10 = sk * b00 + ck * b10;
                const double r01 = ck * b01 - sk * b11, r11 = sk * b01 + ck * b11;
                const double n00 = r00 * cl - r01 * sl, n01 = r00 * sl + r01 * cl;
                const double n10 = r10 * cl - r11 * sl, n11 = r10 * sl + r11 * cl;
                A[p * LD + P] = n00; A[P * LD + p] = n00;
                A[p * LD + Q] = n01; A[Q * LD + p] = n01;
                A[q * LD + P] = n10; A[P * LD + q] = n10;
                A[q * LD + Q] = n11; A[Q * LD + q] = n11;
            }
#pragma unroll
            for (int j = 0; j < EIGEN_TV; j++) {
                if (vl[j] < 0 || (vs[j] == 0.0 && vc[j] == 1.0)) continue;
                const int i = vi[j];
                V[i * LD + vp[j][0]] = ve[j][0] * vc[j] - ve[j][1] * vs[j];
                V[i * LD + vp[j][1]] = ve[j][0] * vs[j] + ve[j][1] * vc[j];
            }
            __syncthreads();
        }
        sweeps++;
    }

    // rank the eigenvalues (ascending, ties by index): order[rank] = column of V
    for (int j = tid; j < S; j += EIGEN_BLOCK) order[j] = j;      // (eigenvalues that do not compare leave no entry unset)
    __syncthreads();
    for (int j = tid; j < S; j += EIGEN_BLOCK) {
        const double mine = A[j * LD + j];
        int rank = 0;
        for (int i = 0; i < S; i++) { const double x = A[i * LD + i]; rank += (x < mine || (x == mine && i < j)) ? 1 : 0; }
        order[rank] = j;
    }
    __syncthreads();
    double* U = eigen + (size_t)(2 * S * S + nLambda) * slots[model];
    double* Ui = U + (size_t)S * S;
    double* lam = Ui + (size_t)S * S;
    for (int e = tid; e < S * S; e += EIGEN_BLOCK) {
        const int i = e / S, j = e - i * S;
        U[e] = V[i * LD + order[j]] / sq[i];                       // U[i][rank]
        Ui[e] = V[j * LD + order[i]] * sq[j];                      // U^-1[rank][j]
    }
    for (int j = tid; j < S; j += EIGEN_BLOCK) {
        lam[j] = capped ? NAN : A[order[j] * LD + order[j]] / norm;
        if (nLambda > S) lam[S + j] = 0.0;
    }
    if (tid == 0) sweepsOut[model] = capped ? -sweeps : sweeps;
}

bool launchEigenReversible(hipStream_t stream, double* eigen, const double* models, const int* slots, int* sweeps, int count, int S,
                           bool complexEigen) {
    if (count <= 0) return true;
    const int nLambda = complexEigen ? 2 * S : S;
    if (S <= 8) {
        const dim3 grid((unsigned)((count + 63) / 64)), block(64);
#define EIGEN_SMALL(N) case N: hipLaunchKernelGGL((k_eigenSmall<N>), grid, block, 0, stream, eigen, models, slots, sweeps, count, nLambda); break;
        switch (S) {
            EIGEN_SMALL(2) EIGEN_SMALL(3) EIGEN_SMALL(4) EIGEN_SMALL(5) EIGEN_SMALL(6) EIGEN_SMALL(7) EIGEN_SMALL(8)
            default: return false;
        }
#undef EIGEN_SMALL
        return true;
    }
    const size_t lds = eigenBlockLds(S);
    const dim3 grid((unsigned)count), block(EIGEN_BLOCK);
    if (S <= 22) hipLaunchKernelGGL(k_eigenBlock<22>, grid, block, lds, stream, eigen, models, slots, sweeps, S, nLambda);
    else if (S <= 44) hipLaunchKernelGGL(k_eigenBlock<44>, grid, block, lds, stream, eigen, models, slots, sweeps, S, nLambda);
    else {
        if (!grantDynamicLds(reinterpret_cast<const void*>(k_eigenBlock<64>), lds)) return false;      // (over 64 KiB from 61 states on)
        hipLaunchKernelGGL(k_eigenBlock<64>, grid, block, lds, stream, eigen, models, slots, sweeps, S, nLambda);
    }
    return true;
}

}  // namespace mi355
