// kernels_nodeheight.hip — first derivatives and diagonal second derivatives of the log-likelihood in the heights of the internal
// nodes (beagleMi355NodeHeightDerivatives; kernels.h NodeHeightJob has the formula).
//
// What the reference does for it (src/dr/evomodel/treedatalikelihood/discrete/DiscreteTraitNodeHeightDelegate.java:63-200): read
// back every post-order and every pre-order partial and every branch matrix, then loop over nodes, patterns, categories and state
// pairs on the host.  Its per-branch terms pre(j) . Q post(j) / pre(j) . post(j) are, with pre(j) = P_j^T (pre(i) * P_k post(k)),
// sums over the states of node i of products of three vectors — P_j post(j) and its images under Q_j, the same for k, and pre(i)
// and its images under Q_i^T — so a NODE is the unit of work: pre(i), post(j), post(k) read once, no pre-order partial of a tip
// needed, nothing written but two block sums.  The ratios are free of scale factors: scaled partials are read as they are.
//
// 4 states (k_nodeHeight4, the hot path) has the shape of k_preNode4 (kernels_preorder4.hip): a pattern per lane, the categories
// walked in registers, partials as 32-byte vectors, compact tips as states, the five matrices of a job at wave-uniform addresses.
// Every other state count (k_nodeHeight) is a plain kernel on either layout: a thread keeps its pattern's three partials in its
// own LDS columns and applies product matrices a small kernel forms first (Q P, Q Q P, Q_i Q_i), so that no intermediate vector
// has to be kept.  Sums over patterns: a fixed-shape butterfly per 64 patterns, then launchEdgeFinal — the same bits every run.
#include "kernels.h"

namespace mi355 {

typedef double v4d __attribute__((ext_vector_type(4)));

__device__ __forceinline__ v4d nhMatvec4(const double* __restrict__ M, const v4d x) {          // y_i = sum_k M[i][k] x_k
    v4d y;
    y.x = M[0] * x.x + M[1] * x.y + M[2] * x.z + M[3] * x.w;
    y.y = M[4] * x.x + M[5] * x.y + M[6] * x.z + M[7] * x.w;
    y.z = M[8] * x.x + M[9] * x.y + M[10] * x.z + M[11] * x.w;
    y.w = M[12] * x.x + M[13] * x.y + M[14] * x.z + M[15] * x.w;
    return y;
}
__device__ __forceinline__ v4d nhMatvecT4(const double* __restrict__ M, const v4d x) {         // y_j = sum_i M[i][j] x_i
    v4d y;
    y.x = M[0] * x.x + M[4] * x.y + M[8] * x.z + M[12] * x.w;
    y.y = M[1] * x.x + M[5] * x.y + M[9] * x.z + M[13] * x.w;
    y.z = M[2] * x.x + M[6] * x.y + M[10] * x.z + M[14] * x.w;
    y.w = M[3] * x.x + M[7] * x.y + M[11] * x.z + M[15] * x.w;
    return y;
}
__device__ __forceinline__ v4d nhTipVector(int s) {
    return s >= 4 ? v4d{1.0, 1.0, 1.0, 1.0} : v4d{s == 0 ? 1.0 : 0.0, s == 1 ? 1.0 : 0.0, s == 2 ? 1.0 : 0.0, s == 3 ? 1.0 : 0.0};
}
__device__ __forceinline__ double nhDot4(const v4d a, const v4d b) { return a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w; }

// the ten sums of a pattern -> its two derivatives
struct NodeHeightSums { double D, Bj, Bk, Ui, Cj, Ck, Bjk, Vi, Bju, Bku; };
template <bool SECOND>
__device__ __forceinline__ void nodeHeightPattern(const NodeHeightSums& t, const NodeHeightJob& jb, bool inner, double& first, double& second) {
    const double rj = jb.rJ, rk = jb.rK, ri = inner ? jb.rI : 0.0;
    const double gj = t.Bj / t.D, gk = t.Bk / t.D, gi = inner ? t.Ui / t.D : 0.0;
    first = rj * gj + rk * gk - ri * gi;
    second = 0.0;
    if (SECOND) {
        const double hjj = t.Cj / t.D - gj * gj, hkk = t.Ck / t.D - gk * gk, hjk = t.Bjk / t.D - gj * gk;
        second = rj * rj * hjj + rk * rk * hkk + 2.0 * rj * rk * hjk;
        if (inner) {
            const double hii = t.Vi / t.D - gi * gi, hij = t.Bju / t.D - gi * gj, hik = t.Bku / t.D - gi * gk;
            second += ri * ri * hii - 2.0 * ri * rj * hij - 2.0 * ri * rk * hik;
        }
    }
}
// blockSums[(slot * nBlocks + block64) * 2] = the wave's two sums (fixed-shape butterfly: deterministic; the layout k_edgeFinal sums)
__device__ __forceinline__ void nodeHeightBlockSum(double w1, double w2, double* __restrict__ blockSums, int slot, int nBlocks, int block64) {
    for (int off = 32; off > 0; off >>= 1) { w1 += __shfl_xor(w1, off, 64); w2 += __shfl_xor(w2, off, 64); }
    if ((threadIdx.x & 63) == 0) {
        double* b = blockSums + ((size_t)slot * nBlocks + block64) * 2;
        b[0] = w1; b[1] = w2;
    }
}

template <bool SECOND>
__global__ __launch_bounds__(256) void k_nodeHeight4(const NodeHeightJob* __restrict__ jobs, const double* __restrict__ matrices,
                                                     const double* __restrict__ catWeights, const double* __restrict__ patternWeights,
                                                     double* __restrict__ blockSums, int P, int C, int nBlocks) {
    const NodeHeightJob& jb = jobs[blockIdx.y];
    const int p = blockIdx.x * 256 + threadIdx.x;
    const bool valid = p < P;
    const int q = valid ? p : P - 1;                               // lanes past the end recompute the last pattern and count for nothing
    const bool stJ = jb.statesJ != 0, stK = jb.statesK != 0, inner = jb.dI >= 0;
    int sj = 4, sk = 4;
    if (stJ) sj = gptr(reinterpret_cast<const uint8_t*>(jb.postJ))[q];
    if (stK) sk = gptr(reinterpret_cast<const uint8_t*>(jb.postK))[q];
    const v4d MI355_GLOBAL* pre = gptr(reinterpret_cast<const v4d*>(jb.pre));
    const v4d MI355_GLOBAL* postJ = gptr(reinterpret_cast<const v4d*>(jb.postJ));
    const v4d MI355_GLOBAL* postK = gptr(reinterpret_cast<const v4d*>(jb.postK));
    const int dI = inner ? jb.dI : jb.dJ;                          // (the root: any matrix that exists; its products are not used)
    NodeHeightSums t = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int c = 0; c < C; c++) {
        const size_t e = (size_t)c * P + q;
        const double* PJ = matrices + ((size_t)jb.matJ * C + c) * 16;
        const double* QJ = matrices + ((size_t)jb.dJ * C + c) * 16;
        const double* PK = matrices + ((size_t)jb.matK * C + c) * 16;
        const double* QK = matrices + ((size_t)jb.dK * C + c) * 16;
        const double* QI = matrices + ((size_t)dI * C + c) * 16;
        const v4d qv = pre[e] * catWeights[c];
        const v4d xj = stJ ? nhTipVector(sj) : postJ[e];
        const v4d xk = stK ? nhTipVector(sk) : postK[e];
        const v4d aj = nhMatvec4(PJ, xj), ak = nhMatvec4(PK, xk);
        const v4d bj = nhMatvec4(QJ, aj), bk = nhMatvec4(QK, ak);
        const v4d aa = aj * ak, ba = bj * ak, ab = aj * bk;
        t.D += nhDot4(aa, qv); t.Bj += nhDot4(ba, qv); t.Bk += nhDot4(ab, qv);
        if (SECOND) {
            const v4d cj = nhMatvec4(QJ, bj), ck = nhMatvec4(QK, bk);
            t.Cj += nhDot4(cj * ak, qv); t.Ck += nhDot4(aj * ck, qv); t.Bjk += nhDot4(bj * bk, qv);
        }
        if (inner) {
            const v4d u = nhMatvecT4(QI, qv);
            t.Ui += nhDot4(aa, u);
            if (SECOND) {
                const v4d v = nhMatvecT4(QI, u);
                t.Vi += nhDot4(aa, v); t.Bju += nhDot4(ba, u); t.Bku += nhDot4(ab, u);
            }
        }
    }
    double first, second;
    nodeHeightPattern<SECOND>(t, jb, inner, first, second);
    const double pw = valid ? patternWeights[p] : 0.0;
    const int block64 = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (block64 < nBlocks) nodeHeightBlockSum(valid ? pw * first : 0.0, valid ? pw * second : 0.0, blockSums, jb.slot, nBlocks, block64);
}

void launchNodeHeight4(hipStream_t stream, const NodeHeightJob* dJobs, int nJobs, const double* matrices, const double* catWeights,
                       const double* patternWeights, double* blockSums, int P, int C, bool second) {
    if (nJobs <= 0 || P <= 0) return;
    for (int o = 0; o < nJobs; o += 65535) {
        const int n = nJobs - o < 65535 ? nJobs - o : 65535;
        const dim3 grid((P + 255) / 256, n), block(256);
        if (second) hipLaunchKernelGGL(k_nodeHeight4<true>, grid, block, 0, stream, dJobs + o, matrices, catWeights, patternWeights, blockSums, P, C, edgeBlocks(P));
        else hipLaunchKernelGGL(k_nodeHeight4<false>, grid, block, 0, stream, dJobs + o, matrices, catWeights, patternWeights, blockSums, P, C, edgeBlocks(P));
    }
}

// ---- 2..64 states ---------------------------------------------------------------------------------------------------------
constexpr int NH_BLOCK = 64;                 // = the patterns per entry of blockSums (edgeBlocks)
constexpr int NH_PRODUCTS = 5;               // per job: Q_j P_j | Q_j Q_j P_j | Q_k P_k | Q_k Q_k P_k | Q_i Q_i, [C][S][S] each

size_t nodeHeightProductDoubles(int nJobs, int S, int C) { return (size_t)nJobs * NH_PRODUCTS * C * S * S; }

// stage 0: products 0, 2, 4 = Q_j P_j, Q_k P_k, Q_i Q_i;  stage 1: products 1, 3 = Q_j (Q_j P_j), Q_k (Q_k P_k)
__global__ __launch_bounds__(256) void k_nodeHeightProducts(const NodeHeightJob* __restrict__ jobs, const double* __restrict__ matrices,
                                                            double* __restrict__ products, int S, int C, int stage) {
    const int t = (int)blockIdx.x * 256 + (int)threadIdx.x, SS = S * S;
    if (t >= C * SS) return;
    const NodeHeightJob& jb = jobs[blockIdx.y];
    const int which = (int)blockIdx.z;                             // stage 0: j, k, i; stage 1: j, k
    const int c = t / SS, r = (t % SS) / S, col = t % S;
    double* base = products + (size_t)blockIdx.y * NH_PRODUCTS * C * SS;
    const int left = which == 0 ? jb.dJ : which == 1 ? jb.dK : jb.dI;
    if (left < 0) return;                                          // (the root has no Q_i)
    const double* L = matrices + ((size_t)left * C + c) * SS;
    const double* R;
    double* out;
    if (stage == 0) {
        const int right = which == 0 ? jb.matJ : which == 1 ? jb.matK : jb.dI;
        R = matrices + ((size_t)right * C + c) * SS;
        out = base + ((size_t)(which * 2) * C + c) * SS;
    } else {
        R = base + ((size_t)(which * 2) * C + c) * SS;
        out = base + ((size_t)(which * 2 + 1) * C + c) * SS;
    }
    double v = 0.0;
    for (int k = 0; k < S; k++) v += L[r * S + k] * R[k * S + col];
    out[r * S + col] = v;
}

template <bool TILED>
__device__ __forceinline__ size_t nhIndex(int c, int p, int i, int P, int S, int ntile) {
    return TILED ? (((size_t)c * ntile + (p >> 5)) * S + i) * 32 + (p & 31) : ((size_t)c * P + p) * S + i;
}

template <bool TILED, bool SECOND>
__global__ __launch_bounds__(NH_BLOCK) void k_nodeHeight(const NodeHeightJob* __restrict__ jobs, const double* __restrict__ matrices,
                                                         const double* __restrict__ products, const double* __restrict__ catWeights,
                                                         const double* __restrict__ patternWeights, double* __restrict__ blockSums,
                                                         int P, int S, int C) {
    extern __shared__ double nhLds[];              // xj[S][64] | xk[S][64] | q[S][64]: a thread reads and writes its own column only
    const int tid = threadIdx.x, p = blockIdx.x * NH_BLOCK + tid, ntile = (P + 31) >> 5, SS = S * S;
    double* xj = nhLds + tid; double* xk = xj + S * NH_BLOCK; double* qv = xk + S * NH_BLOCK;
    const NodeHeightJob& jb = jobs[blockIdx.y];
    const bool valid = p < P, stJ = jb.statesJ != 0, stK = jb.statesK != 0, inner = jb.dI >= 0;
    double first = 0.0, second = 0.0;
    if (valid) {
        const double MI355_GLOBAL* pre = gptr(jb.pre);
        const double MI355_GLOBAL* postJ = gptr(reinterpret_cast<const double*>(jb.postJ));
        const double MI355_GLOBAL* postK = gptr(reinterpret_cast<const double*>(jb.postK));
        int sj = S, sk = S;
        if (stJ) sj = gptr(reinterpret_cast<const uint8_t*>(jb.postJ))[p];
        if (stK) sk = gptr(reinterpret_cast<const uint8_t*>(jb.postK))[p];
        const double* prod = products + (size_t)blockIdx.y * NH_PRODUCTS * C * SS;
        NodeHeightSums t = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (int c = 0; c < C; c++) {
            const double w = catWeights[c];
            for (int i = 0; i < S; i++) {
                xj[i * NH_BLOCK] = stJ ? ((sj >= S || sj == i) ? 1.0 : 0.0) : postJ[nhIndex<TILED>(c, p, i, P, S, ntile)];
                xk[i * NH_BLOCK] = stK ? ((sk >= S || sk == i) ? 1.0 : 0.0) : postK[nhIndex<TILED>(c, p, i, P, S, ntile)];
                qv[i * NH_BLOCK] = pre[nhIndex<TILED>(c, p, i, P, S, ntile)] * w;
            }
            const double* PJ = matrices + ((size_t)jb.matJ * C + c) * SS;
            const double* PK = matrices + ((size_t)jb.matK * C + c) * SS;
            const double* QPJ = prod + ((size_t)0 * C + c) * SS;
            const double* QQPJ = prod + ((size_t)1 * C + c) * SS;
            const double* QPK = prod + ((size_t)2 * C + c) * SS;
            const double* QQPK = prod + ((size_t)3 * C + c) * SS;
            const double* QI = inner ? matrices + ((size_t)jb.dI * C + c) * SS : PJ;
            const double* QQI = inner ? prod + ((size_t)4 * C + c) * SS : PJ;
            for (int s = 0; s < S; s++) {
                double aj = 0.0, bj = 0.0, cj = 0.0, ak = 0.0, bk = 0.0, ck = 0.0, u = 0.0, v = 0.0;
                for (int k = 0; k < S; k++) {
                    const double a = xj[k * NH_BLOCK], b = xk[k * NH_BLOCK];
                    aj += PJ[s * S + k] * a; bj += QPJ[s * S + k] * a;
                    ak += PK[s * S + k] * b; bk += QPK[s * S + k] * b;
                    if (SECOND) { cj += QQPJ[s * S + k] * a; ck += QQPK[s * S + k] * b; }
                }
                if (inner)
                    for (int k = 0; k < S; k++) {
                        const double qk = qv[k * NH_BLOCK];
                        u += QI[k * S + s] * qk;
                        if (SECOND) v += QQI[k * S + s] * qk;
                    }
                const double qs = qv[s * NH_BLOCK], aa = aj * ak, ba = bj * ak, ab = aj * bk;
                t.D += aa * qs; t.Bj += ba * qs; t.Bk += ab * qs; t.Ui += aa * u;
                if (SECOND) { t.Cj += cj * ak * qs; t.Ck += aj * ck * qs; t.Bjk += bj * bk * qs; t.Vi += aa * v; t.Bju += ba * u; t.Bku += ab * u; }
            }
        }
        nodeHeightPattern<SECOND>(t, jb, inner, first, second);
        const double pw = patternWeights[p];
        first *= pw; second *= pw;
    }
    nodeHeightBlockSum(first, second, blockSums, jb.slot, (int)gridDim.x, (int)blockIdx.x);
}

bool launchNodeHeight(hipStream_t stream, const NodeHeightJob* dJobs, int nJobs, const double* matrices, double* products,
                      const double* catWeights, const double* patternWeights, double* blockSums, int P, int S, int C, bool tiled, bool second) {
    if (nJobs <= 0 || P <= 0) return true;
    const size_t lds = (size_t)3 * S * NH_BLOCK * sizeof(double);
    if (lds > 160 * 1024) return false;
    if (!grantDynamicLds(reinterpret_cast<const void*>(k_nodeHeight<false, false>), 160 * 1024) ||
        !grantDynamicLds(reinterpret_cast<const void*>(k_nodeHeight<false, true>), 160 * 1024) ||
        !grantDynamicLds(reinterpret_cast<const void*>(k_nodeHeight<true, false>), 160 * 1024) ||
        !grantDynamicLds(reinterpret_cast<const void*>(k_nodeHeight<true, true>), 160 * 1024)) return false;
    const int entryBlocks = (C * S * S + 255) / 256;
    for (int o = 0; o < nJobs; o += 65535) {
        const int n = nJobs - o < 65535 ? nJobs - o : 65535;
        double* prod = products + nodeHeightProductDoubles(o, S, C);
        hipLaunchKernelGGL(k_nodeHeightProducts, dim3(entryBlocks, n, 3), dim3(256), 0, stream, dJobs + o, matrices, prod, S, C, 0);
        if (second) hipLaunchKernelGGL(k_nodeHeightProducts, dim3(entryBlocks, n, 2), dim3(256), 0, stream, dJobs + o, matrices, prod, S, C, 1);
        const dim3 grid(edgeBlocks(P), n), block(NH_BLOCK);
#define NH_LAUNCH(T, W) hipLaunchKernelGGL((k_nodeHeight<T, W>), grid, block, lds, stream, dJobs + o, matrices, prod, catWeights, patternWeights, blockSums, P, S, C)
        if (tiled) { if (second) NH_LAUNCH(true, true); else NH_LAUNCH(true, false); }
        else { if (second) NH_LAUNCH(false, true); else NH_LAUNCH(false, false); }
#undef NH_LAUNCH
    }
    return true;
}

}  // namespace mi355
