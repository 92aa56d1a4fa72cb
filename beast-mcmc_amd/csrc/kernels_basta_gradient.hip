// kernels_basta_gradient.hip — the gradient of the BASTA log-density with respect to the migration rates and the population sizes, in
// reverse mode (beagleBastaGradient; the rule is stated in include/beagle_mi355.h).
//
// What it restates: the numbers GenericBastaLikelihoodDelegate.peelPartialsGrad / peelPopSizeSGrad / reduceWithinIntervalGrad /
// reduceAcrossIntervalsGrad(PopSize) (src/dr/evomodel/coalescent/basta/GenericBastaLikelihoodDelegate.java:443-753) compute on zeroed
// storage.  The reference carries S^2 tangent vectors per buffer forwards; here one adjoint vector per buffer is carried backwards,
// which costs what a likelihood costs.
//
// The adjoint of a vector needs the adjoint of the one vector computed from it, so the work fans out from the roots exactly as the
// lineage-deme sampler's does (kernels_basta_states.hip): the same chains, one launch per level of coalescences, a wave per chain,
// lane = state.  A step is a TRANSPOSED matrix-vector product, out_j = sum_i M[i][j] lambda_i: lane j reads column j, so for every i
// the wave reads one contiguous row.  A chain is a sequence of dependent small products, so a step costs what its memory latencies
// cost:
//   k_bastaGradientSweepAhead<REGS>  up to 64 states: the NEXT step's matrix (REGS entries a lane) and the next step's entries of the
//                                    vectors are asked for before the current product and go into LDS after it; the product reads
//                                    rows from LDS (consecutive lanes, consecutive words: no padding)
//   k_bastaGradientSweep             above 64 states (up to four a lane): rows straight from memory, sixteen asked for before the
//                                    first is used
//
// The two reductions (W and G_theta) take the adjoints and vectors as they stand: a workgroup per list interval sums its operations
// in list order, then one thread per entry adds the intervals in index order.  No atomics, so the bits do not depend on the schedule.
//
// Sums run in index order and nothing is contracted into an FMA: every value is the host restatement's bit for bit
// (tests/basta_gradient_reference.py adjoint).
#pragma clang fp contract(off)

#include "kernels.h"

namespace mi355 {

namespace {

constexpr int GRADIENT_ROWS = BASTA_GRADIENT_MAX_STATES / 64;      // states per lane of the kernel that reads from memory
constexpr int GRADIENT_AHEAD_STATES = 64;                          // up to here k_bastaGradientSweepAhead

// what a wave knows of its chain
struct GradientChain { int nSteps, top, flags; int4 aux; const int4* steps; const int* numbers; };

__device__ __forceinline__ GradientChain bastaGradientChain(const BastaGradientArgs& a, int first) {
    const int4 chain = a.chains[first + (int)blockIdx.x];
    GradientChain c;
    c.aux = a.chainAux[first + (int)blockIdx.x];
    c.nSteps = __builtin_amdgcn_readfirstlane(chain.y);
    c.top = __builtin_amdgcn_readfirstlane(chain.z);
    c.flags = chain.w;
    c.steps = a.steps + __builtin_amdgcn_readfirstlane(chain.x);
    c.numbers = a.stepNumbers + __builtin_amdgcn_readfirstlane(chain.x);
    return c;
}

// The adjoint of the end vector at the top of the chain — an input of a coalescence as it arrived there, or a root that is no
// coalescence — stored, and left in lam for the first product.  theta and coef (c of the first step's interval) are filled.
template <int ROWS>
__device__ __forceinline__ void bastaGradientTop(const BastaGradientArgs& a, const GradientChain& ch, const int4& cur, int number,
                                                 double (&theta)[ROWS], double (&coef)[ROWS], double* lam, double* vec) {
    const int S = a.S, lane = threadIdx.x, top = ch.top;
    const double half = -a.lengths[cur.w] * 0.5;
#pragma unroll
    for (int r = 0; r < ROWS; r++) {
        const int j = lane + 64 * r;
        theta[r] = j < S ? 1.0 / a.sizes[j] : 0.0;
        coef[r] = half * theta[r];
    }
    if (cur.z >= 0) {
        const bool root = (ch.flags & BASTA_CHAIN_ROOT) != 0;
        double own[ROWS];
#pragma unroll
        for (int r = 0; r < ROWS; r++) {
            const int j = lane + 64 * r;
            own[r] = 0.0;
            if (j < S) {
                if (!root) own[r] = a.adjoints[(size_t)top * S + j];
                lam[j] = own[r];
                vec[j] = a.partials[(size_t)top * S + j];
            }
        }
        __syncthreads();
        double dot = 0.0;
        for (int i = 0; i < S; i++) dot += lam[i] * vec[i];
        const double J = a.coalescent[ch.aux.y];
        __syncthreads();
#pragma unroll
        for (int r = 0; r < ROWS; r++) {
            const int j = lane + 64 * r;
            if (j < S) {
                const double w = ((own[r] - dot) + 1.0) / J;
                const double other = a.partials[(size_t)ch.aux.x * S + j], end = a.partials[(size_t)cur.z * S + j];
                const double l = (w * other) * theta[r] + coef[r] * (a.g[(size_t)number * S + j] - end);
                a.adjoints[(size_t)cur.z * S + j] = l;
                if (ch.aux.z == 0) a.w[(size_t)top * S + j] = w;
                lam[j] = l;
            }
        }
    } else {
#pragma unroll
        for (int r = 0; r < ROWS; r++) {
            const int j = lane + 64 * r;
            if (j < S) {
                const double end = a.partials[(size_t)top * S + j];
                const double l = 0.0 + coef[r] * (a.g[(size_t)number * S + j] - end);
                a.adjoints[(size_t)top * S + j] = l;
                lam[j] = l;
            }
        }
    }
}

// sum_i M[i][j] x_i, i in index order (x: S values at a wave-uniform address)
__device__ __forceinline__ double bastaColumn(const double* __restrict__ M, const double* x, int S, int j) {
    double sum = 0.0;
    for (int i0 = 0; i0 < S; i0 += 16) {
        double r[16];
#pragma unroll
        for (int u = 0; u < 16; u++) r[u] = i0 + u < S ? M[(size_t)(i0 + u) * S + j] : 0.0;
#pragma unroll
        for (int u = 0; u < 16; u++) if (i0 + u < S) sum += r[u] * x[i0 + u];
    }
    return sum;
}

__global__ __launch_bounds__(64) void k_bastaGradientSweep(BastaGradientArgs a, int first) {
    extern __shared__ double lds[];
    const int S = a.S, lane = threadIdx.x;
    double* lam = lds;                 // the adjoint the next product starts from
    double* vec = lds + S;             // a coalescence's dest vector
    const GradientChain ch = bastaGradientChain(a, first);
    int4 cur = ch.steps[0];
    int number = ch.numbers[0];
    double theta[GRADIENT_ROWS], c[GRADIENT_ROWS];
    bastaGradientTop<GRADIENT_ROWS>(a, ch, cur, number, theta, c, lam, vec);
    for (int i = 0; i < ch.nSteps; i++) {
        const bool more = i + 1 < ch.nSteps;
        const int4 next = ch.steps[more ? i + 1 : i];                        // asked for now, used after this step's product
        const int nextNumber = ch.numbers[more ? i + 1 : i];
        __syncthreads();                                                     // (lam is complete)
        const double* M = a.matrices + (size_t)cur.y * S * S;
        // the input was written by a one-input operation of an earlier interval (more): there it is an end vector
        const double halfNext = -a.lengths[next.w] * 0.5;
        double left[GRADIENT_ROWS], start[GRADIENT_ROWS], g[GRADIENT_ROWS];
#pragma unroll
        for (int r = 0; r < GRADIENT_ROWS; r++) {
            const int j = lane + 64 * r;
            left[r] = start[r] = g[r] = 0.0;
            if (j < S) {
                g[r] = a.g[(size_t)nextNumber * S + j];
                start[r] = a.partials[(size_t)cur.x * S + j];
                const double e = a.e[(size_t)number * S + j];
                left[r] = bastaColumn(M, lam, S, j) + c[r] * (e - start[r]);
            }
        }
        __syncthreads();                                                     // (the lanes are done with lam)
#pragma unroll
        for (int r = 0; r < GRADIENT_ROWS; r++) {
            const int j = lane + 64 * r;
            c[r] = halfNext * theta[r];
            if (j < S) {
                const double l = more ? left[r] + c[r] * (g[r] - start[r]) : left[r];
                a.adjoints[(size_t)cur.x * S + j] = l;
                lam[j] = l;
            }
        }
        cur = next; number = nextNumber;
    }
}

// a step's matrix from memory into registers (REGS entries a lane) ...
template <int REGS>
__device__ __forceinline__ void bastaGradientLoad(const double* __restrict__ M, int n, double (&m)[REGS]) {
#pragma unroll
    for (int u = 0; u < REGS; u++) { const int at = (int)threadIdx.x + 64 * u; m[u] = at < n ? M[at] : 0.0; }
}
// ... and from there into LDS, as it lies in memory
template <int REGS>
__device__ __forceinline__ void bastaGradientStore(double* stage, int n, const double (&m)[REGS]) {
#pragma unroll
    for (int u = 0; u < REGS; u++) { const int at = (int)threadIdx.x + 64 * u; if (at < n) stage[at] = m[u]; }
}

template <int REGS>
__global__ __launch_bounds__(64) void k_bastaGradientSweepAhead(BastaGradientArgs a, int first) {
    extern __shared__ double lds[];
    const int S = a.S, n = S * S, lane = threadIdx.x;
    const bool on = lane < S;
    const int j = on ? lane : 0;                                             // (an idle lane reads what lane 0 reads and stores nothing)
    double* lam = lds;
    double* vec = lds + S;
    double* stage = lds + 2 * S;       // the step's matrix
    const GradientChain ch = bastaGradientChain(a, first);
    int4 cur = ch.steps[0];
    int number = ch.numbers[0];
    int4 next = ch.steps[ch.nSteps > 1 ? 1 : 0];
    int nextNumber = ch.numbers[ch.nSteps > 1 ? 1 : 0];
    // the first step's matrix and entries: asked for now, they arrive while the top of the chain is worked out
    double m[REGS];
    bastaGradientLoad<REGS>(a.matrices + (size_t)cur.y * n, n, m);
    double start = a.partials[(size_t)cur.x * S + j], e = a.e[(size_t)number * S + j];
    double g = a.g[(size_t)nextNumber * S + j], halfNext = -a.lengths[next.w] * 0.5;
    double theta[1], c[1];
    bastaGradientTop<1>(a, ch, cur, number, theta, c, lam, vec);
    for (int i = 0; i < ch.nSteps; i++) {
        const bool more = i + 1 < ch.nSteps;
        const int4 after = ch.steps[i + 2 < ch.nSteps ? i + 2 : i];          // the step after the next: its record, asked for now
        const int afterNumber = ch.numbers[i + 2 < ch.nSteps ? i + 2 : i];
        bastaGradientStore<REGS>(stage, n, m);
        __syncthreads();                                                     // (the matrix and lam are complete)
        const double startNow = start, eNow = e, gNow = g, halfNow = halfNext;
        if (more) {                                                          // the next step's data: asked for now, used after this product
            bastaGradientLoad<REGS>(a.matrices + (size_t)next.y * n, n, m);
            start = a.partials[(size_t)next.x * S + j]; e = a.e[(size_t)nextNumber * S + j];
            g = a.g[(size_t)afterNumber * S + j]; halfNext = -a.lengths[after.w] * 0.5;
        }
        double sum = 0.0;
        for (int k = 0; k < S; k++) sum += stage[k * S + j] * lam[k];
        const double left = sum + c[0] * (eNow - startNow);
        __syncthreads();                                                     // (the lanes are done with the matrix and lam)
        // with more steps the input was written by a one-input operation of an earlier interval: there it is an end vector
        c[0] = halfNow * theta[0];
        const double l = more ? left + c[0] * (gNow - startNow) : left;
        if (on) { a.adjoints[(size_t)cur.x * S + j] = l; lam[j] = l; }
        cur = next; number = nextNumber; next = after; nextNumber = afterNumber;
    }
}

// One workgroup per list interval: entry a * S + b of W, then entry a of G_theta, each summed over the interval's operations in list
// order (side 0, then side 1).
__global__ __launch_bounds__(256) void k_bastaGradientIntervals(BastaGradientArgs a) {
    const int S = a.S, k = blockIdx.x, entries = S * S + S;
    const int begin = a.intervals[k], end = a.intervals[k + 1];
    double* part = a.parts + (size_t)k * entries;
    if (begin >= end) {
        for (int idx = threadIdx.x; idx < entries; idx += 256) part[idx] = 0.0;
        return;
    }
    const int number = a.ops[(size_t)begin * 8 + 7];
    const double t = a.distances ? a.distances[k] : 0.0;
    const double quarter = -a.lengths[k] * 0.25;
    for (int idx = threadIdx.x; idx < entries; idx += 256) {
        double sum = 0.0;
        if (idx < S * S) {
            if (a.distances) {
                const int ia = idx / S, ib = idx - ia * S;
                for (int o = begin; o < end; o++) {
                    const int* op = a.ops + (size_t)o * 8;
                    const int acc1 = op[5];
                    sum += (t * a.partials[(size_t)acc1 * S + ia]) * a.adjoints[(size_t)acc1 * S + ib];
                    if (op[3] >= 0) {
                        const int acc2 = op[6];
                        sum += (t * a.partials[(size_t)acc2 * S + ia]) * a.adjoints[(size_t)acc2 * S + ib];
                    }
                }
            }
        } else {
            const int i = idx - S * S;
            const size_t at = (size_t)number * S + i;
            const double e = a.e[at], g = a.g[at];
            sum = quarter * (((e * e - a.f[at]) + g * g) - a.h[at]);
            for (int o = begin; o < end; o++) {
                const int* op = a.ops + (size_t)o * 8;
                if (op[3] >= 0) sum += (a.w[(size_t)op[0] * S + i] * a.partials[(size_t)op[5] * S + i]) * a.partials[(size_t)op[6] * S + i];
            }
        }
        part[idx] = sum;
    }
}

// the intervals' shares in index order, a thread per entry (sixteen asked for before the first is added)
__global__ __launch_bounds__(256) void k_bastaGradientTotal(BastaGradientArgs a, int nIntervals) {
    const int entries = a.S * a.S + a.S;
    const int idx = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (idx >= entries) return;
    double sum = 0.0;
    for (int k0 = 0; k0 < nIntervals; k0 += 16) {
        double r[16];
#pragma unroll
        for (int u = 0; u < 16; u++) r[u] = k0 + u < nIntervals ? a.parts[(size_t)(k0 + u) * entries + idx] : 0.0;
#pragma unroll
        for (int u = 0; u < 16; u++) if (k0 + u < nIntervals) sum += r[u];
    }
    a.out[idx] = sum;
}

}  // namespace

void launchBastaGradientSweep(hipStream_t stream, const BastaGradientArgs& a, int first, int n) {
    if (n <= 0) return;
    const int S = a.S, entries = (S * S + 63) / 64;          // matrix entries a lane
    const size_t vectors = (size_t)2 * S * sizeof(double), staged = vectors + (size_t)S * S * sizeof(double);
    if (S > GRADIENT_AHEAD_STATES) hipLaunchKernelGGL(k_bastaGradientSweep, dim3(n), dim3(64), vectors, stream, a, first);
    else if (entries <= 1) hipLaunchKernelGGL(k_bastaGradientSweepAhead<1>, dim3(n), dim3(64), staged, stream, a, first);
    else if (entries <= 4) hipLaunchKernelGGL(k_bastaGradientSweepAhead<4>, dim3(n), dim3(64), staged, stream, a, first);
    else if (entries <= 16) hipLaunchKernelGGL(k_bastaGradientSweepAhead<16>, dim3(n), dim3(64), staged, stream, a, first);
    else hipLaunchKernelGGL(k_bastaGradientSweepAhead<64>, dim3(n), dim3(64), staged, stream, a, first);
}

void launchBastaGradientReduce(hipStream_t stream, const BastaGradientArgs& a, int nIntervals) {
    const int entries = a.S * a.S + a.S;
    if (nIntervals > 0) hipLaunchKernelGGL(k_bastaGradientIntervals, dim3(nIntervals), dim3(256), 0, stream, a);
    hipLaunchKernelGGL(k_bastaGradientTotal, dim3((entries + 255) / 256), dim3(256), 0, stream, a, nIntervals);
}

}  // namespace mi355
