// jump_aux.h — what the Markov-jump tables of kernels_markovjumps.hip and kernels_robustcounts.hip share.  Device code only;
// include it from a .hip file that turns FMA contraction off.
#pragma once

namespace mi355 {

// A[a][b] of Minin & Suchard eq. 37 (MarkovJumpsCore.populateAuxInt) from ea = exp(lambda_a tau), eb = exp(lambda_b tau)
__device__ __forceinline__ double auxInt(double la, double lb, double ea, double eb, double tau) {
    return fabs(la - lb) < 1e-7 ? ea * tau : (ea - eb) / (la - lb);
}

}  // namespace mi355
