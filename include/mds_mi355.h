/* mds_mi355.h — C ABI of libmds2_jni.so: multidimensional scaling (MDS) on an AMD Instinct MI355X.
 *
 * One function per native of dr.inference.multidimensionalscaling.NativeMDSSingleton (NativeMDSSingleton.java:134-161), called
 * by MassivelyParallelMDSImpl for MultiDimensionalScalingLikelihood; the natives themselves (jni_mds/jni_mds.cpp) are copy-in /
 * copy-out wrappers over these.  The library stands alone: it does not need libhmsbeagle-jni.so.
 *
 * The arithmetic.  N locations x_i in D dimensions (1 <= D <= 8), a symmetric N x N table of observations y_ij with a zero
 * diagonal and NaN for a missing pair (behaviour on an asymmetric table is unspecified), precision tau = parameters[0],
 * d_ij = |x_i - x_j|, Phi and phi the standard normal distribution function and density:
 *
 *   increment(i,j) = tau (d_ij - y_ij)^2 / 2  +  [LEFT_TRUNCATION] log Phi(d_ij sqrt(tau))         i != j, y_ij not NaN
 *   S              = sum_{i<j} increment(i,j)                                                       mdsGetSumOfIncrements
 *   dlogL/dx_i     = - sum_{j != i} [tau (d_ij - y_ij) + [LEFT_TRUNCATION] sqrt(tau) phi(z)/Phi(z)] (x_i - x_j) / d_ij,
 *                    z = d_ij sqrt(tau)                                                             mdsGetLocationGradient
 *
 * S has tau applied in both modes: the caller computes log L = (log tau - log 2 pi) n / 2 - S with n the number of pairs that
 * are not missing (MassivelyParallelMDSImpl.java:122-127).  The diagonal carries no truncation term.  A pair with d_ij = 0
 * contributes nothing to the gradient: the limit has no direction, and the reference's Java core has no gradient to follow.
 * Everything is fp64.  Every sum is made in a fixed order without floating-point atomics: the same calls give the same bits.
 *
 * The state machine is the one of MultiDimensionalScalingCoreImpl: after exactly one single-location update since the last
 * mdsStoreState (and a known sum before it) mdsGetSumOfIncrements recomputes row k only — the old row from the location the
 * device still holds, the new one from the update, in one kernel launch; after an all-location update, a second single update,
 * mdsMakeDirty, mdsSetPairwiseData, or mdsSetParameters on a truncated instance it evaluates all pairs.  On an untruncated
 * instance the library keeps sum (d - y)^2 and applies tau on the way out, so a change of tau alone costs no pass.  Where the
 * Java core's table of increments would go stale (locations changed and stored without an evaluation in between) this library
 * evaluates all pairs instead.
 *
 * Conventions: a function returns 0 or a negative code (BEAGLE's numbering); mdsInitialize returns the instance number, 0, 1,
 * 2, ... in creation order per process (numbers are not reused).  Arrays are borrowed for the duration of the call; each comes
 * with its length, and one that is NULL or shorter than the call needs gives MDS_ERROR_OUT_OF_RANGE and changes nothing.
 * Calls on one instance are serialised; different instances may be driven from different threads.
 *
 * NOT BUILT, answered MDS_ERROR_NO_IMPLEMENTATION (-7): the rows x columns layout (mdsInitializeLayout, the native
 * initialize(IIIJII) used by NewAntigenicLikelihood), mdsGetObservationGradient, and D > 8.
 */
#ifndef MDS_MI355_H
#define MDS_MI355_H

#ifdef __cplusplus
extern "C" {
#endif

#define MDS_SUCCESS                        0
#define MDS_ERROR_GENERAL                 -1
#define MDS_ERROR_OUT_OF_MEMORY           -2
#define MDS_ERROR_UNIDENTIFIED_EXCEPTION  -3
#define MDS_ERROR_UNINITIALIZED_INSTANCE  -4
#define MDS_ERROR_OUT_OF_RANGE            -5
#define MDS_ERROR_NO_RESOURCE             -6   /* no MI355X visible: there is no CPU fallback */
#define MDS_ERROR_NO_IMPLEMENTATION       -7

/* flags: MultiDimensionalScalingCore.java.  Only LEFT_TRUNCATION changes anything; the others are accepted (fp64 runs at
 * full rate on this device, and one device is the whole of the parallelism). */
#define MDS_FLAG_USE_NATIVE_MDS            1
#define MDS_FLAG_SINGLE_PRECISION          4
#define MDS_FLAG_MULTI_CORE                8
#define MDS_FLAG_OPENCL_VECTORIZATION     16
#define MDS_FLAG_LEFT_TRUNCATION          32

#define MDS_MAX_DIMENSION                  8

/* initialize (IIJII)I.  deviceNumber -1 is device 0 (MassivelyParallelMDSImpl.java:59-69 sends mds.resource - 1); `threads`
 * is ignored.  Device memory: N * roundup(N, 16) doubles for the observations and O(N D) besides. */
int mdsInitialize(int dimension, int locationCount, long long flags, int deviceNumber, int threads);
/* initialize (IIIJII)I: not built, MDS_ERROR_NO_IMPLEMENTATION. */
int mdsInitializeLayout(int dimension, int rowLocationCount, int columnLocationCount, long long flags, int deviceNumber, int threads);
/* releases the instance; its number answers MDS_ERROR_UNINITIALIZED_INSTANCE from then on (the Java side never calls this). */
int mdsFinalize(int instance);

/* updateLocations (II[D)V: index -1 replaces all N * D values (location-major), index k >= 0 the D values of location k. */
int mdsUpdateLocations(int instance, int index, const double* values, long long length);
/* getSumOfIncrements (I)D */
int mdsGetSumOfIncrements(int instance, double* outSum);
/* storeState / restoreState / acceptState / makeDirty (I)V: locations, tau and the sum are kept and brought back. */
int mdsStoreState(int instance);
int mdsRestoreState(int instance);
int mdsAcceptState(int instance);
int mdsMakeDirty(int instance);
/* setPairwiseData (I[D)V, getPairwiseData (I)[D: N * N doubles, row-major.  Setting them makes the instance dirty. */
int mdsSetPairwiseData(int instance, const double* observations, long long length);
int mdsGetPairwiseData(int instance, double* outObservations, long long length);
/* setParameters (I[D)V: parameters[0] = tau. */
int mdsSetParameters(int instance, const double* parameters, long long length);
/* getLocationGradient (I[D)V: N * D doubles, location-major, the gradient of log L at the current locations and tau. */
int mdsGetLocationGradient(int instance, double* outGradient, long long length);
/* getObservationGradient (I[D)V: not built, MDS_ERROR_NO_IMPLEMENTATION. */
int mdsGetObservationGradient(int instance, double* outGradient, long long length);
/* getInternalDimension (I)I: D (no padding is exposed), or a negative code. */
int mdsGetInternalDimension(int instance);

/* not natives: what the natives and the tests need to know */
int mdsGetLocationCount(int instance);
/* out[0] evaluations over all pairs, [1] row updates, [2] gradients, [3] kernel launches so far, [4] kernel launches of the
 * last mdsGetSumOfIncrements (0: the sum was known), [5] the path it took (0 known, 1 row, 2 all pairs).  count <= 6. */
#define MDS_STATS_COUNT 6
int mdsStats(int instance, long long* out, int count);

#ifdef __cplusplus
}
#endif
#endif
