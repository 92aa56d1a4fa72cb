/*
 * beagle_mi355.h — C ABI of the MI355X-native tree-likelihood engine.
 *
 * This is the drop-in boundary.  Every entry point below is the plain-C shape of one
 * `native` method of the reference's JNI binding class
 *     /root/reference/lib/beagle.jar!beagle/BeagleJNIWrapper.class
 * (descriptors listed next to each function; the leading `I` of every descriptor is the
 * instance handle).  The Java-side caller of each method is cited as file:line relative
 * to /root/reference/.  Names follow BEAGLE's public C API (`beagle*`), which is what the
 * reference's `libhmsbeagle-jni.so` forwards to; the JNI symbols
 * `Java_beagle_BeagleJNIWrapper_<name>` live in csrc/jni_shim.cpp and call these functions
 * one-to-one.
 *
 * Conventions (lib/beagle.jar!beagle/BeagleErrorCode, BeagleJNIImpl):
 *   - every function returns an int error code: 0 = success, <0 = BEAGLE_ERROR_*;
 *     beagleCreateInstance returns the instance handle (>=0) or an error (<0);
 *   - arrays are borrowed for the duration of the call and may be LONGER than `count`
 *     (BeagleDataLikelihoodDelegate.java:179-183): exactly `count` (or 7*count / 9*count)
 *     entries are read;
 *   - index arrays documented "may be NULL" are accepted as NULL
 *     (HomogenousSubstitutionModelDelegate.java:260-261 passes null derivative indices);
 *   - BEAGLE_OP_NONE (-1) marks an unused scale/cumulative index (beagle.Beagle.NONE).
 *
 * Layouts at the boundary (lib/beagle.jar!beagle/GeneralBeagleImpl; BeagleTreeLikelihood.java:625-658):
 *   partials   double[C][P][S]      index c*P*S + p*S + i
 *   matrices   double[C][S][S]      row = parent state i, column = child state j
 *   eigen      U[i*S+k], Uinv[k*S+j] row-major S x S, lambda[S]
 *   tip states int[P], value >= S means missing/ambiguous (all-ones partial)
 * The layout in HBM is the engine's own.
 */
#ifndef BEAGLE_MI355_H
#define BEAGLE_MI355_H

#ifdef __cplusplus
extern "C" {
#endif
/* the engine is built with -fvisibility=hidden: what this header declares is what libhmsbeagle-jni.so exports (with the JNI natives) */
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

/* ---- error codes: lib/beagle.jar!beagle/BeagleErrorCode#<clinit> ------------------- */
#define BEAGLE_SUCCESS                      0
#define BEAGLE_ERROR_GENERAL               -1
#define BEAGLE_ERROR_OUT_OF_MEMORY         -2
#define BEAGLE_ERROR_UNIDENTIFIED_EXCEPTION -3
#define BEAGLE_ERROR_UNINITIALIZED_INSTANCE -4
#define BEAGLE_ERROR_OUT_OF_RANGE          -5
#define BEAGLE_ERROR_NO_RESOURCE           -6
#define BEAGLE_ERROR_NO_IMPLEMENTATION     -7
#define BEAGLE_ERROR_FLOATING_POINT        -8

#define BEAGLE_OP_NONE                     -1
#define BEAGLE_OP_COUNT                     7   /* beagle.Beagle.OPERATION_TUPLE_SIZE */
#define BEAGLE_PARTITION_OP_COUNT           9   /* MultiPartitionDataLikelihoodDelegate.java:972-997 */

/* ---- flag bits: lib/beagle.jar!beagle/BeagleFlag#<clinit> --------------------------- */
#define BEAGLE_FLAG_PRECISION_SINGLE    (1L << 0)
#define BEAGLE_FLAG_PRECISION_DOUBLE    (1L << 1)
#define BEAGLE_FLAG_COMPUTATION_SYNCH   (1L << 2)
#define BEAGLE_FLAG_COMPUTATION_ASYNCH  (1L << 3)
#define BEAGLE_FLAG_EIGEN_REAL          (1L << 4)
#define BEAGLE_FLAG_EIGEN_COMPLEX       (1L << 5)
#define BEAGLE_FLAG_SCALING_MANUAL      (1L << 6)
#define BEAGLE_FLAG_SCALING_AUTO        (1L << 7)
#define BEAGLE_FLAG_SCALING_ALWAYS      (1L << 8)
#define BEAGLE_FLAG_SCALERS_RAW         (1L << 9)
#define BEAGLE_FLAG_SCALERS_LOG         (1L << 10)
#define BEAGLE_FLAG_VECTOR_SSE          (1L << 11)
#define BEAGLE_FLAG_VECTOR_NONE         (1L << 12)
#define BEAGLE_FLAG_THREADING_OPENMP    (1L << 13)
#define BEAGLE_FLAG_THREADING_NONE      (1L << 14)
#define BEAGLE_FLAG_PROCESSOR_CPU       (1L << 15)
#define BEAGLE_FLAG_PROCESSOR_GPU       (1L << 16)
#define BEAGLE_FLAG_SCALING_DYNAMIC     (1L << 19)
#define BEAGLE_FLAG_FRAMEWORK_CUDA      (1L << 22)
#define BEAGLE_FLAG_FRAMEWORK_OPENCL    (1L << 23)
#define BEAGLE_FLAG_FRAMEWORK_CPU       (1L << 27)
#define BEAGLE_FLAG_PARALLELOPS_STREAMS (1L << 28)
#define BEAGLE_FLAG_PARALLELOPS_GRID    (1L << 29)
#define BEAGLE_FLAG_THREADING_CPP       (1L << 30)

/* Filled by beagleCreateInstance; mirrors beagle.InstanceDetails (setResourceNumber,
 * setFlags, setResourceName, setImplementationName — BeagleDataLikelihoodDelegate.java:454-480). */
typedef struct {
    int   resourceNumber;
    char* resourceName;
    char* implName;
    char* implDescription;
    long  flags;
} BeagleInstanceDetails;

/* One entry of beagleGetResourceList; mirrors beagle.ResourceDetails. */
typedef struct {
    char* name;
    char* description;
    long  supportFlags;
    long  requiredFlags;
} BeagleResource;

typedef struct {
    BeagleResource* list;
    int length;
} BeagleResourceList;

/* getVersion ()Ljava/lang/String;  — must match (\d+)\.(\d+)\.(\d+).* (beagle.jar!BeagleInfo#getVersionNumbers;
 * gates in treedatalikelihood/BeagleFunctionality.java:40-70). */
const char* beagleGetVersion(void);
/* getCitation ()Ljava/lang/String; */
const char* beagleGetCitation(void);
/* getResourceList ()[Lbeagle/ResourceDetails;  — resource 0 is the host by BEAST convention
 * (BeagleTreeLikelihood.java:90-92); resources 1..G are the visible MI355X devices. */
BeagleResourceList* beagleGetResourceList(void);

/* One entry of beagleGetBenchmarkedResourceList; mirrors beagle.BenchmarkedResourceDetails (lib/beagle.jar: ctor (I),
 * setResourceNumber, setName, setDescription, setSupportFlags, setRequiredFlags, setReturnCode, setImplName,
 * setBenchedFlags, setBenchmarkResult, setPerformanceRatio). */
typedef struct {
    int    number;             /* resource number (what the caller passes back to createInstance) */
    char*  name;
    char*  description;
    long   supportFlags;
    long   requiredFlags;
    int    returnCode;         /* of the benchmark's createInstance / evaluation on that resource */
    char*  implName;
    long   benchedFlags;
    double benchmarkResult;    /* milliseconds per full-tree evaluation of the benchmark workload */
    double performanceRatio;   /* relative to the fastest resource (1.0 = fastest) */
} BeagleBenchmarkedResource;

typedef struct {
    BeagleBenchmarkedResource* list;
    int length;
} BeagleBenchmarkedResourceList;

#define BEAGLE_BENCHFLAG_SCALING_NONE    (1L << 0)
#define BEAGLE_BENCHFLAG_SCALING_ALWAYS  (1L << 1)
#define BEAGLE_BENCHFLAG_SCALING_DYNAMIC (1L << 2)

/* getBenchmarkedResourceList (IIIII[IIJJIIIJ)[Lbeagle/BenchmarkedResourceDetails;  — BEAST's -beagle_auto
 * (BeagleTreeLikelihood.java:392-414, BeagleDataLikelihoodDelegate.java:413-433): times a full-tree evaluation of a
 * synthetic alignment of the caller's shape (tips, states, patterns, categories) on every candidate resource
 * (resourceList, or all GPU resources incl. the pattern-sharded one when it is NULL) and returns them fastest first.
 * The list is owned by the library and valid until the next call. */
BeagleBenchmarkedResourceList* beagleGetBenchmarkedResourceList(int tipCount, int compactBufferCount, int stateCount, int patternCount,
                                      int categoryCount, const int* resourceList, int resourceCount, long preferenceFlags,
                                      long requirementFlags, int eigenModelCount, int partitionCount, int calculateDerivatives,
                                      long benchmarkFlags);

/* createInstance (IIIIIIIII[IIJJLbeagle/InstanceDetails;)I
 * callers: BeagleTreeLikelihood.java:420-433, BeagleDataLikelihoodDelegate.java:439-452
 * 2..64 states; more returns BEAGLE_ERROR_NO_IMPLEMENTATION (no kernel of this engine is built for it). */
int beagleCreateInstance(int tipCount, int partialsBufferCount, int compactBufferCount,
                         int stateCount, int patternCount, int eigenBufferCount,
                         int matrixBufferCount, int categoryCount, int scaleBufferCount,
                         const int* resourceList, int resourceCount,
                         long preferenceFlags, long requirementFlags,
                         BeagleInstanceDetails* returnInfo);
/* finalize (I)I — BeagleDataLikelihoodDelegate.java:1234-1238 */
int beagleFinalizeInstance(int instance);
/* setCPUThreadCount (II)I — BeagleTreeLikelihood.java:461-467 (must return 0 on a GPU instance) */
int beagleSetCPUThreadCount(int instance, int threadCount);

/* setPatternWeights (I[D)I — BeagleTreeLikelihood.java:533 */
int beagleSetPatternWeights(int instance, const double* inPatternWeights);
/* setPatternPartitions (II[I)I — MultiPartitionDataLikelihoodDelegate.java:553 */
int beagleSetPatternPartitions(int instance, int partitionCount, const int* inPatternPartitions);
/* setTipStates (II[I)I — BeagleTreeLikelihood.java:696-710 */
int beagleSetTipStates(int instance, int tipIndex, const int* inStates);
/* getTipStates (II[I)I */
int beagleGetTipStates(int instance, int tipIndex, int* outStates);
/* setTipPartials (II[D)I — double[P*S], replicated over categories by the library
 * (beagle.jar!GeneralBeagleImpl#setTipPartials) */
int beagleSetTipPartials(int instance, int tipIndex, const double* inPartials);
/* setPartials (II[D)I — double[C*P*S]; BeagleTreeLikelihood.java:621-661 */
int beagleSetPartials(int instance, int bufferIndex, const double* inPartials);
/* getPartials (III[D)I — BeagleTreeLikelihood.java:1132-1136; scaleIndex != NONE un-scales */
int beagleGetPartials(int instance, int bufferIndex, int scaleIndex, double* outPartials);
/* getLogScaleFactors (II[D)I */
int beagleGetLogScaleFactors(int instance, int scaleIndex, double* outScaleFactors);

/* setEigenDecomposition (II[D[D[D)I — HomogenousSubstitutionModelDelegate.java:228-240 */
int beagleSetEigenDecomposition(int instance, int eigenIndex, const double* inEigenVectors,
                                const double* inInverseEigenVectors, const double* inEigenValues);
/* setStateFrequencies (II[D)I — BeagleTreeLikelihood.java:1030 */
int beagleSetStateFrequencies(int instance, int stateFrequenciesIndex, const double* inStateFrequencies);
/* setCategoryWeights (II[D)I — BeagleTreeLikelihood.java:1029 */
int beagleSetCategoryWeights(int instance, int categoryWeightsIndex, const double* inCategoryWeights);
/* setCategoryRates (I[D)I — BeagleTreeLikelihood.java:970 */
int beagleSetCategoryRates(int instance, const double* inCategoryRates);
/* setCategoryRatesWithIndex (II[D)I — MultiPartitionDataLikelihoodDelegate.java:835 */
int beagleSetCategoryRatesWithIndex(int instance, int categoryRatesIndex, const double* inCategoryRates);
/* setTransitionMatrix (II[DD)I — double[C*S*S] */
int beagleSetTransitionMatrix(int instance, int matrixIndex, const double* inMatrix, double paddedValue);
/* getTransitionMatrix (II[D)I — AncestralStateBeagleTreeLikelihood.java:331 */
int beagleGetTransitionMatrix(int instance, int matrixIndex, double* outMatrix);
/* convolveTransitionMatrices (I[I[I[II)I — treelikelihood/SubstitutionModelDelegate.java:382-405 */
int beagleConvolveTransitionMatrices(int instance, const int* firstIndices, const int* secondIndices,
                                     const int* resultIndices, int matrixCount);
/* updateTransitionMatrices (II[I[I[I[DI)I — HomogenousSubstitutionModelDelegate.java:247-266;
 * derivative index arrays may be NULL */
int beagleUpdateTransitionMatrices(int instance, int eigenIndex, const int* probabilityIndices,
                                   const int* firstDerivativeIndices, const int* secondDerivativeIndices,
                                   const double* edgeLengths, int count);
/* updateTransitionMatricesWithMultipleModels (I[I[I[I[I[I[DI)I — MultiPartitionDataLikelihoodDelegate.java:880-887 */
int beagleUpdateTransitionMatricesWithMultipleModels(int instance, const int* eigenIndices,
                                   const int* categoryRateIndices, const int* probabilityIndices,
                                   const int* firstDerivativeIndices, const int* secondDerivativeIndices,
                                   const double* edgeLengths, int count);

/* updatePartials (I[III)I — BeagleTreeLikelihood.java:1003, BeagleDataLikelihoodDelegate.java:904.
 * operations = int[7*count]: {dest, writeScale, readScale, child1, matrix1, child2, matrix2}
 * (tuple built at BeagleTreeLikelihood.java:1266-1299).  The list must be dependency ordered;
 * it need not be level ordered (the engine levelises it).  On an instance with several pattern partitions
 * the list covers every pattern: it runs as the 9-int list that names each operation once per non-empty
 * partition, in a row, with cumulativeScaleIndex as every tuple's cumulative index.  Whole-range
 * accumulate/remove/resetScaleFactors and calculateRootLogLikelihoods likewise cover all P patterns. */
int beagleUpdatePartials(int instance, const int* operations, int operationCount, int cumulativeScaleIndex);
/* updatePartialsByPartition (I[II)I — int[9*count]:
 * {dest, writeScale, readScale, child1, matrix1, child2, matrix2, partition, cumulativeScale} */
int beagleUpdatePartialsByPartition(int instance, const int* operations, int operationCount);
/* waitForPartials (I[II)I */
int beagleWaitForPartials(int instance, const int* destinationPartials, int destinationPartialsCount);

/* accumulateScaleFactors (I[III)I — BeagleTreeLikelihood.java:1016-1023 */
int beagleAccumulateScaleFactors(int instance, const int* scaleIndices, int count, int cumulativeScaleIndex);
/* accumulateScaleFactorsByPartition (I[IIII)I */
int beagleAccumulateScaleFactorsByPartition(int instance, const int* scaleIndices, int count,
                                            int cumulativeScaleIndex, int partitionIndex);
/* removeScaleFactors (I[III)I */
int beagleRemoveScaleFactors(int instance, const int* scaleIndices, int count, int cumulativeScaleIndex);
/* removeScaleFactorsByPartition (I[IIII)I */
int beagleRemoveScaleFactorsByPartition(int instance, const int* scaleIndices, int count,
                                        int cumulativeScaleIndex, int partitionIndex);
/* resetScaleFactors (II)I */
int beagleResetScaleFactors(int instance, int cumulativeScaleIndex);
/* resetScaleFactorsByPartition (III)I */
int beagleResetScaleFactorsByPartition(int instance, int cumulativeScaleIndex, int partitionIndex);
/* copyScaleFactors (III)I */
int beagleCopyScaleFactors(int instance, int destScalingIndex, int srcScalingIndex);

/* calculateRootLogLikelihoods (I[I[I[I[II[D)I — BeagleTreeLikelihood.java:1038-1039,
 * BeagleDataLikelihoodDelegate.java:934-935.  Returns BEAGLE_ERROR_FLOATING_POINT (-8) when
 * the sum is NaN; outSumLogLikelihood is still written (BeagleJNIImpl tolerates -8). */
int beagleCalculateRootLogLikelihoods(int instance, const int* bufferIndices,
                                      const int* categoryWeightsIndices, const int* stateFrequenciesIndices,
                                      const int* cumulativeScaleIndices, int count,
                                      double* outSumLogLikelihood);
/* calculateRootLogLikelihoodsByPartition (I[I[I[I[I[III[D[D)I — MultiPartitionDataLikelihoodDelegate.java:1074-1083 */
int beagleCalculateRootLogLikelihoodsByPartition(int instance, const int* bufferIndices,
                                      const int* categoryWeightsIndices, const int* stateFrequenciesIndices,
                                      const int* cumulativeScaleIndices, const int* partitionIndices,
                                      int partitionCount, int count,
                                      double* outSumLogLikelihoodByPartition, double* outSumLogLikelihood);
/* getSiteLogLikelihoods (I[D)I — BeagleTreeLikelihood.java:1050 */
int beagleGetSiteLogLikelihoods(int instance, double* outLogLikelihoods);

/* ---- pre-order partials and branch gradients ---------------------------
 * Semantics from the callers (the implementing library is not in the reference tree):
 * src/dr/evomodel/treedatalikelihood/preorder/AbstractBeagleGradientDelegate.java:115-151, 207-221 and
 * AbstractBeagleBranchGradientDelegate.java:52-95 (+ the arithmetic spelled out at :103-140). */

/* setRootPrePartials (I[I[II)I — pre-order partial of a root = its state frequencies, replicated over
 * patterns and categories (what AbstractBeagleGradientDelegate.java:142-151 does through setPartials). */
int beagleSetRootPrePartials(int instance, const int* bufferIndices, const int* stateFrequenciesIndices, int count);
/* setDifferentialMatrix (II[D)I — HomogenousSubstitutionModelDelegate.java:179-193: stateCount^2 * categoryCount
 * doubles into a matrix buffer (the infinitesimal matrix scaled per category rate,
 * discrete/DiscreteTraitBranchRateDelegate.java:49-89). */
int beagleSetDifferentialMatrix(int instance, int matrixIndex, const double* inMatrix);
/* transposeTransitionMatrices (I[I[II)I — AbstractBeagleGradientDelegate.java:93-105: result[n] = input[n]^T per category */
int beagleTransposeTransitionMatrices(int instance, const int* inputIndices, const int* resultIndices, int matrixCount);
/* updatePrePartials (I[III)I — AbstractBeagleGradientDelegate.java:120.  7-int tuples
 * {pre(child) dest, writeScale, readScale, pre(parent), matrix(child), post(sibling), matrix(sibling)} (:211-217), matrices
 * untransposed:  dest[j] = sum_i P_child[i][j] * ( pre(parent)[i] * sum_k P_sib[i][k] post(sib)[k] ).
 * The list is in pre-order (a parent's op before its children's); the engine levelises it. */
int beagleUpdatePrePartials(int instance, const int* operations, int operationCount, int cumulativeScaleIndex);
/* calculateEdgeDifferentials (I[I[I[I[II[D[D[D)I — AbstractBeagleBranchGradientDelegate.java:82-92.  Per edge e and
 * pattern p: num = sum_c w_c sum_j pre[c,p,j] sum_k D[c][j][k] post[c,p,k], den = sum_c w_c sum_j pre[c,p,j] post[c,p,j];
 * outSumDerivatives[e] = sum_p weight_p num/den, outSumSquaredDerivatives[e] = sum_p weight_p (num/den)^2,
 * outDerivatives[e*P + p] = num/den.  Any of the three outputs may be NULL (BEAST passes null for outDerivatives). */
int beagleCalculateEdgeDifferentials(int instance, const int* postBufferIndices, const int* preBufferIndices,
                                     const int* derivativeMatrixIndices, const int* categoryWeightsIndices, int count,
                                     double* outDerivatives, double* outSumDerivatives, double* outSumSquaredDerivatives);

/* calculateCrossProductDifferentials (I[I[I[I[I[DI[D[D)I — discrete/SubstitutionModelCrossProductDelegate.java:153-178.
 * The arithmetic lives only in the absent beagle-lib; the semantics follow the call site and its consumer, which names what it
 * expects: "a first-order" approximation of d lnL / d Q_ij (AbstractLogAdditiveSubstitutionModelGradient.java:74-93; its
 * AFFINE_CORRECTED mode adds a term computed in Java from the same numbers).  First-order form, pinned by finite differences of
 * the golden-pinned lnL along random generator perturbations (tests/test_oracle_golden.py: the error falls in proportion to
 * the branch lengths) and exactly in the scaling direction:
 *   outSumDerivatives[i*S+j] += sum_e edgeLengths[e] sum_p weight_p (sum_c w_c r_c pre_e[c,p,i] post_e[c,p,j]) / (sum_c w_c pre_e . post_e)
 * outSumSquaredDerivatives must be NULL (BEAST passes null); otherwise BEAGLE_ERROR_NO_IMPLEMENTATION. */
int beagleCalculateCrossProductDifferentials(int instance, const int* postBufferIndices, const int* preBufferIndices,
                                             const int* categoryRateIndices, const int* categoryWeightsIndices,
                                             const double* edgeLengths, int count,
                                             double* outSumDerivatives, double* outSumSquaredDerivatives);

/* ---- entry points that exist in the binding but are not built yet: exported so the JNI shim links, and
 * return BEAGLE_ERROR_NO_IMPLEMENTATION (-7). ------------------------------------------------------ */
int beagleAddTransitionMatrices(int instance, const int* firstIndices, const int* secondIndices,
                                const int* resultIndices, int matrixCount);
int beagleUpdatePrePartialsByPartition(int instance, const int* operations, int operationCount);

/* ---- MI355X extensions (not part of the reference binding) -------------------------- */

/* Make every subsequent call of this instance enqueue on `hipStream` (a hipStream_t) instead
 * of the instance's own stream — lets a host that owns streams (torch, a JVM-side pool)
 * order the engine against its collectives. */
int beagleMi355SetStream(int instance, void* hipStream);
/* As beagleCalculateRootLogLikelihoods with count == 1, but the weighted sum stays on the
 * device: it is written to `deviceOut` (a device pointer to one double) on the instance's
 * stream and nothing is synchronised.  The pattern-sharded multi-GPU path all-reduces that
 * double over RCCL (DESIGN.md, row e). */
int beagleMi355CalculateRootLogLikelihoodsDevice(int instance, int bufferIndex, int categoryWeightsIndex,
                                      int stateFrequenciesIndex, int cumulativeScaleIndex, void* deviceOut);
/* One process per GPU, unique site patterns sharded over the processes (the job BEAST runs as -beagle_instances G,
 * TreeDataLikelihoodParser.java:205-278, with its Java-side sum): the sum over the shards as ONE all-reduce inside the engine.
 * beagleMi355GetCommUniqueId fills 128 bytes on one rank; the host hands them to every rank (any channel) and each calls
 * beagleMi355CommInit(instance, id, rank, rankCount) — RCCL over xGMI, one communicator per instance.  Then
 * beagleMi355CalculateRootLogLikelihoodsAllReduce is beagleCalculateRootLogLikelihoods with count == 1 whose result is the
 * sum over ALL ranks: reduction kernel, ncclAllReduce of one double and the hand-over to the host are enqueued back to back on
 * the instance's stream; every rank gets the same value (BEAGLE_ERROR_FLOATING_POINT when it is NaN, on every rank alike). */
int beagleMi355GetCommUniqueId(void* out128);
int beagleMi355CommInit(int instance, const void* uniqueId128, int rank, int rankCount);
int beagleMi355CalculateRootLogLikelihoodsAllReduce(int instance, int bufferIndex, int categoryWeightsIndex,
                                      int stateFrequenciesIndex, int cumulativeScaleIndex, double* outGlobalSum);
/* How many ranks the instance's communicator has — RCCL's own count (ncclCommCount), 0 without a communicator; on the
 * pattern-sharded handle (resource G+1) the ranks of its in-library communicator (0: host-side sum, no RCCL).  What a multi-GPU
 * benchmark line quotes as proof that the collective really spanned N GPUs. */
int beagleMi355CommInfo(int instance, int* outRanks);
/* getPartials for `count` buffers in one call: out = [count][C][P][S] (API layout), scale factors folded in where
 * scaleIndices[k] != BEAGLE_OP_NONE (scaleIndices may be NULL).  One batched materialisation of virtual buffers, device-side
 * layout conversion, pinned copies, one synchronisation per 256 MiB — for hosts that read many nodes per sample
 * (AncestralStateBeagleTreeLikelihood.java:414-542); the per-buffer beagleGetPartials takes the same path with count 1. */
int beagleMi355GetPartialsBatch(int instance, const int* bufferIndices, const int* scaleIndices, int count, double* outPartials);
/* Ancestral states: ONE draw of every listed node's state per pattern, on the device — what AncestralStateBeagleTreeLikelihood
 * .traverseSample computes from a getPartials per internal node and a getTransitionMatrix per branch
 * (AncestralStateBeagleTreeLikelihood.java:414-625; linear-space conditionals, marginal mode).
 *   nodes: nodeCount triples {bufferIndex, matrixIndex, parentRow} in pre-order — row 0 is the root {rootBuffer, ignored, -1},
 *          every other row names its branch matrix and a parentRow smaller than its own.  A buffer may hold partials (internal
 *          node, or a tip set with setTipPartials) or compact tip states (not at the root); a compact state >= stateCount is
 *          drawn from the matrix row alone.
 *   outStates: [nodeCount][patternCount] bytes, row r = nodes[r];  outRateCategories: [patternCount] or NULL.
 *   flags: BEAGLE_MI355_ANCESTRAL_MAP = argmax instead of a draw (useMAP).
 * Rate category (C > 1) drawn from (sum_k rootPartial[c][p][k]) * categoryWeight[c]; root state from rootPartial[c*][p][i] * freq[i];
 * other rows from partial[c*][p][i] * M[c*][parentState][i].  Every draw is randomChoicePDF (MathUtils.java:82-104) with
 * u = SplitMix64 output number ctr + 1 from state `seed`, ctr = (row * patternCount + p) * 2 + kind (kind 1: the root's rate
 * category), u = (z >> 11) * 2^-53 — stateless, so a host can restate every draw; the sharded handle (resource G+1) keys it on the
 * global pattern and returns a single instance's states byte for byte.  Stored partials are read as they are (rescaling does not
 * change any draw).  BEAGLE_ERROR_OUT_OF_RANGE for a bad index, parent row or root, nodeCount < 1 or outStates == NULL;
 * BEAGLE_ERROR_NO_IMPLEMENTATION on an instance with more than one pattern partition; BEAGLE_ERROR_FLOATING_POINT when some
 * draw's total weight was not finite and > 0 — that state is 0 and every other draw is still made. */
#define BEAGLE_MI355_ANCESTRAL_MAP 1
int beagleMi355SampleAncestralStates(int instance, const int* nodes, int nodeCount, int categoryWeightsIndex, int stateFrequenciesIndex,
                                     unsigned long long seed, int flags, unsigned char* outStates, int* outRateCategories);
/* Sequence simulation: ONE call that draws an alignment FROM the model, down the tree — what dr.app.beagle.tools.Partition.traverse
 * computes from an updateTransitionMatrices and a getTransitionMatrix per branch and a randomChoicePDF per site in Java
 * (Partition.java:292-431, :519-536; BeagleSequenceSimulator).  It reads branch matrices, category weights and state frequencies and
 * nothing else: no partials, no patterns — siteCount is independent of the instance's pattern count, updatePartials need never have
 * been called, and an instance with pattern partitions is served like any other (the caller offsets its matrix indices).
 *   nodes: nodeCount triples {outRow, matrixIndex, parentRow} in pre-order — row 0 is the root {outRow, ignored, -1}, every other row
 *          names its branch matrix and a parentRow smaller than its own index.  outRow: the row of outStates that receives the node's
 *          states, -1 for a node the caller does not want (tips only = outputAncestralSequences false); every outRow >= 0 at most once.
 *   outStates: [1 + max outRow][siteCount] bytes; rows no node names are left alone.  outRateCategories: [siteCount] or NULL.
 *   inRateCategories (NULL: drawn): the rate category of every site, each < categoryCount.
 *   inRootStates (NULL: drawn): the root's state at every site, each < stateCount (setRootSequence).
 *   flags: none is defined; it must be 0.
 * Rate category of site s: inRateCategories[s], else (categoryCount > 1) a draw from the category weights, else 0.  Root state:
 * inRootStates[s], else a draw from the state frequencies.  Row r > 0: a draw from M[category][parentState][.] of its matrix as
 * beagleGetTransitionMatrix returns it (the caller's matrices: a tip's folded emission table is not part of it).
 * A draw over p_0 .. p_{n-1} is Partition.randomChoicePDF: cum_i = cum_{i-1} + p_i from cum_{-1} = 0.0 in index order (one IEEE
 * addition each), the result is the first i with u < cum_i.  Where no i satisfies it — rounding has left the total below u — the
 * reference returns an invalid index (-Integer.MAX_VALUE); HERE THE RESULT IS THE LARGEST INDEX WITH p_i > 0.  A vector that is
 * drawn from and whose total cum_{n-1} is not finite and > 0 gives 0 for that draw; every other draw is still made, the outputs are
 * written and the call returns BEAGLE_ERROR_FLOATING_POINT.
 * u = SplitMix64 output number ctr + 1 from state `seed` as (z >> 11) * 2^-53 (beagleMi355SampleAncestralStates' numbers), with
 * ctr = (row * siteCount + site) * 2 for a state and ctr = site * 2 + 1 for the rate category — stateless, so a host can restate
 * every draw, and the bytes depend on the seed alone: not on the launch shape, not on the chunks the sites are processed in
 * (BEAGLE_MI355_SIM_CHUNK_SITES=<n> overrides their size), not on the number of GPUs (the sharded handle, resource G+1, splits the
 * SITES into contiguous ranges; every shard holds all matrices).
 * The instance is left as it was found: partials, scale buffers, plans, tip states and folded tip emissions are not touched.
 * BEAGLE_ERROR_OUT_OF_RANGE for nodes or outStates NULL, nodeCount < 1, siteCount < 1, non-zero flags, a bad weight, frequency or
 * matrix index, a parent row that is not earlier than the row itself, an outRow below -1 or used twice, an input state >= stateCount
 * or an input category >= categoryCount (or negative).  An extension: no BEAST class calls it today. */
int beagleMi355SimulateSequences(int instance, const int* nodes, int nodeCount, int siteCount, int categoryWeightsIndex,
                                 int stateFrequenciesIndex, unsigned long long seed, int flags, const unsigned char* inRootStates,
                                 const int* inRateCategories, unsigned char* outStates, int* outRateCategories);
/* Node heights: d lnL / d h_i and d^2 lnL / d h_i^2 for every listed internal node i in ONE call, from the partials where they are —
 * what DiscreteTraitNodeHeightDelegate.getNodeDerivatives computes from a getPartials per post-order and per pre-order buffer and a
 * getTransitionMatrix per branch (DiscreteTraitNodeHeightDelegate.java:63-200; the NodeHeightGradient / NodeHeightHessian traits of
 * the divergence-time HMC).  Call it after a gradient pass: post-order partials, the pre-order partials of the INTERNAL nodes, the
 * branch matrices and the rate-scaled infinitesimal matrices (setDifferentialMatrix: Q x category rate, [C][S][S]) are all it reads.
 *   nodes: [nodeCount][8], one row per internal node i with children j, k:
 *          {pre(i), post(j), matrix(j), dmatrix(j), post(k), matrix(k), dmatrix(k), dmatrix(i)}; dmatrix(i) = -1 at the root.
 *          post(.) may hold compact tip states (a state >= stateCount: all ones), a tip's partials or an internal node's.
 *   rates: [nodeCount][3] = {r_j, r_k, r_i}, the branch rates (branch length = rate x height difference); r_i is ignored at the root.
 *   outFirst, outSecond: [nodeCount]; either may be NULL, not both.
 * Per pattern p and category c (weight w_c): x = the child's partial, a_j = P_j x_j, b_j = Q_j a_j, c_j = Q_j b_j (the same for k),
 * q = pre(i), u = Q_i^T q, v = Q_i^T u, and with <.> = sum_c w_c sum_s
 *   D    = <a_j a_k q>
 *   g_j  = <b_j a_k q>/D      g_k = <a_j b_k q>/D      g_i = <a_j a_k u>/D
 *   h_jj = <c_j a_k q>/D - g_j^2    h_kk likewise    h_jk = <b_j b_k q>/D - g_j g_k
 *   h_ii = <a_j a_k v>/D - g_i^2    h_ij = <b_j a_k u>/D - g_i g_j    h_ik likewise
 *   first[i]  = sum_p weight_p ( r_j g_j + r_k g_k - r_i g_i )
 *   second[i] = sum_p weight_p ( r_j^2 h_jj + r_k^2 h_kk + 2 r_j r_k h_jk + r_i^2 h_ii - 2 r_i r_j h_ij - 2 r_i r_k h_ik )
 * (the i terms dropped at the root).  Every ratio is free of scale factors: rescaled partials are read as they are.  The sums over
 * patterns are formed in a fixed order: two calls return the same bits.  The sharded handle adds its shards' sums.
 * BEAGLE_ERROR_OUT_OF_RANGE for a bad index, a pre(i) that holds tip states or nothing, NULL arguments, nodeCount < 1;
 * BEAGLE_ERROR_NO_IMPLEMENTATION with more than one pattern partition or more than 64 states; BEAGLE_ERROR_FLOATING_POINT when a
 * result is not finite — the outputs are still written.  An extension: no BEAST class calls it today. */
int beagleMi355NodeHeightDerivatives(int instance, const int* nodes, const double* rates, int nodeCount, int categoryWeightsIndex,
                                     double* outFirst, double* outSecond);
/* Substitution-parameter gradients: the "differential mass matrix" of every listed branch and rate category, formed on the device in
 * ONE call — what BranchSubstitutionParameterDelegate.cacheDifferentialMassMatrix (BranchSubstitutionParameterDelegate.java:62-81),
 * HomogeneousSubstitutionParameterGradient and ArbitrarySubstitutionGeneratorGradient form per branch on the host with
 * DifferentiableSubstitutionModelUtil.getExactDifferentialMassMatrix (DifferentiableSubstitutionModelUtil.java:57-171) and upload with a
 * beagleSetDifferentialMatrix per branch.  beagleCalculateEdgeDifferentials over the written slots then yields d lnL / d theta per branch.
 *   eigenIndices, categoryRatesIndices [count]: the branch's eigen system and rate set; NULL = 0 for every branch.
 *   inDifferentials [differentialCount][S][S], row-major: dQ / d theta of every parameter (and model) of the call.
 *   differentialIndices [count]: which of them the branch uses; NULL = 0 for every branch.
 *   matrixIndices [count]: the slot of the transition-matrix pool that receives the branch's C matrices, category-major as
 *          beagleSetDifferentialMatrix takes them; no slot twice in one call.
 *   edgeLengths [count]: branch length x clock rate.  With dist = edgeLengths[k] x rate(c) of the branch's rate set:
 * BEAGLE_MI355_DIFFERENTIAL_EXACT: D = U (V o Phi) U^-1 with V = U^-1 dQ U, entries of V with |V_ij| < 1e-10 set to 0 (the reference's
 *   setZeros), Phi_ij = dist where i = j or |lambda_i - lambda_j| < 1e-10, otherwise (1 - exp((lambda_j - lambda_i) dist)) /
 *   (lambda_i - lambda_j), and 0 where V_ij is 0: then dP / d theta = P D.  On an EIGEN_COMPLEX instance the 2 x 2 blocks of conjugate pairs
 *   (real-complex, complex-real, complex-complex and its special case of equal pairs) follow lines 88-160 of the same file with the
 *   exp-cosine and exp-sine integrals of lines 210-222; pairs are found as beagleUpdateTransitionMatrices finds them.
 * BEAGLE_MI355_DIFFERENTIAL_FIRST_ORDER: D = dist x dQ.
 * (The reference's affine-corrected form is not offered: its rule hangs on an eigenvalue being exactly 0.0.)
 * V is formed once per distinct (eigen system, differential) pair of the call; every sum runs over its index in ascending order, so a
 * slot receives the same bits whatever else the call lists, in whatever order, and on every shard.  Writing a slot does for it what
 * beagleSetTransitionMatrix does; a held-back pre-order list runs first only if it reads one of the written slots.  The sharded handle
 * gives the call to every shard (matrices are replicated).
 * BEAGLE_ERROR_OUT_OF_RANGE for a bad index, a slot named twice, another mode, differentialCount < 1, inDifferentials, matrixIndices or
 * edgeLengths NULL with count > 0, and for arguments that exceed half the 16 MiB staging ring;
 * BEAGLE_ERROR_NO_IMPLEMENTATION with more than 64 states and on a BASTA instance.  count <= 0: success, nothing is launched.
 * An extension: no BEAST class calls it today. */
#define BEAGLE_MI355_DIFFERENTIAL_EXACT        0
#define BEAGLE_MI355_DIFFERENTIAL_FIRST_ORDER  1
int beagleMi355UpdateDifferentialMatrices(int instance, const int* eigenIndices, const int* categoryRatesIndices,
                                          const double* inDifferentials, int differentialCount, const int* differentialIndices,
                                          const int* matrixIndices, const double* edgeLengths, int count, int mode);
/* Eigen systems of time-reversible models, decomposed on the device in ONE call — what the caller of beagleSetEigenDecomposition
 * computes per model on the host (SubstitutionModelDelegate.java:272-288; BaseSubstitutionModel.java:256-289, 314-319) and uploads with
 * one call per model.  After it, eigen slot eigenIndices[k] holds what beagleSetEigenDecomposition would have been handed for model k.
 *   relativeRates [count][S (S - 1) / 2]: the upper triangle of r in row order;  frequencies [count][S].
 * Q_ij = r_ij pi_j (i != j), rows summing to zero; n = -sum_i pi_i Q_ii; A_ij = sqrt(pi_i) r_ij sqrt(pi_j), A_ii = Q_ii (symmetric by
 * construction); A = V diag(mu) V^T by cyclic Jacobi in a fixed rotation order (csrc/kernels_eigen.hip), to off(A) <= eps ||A||_F;
 * U = Pi^-1/2 V, U^-1 = V^T Pi^1/2, lambda = mu / n, eigenvalues ascending with columns and rows to match; the S imaginary parts of an
 * EIGEN_COMPLEX instance are zeros.  A model that has not converged after 30 sweeps (none is known to need more than 8) gets NaN
 * eigenvalues — a likelihood behind it answers BEAGLE_ERROR_FLOATING_POINT — and is counted by beagleMi355EigenStats.
 * The call is queued behind everything queued on the instance; nothing is read back and the host does not wait.  A held-back
 * pre-order list stays held.  A later beagleSetEigenDecomposition into a written slot is always uploaded.  Input goes through the
 * staging ring; a list over half the ring is split into several launches, so no list is refused for its size.  A slot receives the
 * same bits whatever else the call lists, in whatever order or split, and on every shard: the sharded handle gives the call to every
 * shard (eigen systems are replicated).
 * BEAGLE_ERROR_OUT_OF_RANGE for a NULL pointer, count < 0, an index outside the eigen buffers or named twice, non-zero flags, a
 * frequency that is not finite and > 0, a rate that is not finite and >= 0, a model whose n is not finite and > 0;
 * BEAGLE_ERROR_NO_IMPLEMENTATION with more than 64 states.  Everything is checked before anything is queued: a refused call leaves
 * every slot as it was.  count == 0: success, nothing is launched.  An extension: no BEAST class calls it today. */
int beagleMi355SetReversibleModels(int instance, const int* eigenIndices, int count, const double* relativeRates,
                                   const double* frequencies, int flags);
/* Eigen slot eigenIndex back on the host, however it was filled: outEigenVectors and outInverseEigenVectors [S][S], outEigenValues [S]
 * ([2 S] on an EIGEN_COMPLEX instance).  Drains the instance's stream.  The sharded handle reads shard 0. */
int beagleMi355GetEigenDecomposition(int instance, int eigenIndex, double* outEigenVectors, double* outInverseEigenVectors,
                                     double* outEigenValues);
/* out4 = {beagleMi355SetReversibleModels calls since creation, models they decomposed, the most Jacobi sweeps a model of the last call
 * took, models of the last call that hit the cap of 30} (shard 0 of a sharded handle).  Drains the instance's stream. */
int beagleMi355EigenStats(int instance, long long* out4);
/* Transition matrices straight from generators, in ONE call and with no eigen system — for the models that have no real or no
 * well-conditioned one (ComplexSubstitutionModel, BSSVS / GLM rate matrices, BASTA's migration matrices; a defective generator is as
 * good as any other here).  Slot probabilityIndices[e] receives exp(Q_g d) for each of the C categories, as
 * beagleUpdateTransitionMatrices leaves them, by uniformization with scaling and squaring.
 *   generators [generatorCount][S][S] row-major: what getInfinitesimalMatrix returns (already normalised).  Rows need not sum to zero.
 *   generatorIndices [count] (NULL: 0 for every entry): the generator g of entry e.
 *   categoryRateIndices [count] (NULL: rate set 0): the rate set of entry e, as in beagleUpdateTransitionMatricesWithMultipleModels.
 *   probabilityIndices [count]: the slot of entry e, no slot twice in one call;  edgeLengths [count].
 * For generator g: mu = max_i -Q_ii (scanned upwards from i = 0, a later entry replaces an earlier one only if greater);
 *   B = Q / mu entry by entry, then + 1 on the diagonal;  B^0 = I, B^1 = B, B^k = B^(k-1) B for k = 2 .. 20, the inner index summed
 *   upwards from 0.0, every product rounded on its own (no fused multiply-add).
 * For entry e and category c: d = edgeLengths[e] * rate_c (one product, as beagleUpdateTransitionMatrices forms its distance);
 *   x = mu d;  s = the smallest integer >= 0 with x 2^-s <= 1;  tau = x 2^-s (exact);  w_0 = exp(-tau), w_k = w_(k-1) tau / k;
 *   T = sum_{k = 0 .. 20} w_k B^k, k upwards;  then s times T <- T T.
 * B and every T are non-negative, so nothing cancels: every entry is >= 0, structural zeros stay exact zeros, d = 0 gives I exactly, and
 * the componentwise relative error is of the order of (2^s + 20) eps (tests/generator_matrices_reference.py).  The power tables are
 * formed once per generator of the call.  The squarings run on the fp64 matrix cores from 16 states up (there the inner index is summed
 * four at a time) and with fused multiply-adds below; every sum has a fixed order and there are no atomics on values, so a slot's bits
 * depend on (Q_g, edgeLengths[e], rate_c) alone: not on its place in the list, on the split into launches, on the other generators of the
 * call or on the shard.  s > 40 (and an x that is not finite) writes NaN into that matrix and is counted by beagleMi355GeneratorStats — a
 * likelihood behind it answers BEAGLE_ERROR_FLOATING_POINT.
 * The call is queued behind everything queued on the instance; nothing is read back and the host does not wait.  Writing a slot does
 * for it what beagleUpdateTransitionMatrices does; a held-back pre-order list runs first only if it reads one of the written slots.
 * Input goes through the staging ring and the power tables (21 S^2 doubles a generator) through a scratch buffer: a list over either
 * budget is split into several launches, so no list is refused for its size.  It works on EIGEN_REAL and EIGEN_COMPLEX instances, on
 * partitioned ones and on instances with BASTA buffers, and writes matrix slots only.  The sharded handle gives the call to every shard.
 * BEAGLE_ERROR_OUT_OF_RANGE for generators, probabilityIndices or edgeLengths NULL, count < 0, generatorCount < 1, an index out of range, a
 * slot named twice, a Q entry that is not finite, a negative off-diagonal, a positive diagonal, mu not finite and > 0, an edge length
 * not finite or < 0;  BEAGLE_ERROR_NO_IMPLEMENTATION with more than 64 states.  Everything is checked before anything is queued: a
 * refused call leaves every slot as it was.  count == 0: success, nothing is launched.  Derivative matrices are not offered.
 * An extension: no BEAST class calls it today. */
int beagleMi355UpdateTransitionMatricesFromGenerators(int instance, const double* generators, int generatorCount,
                                                      const int* generatorIndices, const int* categoryRateIndices,
                                                      const int* probabilityIndices, const double* edgeLengths, int count);
/* out4 = {beagleMi355UpdateTransitionMatricesFromGenerators calls since creation, matrices (entry x category) they wrote, the largest s
 * of any of them, matrices refused (NaN) for s > 40} (shard 0 of a sharded handle).  Drains the instance's stream. */
int beagleMi355GeneratorStats(int instance, long* out4);
/* Branch matrices of epoch models in ONE call: a branch that crosses epoch boundaries gets the product of its segments' transition
 * matrices — what SubstitutionModelDelegate builds from one updateTransitionMatrices per eigen system into a pool of extra matrix
 * buffers and rounds of convolveTransitionMatrices (treelikelihood/SubstitutionModelDelegate.java:162-405).
 *   segmentOffsets [count + 1]: entry e owns segments segmentOffsets[e] .. segmentOffsets[e + 1] - 1; segmentOffsets[0] == 0, strictly
 *          increasing (every entry has a segment).  Segments come in the order of BranchModel.Mapping.getOrder(): root end first.
 *   segmentEigenIndices, segmentLengths [segmentOffsets[count]]: the eigen slot and the length (finite, >= 0) of each segment.
 *   categoryRateIndices [count] (NULL: rate set 0): the rate set of entry e, as in beagleUpdateTransitionMatricesWithMultipleModels.
 *   probabilityIndices [count]: the slot of entry e, no slot twice in one call.   flags: must be 0.
 * For entry e with segments j = 0 .. n - 1 and category c, M_j is what beagleUpdateTransitionMatrices leaves in a slot for (eigen slot
 * k_j, length l_j, the entry's rate set, category c): the distance l_j * rate_c is one product, the sums over the eigen index run upwards,
 * negative entries become 0, on real and on complex (conjugate-pair) eigen systems alike — the same code, so the same bits.  The slot
 * receives the left fold ((M_0 M_1) M_2) ... M_(n-1), the order the reference's deque produces (first x second -> result, pushed to the
 * front); an entry with n = 1 receives exactly M_0.
 * A product is sum_k a_ik b_kj, not clamped (as beagleConvolveTransitionMatrices).  Its order is fixed per state count:
 *   up to 15 states: k upwards from 0.0, one fused multiply-add per k;
 *   16 .. 64 states: on the fp64 matrix cores (v_mfma_f64_4x4x4), k four at a time in ascending order, each instruction adding its four
 *          products to the running sum, which starts at 0.0 (rows and columns are padded with zeros to a multiple of 4: the padded steps
 *          add 0 x 0).
 * There are no atomics on values, so a slot's bits depend on its own segments, rate set and category alone: not on its place in the
 * list, on the split into launches, on the other entries or on the shard.
 * The eigen systems, category rates and matrix slots are read and written where they are on the device (an eigen slot may have been
 * written by beagleMi355SetReversibleModels just before).  The call is queued behind everything queued on the instance; nothing is read
 * back and the host does not wait.  Writing a slot does for it what beagleUpdateTransitionMatrices does; a held-back pre-order list runs
 * first only if it reads one of the written slots.  Input goes through the staging ring: a list over its budget is split into several
 * launches (BEAGLE_MI355_EPOCH_CHUNK=<entries> in the environment, read at every call, forces a smaller split), so no list is refused for
 * its size.  It works on EIGEN_REAL and EIGEN_COMPLEX instances, on partitioned ones and on instances with BASTA buffers, and writes
 * matrix slots only.  The sharded handle gives the call to every shard.
 * BEAGLE_ERROR_OUT_OF_RANGE for a NULL segmentOffsets, segmentEigenIndices, segmentLengths or probabilityIndices, count < 0, offsets that
 * do not start at 0 or do not increase strictly (an entry without a segment), an index out of range, a slot named twice, a length not
 * finite or < 0, flags != 0;  BEAGLE_ERROR_NO_IMPLEMENTATION with more than 64 states.  Everything is checked before anything is queued: a
 * refused call leaves every slot as it was.  count == 0: success, nothing is read or launched.  Derivative matrices are not offered.
 * An extension: no BEAST class calls it today. */
int beagleMi355UpdateTransitionMatricesWithEpochs(int instance, const int* segmentOffsets, const int* segmentEigenIndices,
                                                  const double* segmentLengths, const int* categoryRateIndices,
                                                  const int* probabilityIndices, int count, int flags);
/* out4 = {beagleMi355UpdateTransitionMatricesWithEpochs calls since creation, matrices (entry x category) they wrote, segments they
 * processed, the longest entry (segments) of the last call} (shard 0 of a sharded handle).  Host counters: nothing is drained. */
int beagleMi355EpochStats(int instance, long* out4);
/* The stochastic Dollo (ALS) node-pattern likelihood: ONE call behind an ordinary pruning pass — what
 * AbstractObservationProcess.nodePatternLikelihood computes from a getPartials per node (tips included), a getLogScaleFactors per
 * internal node and a host loop over nodes x patterns x states (oldevomodel/MSSD/AbstractObservationProcess.java:174-210,
 * AnyTipObservationProcess.java:97-168, oldevomodel/treelikelihood/ScaleFactorsHelper.java:83-140).
 *   nodes [nodeCount][4] in post-order: {bufferIndex, scaleBufferIndex, child1Row, child2Row}.  A tip has both child rows -1 and its
 *          buffer holds compact states or partials; an internal row's children are two different earlier rows, and a row is a child at
 *          most once.  scaleBufferIndex: the buffer with the log factors the node's partials were divided by, or -1 (ignored on a tip row).
 *   nodeLogWeights [nodeCount]: logw_i = log(getNodeSurvivalProbability(i)), 0 at the root.
 *   deathState in [0, stateCount).
 * For row i and pattern j:
 *   site_ij   = sum_c w_c (sum_s pi_s x_i[c][j][s]), s and c upwards from 0.0 (a compact tip: pi_state, or sum_s pi_s for a code >=
 *               stateCount).  The reference reads one category's worth of partials and so only runs with ONE category; the
 *               category-weighted sum is this library's extension.
 *   Lambda_ij = (Lambda_child1 + Lambda_child2) + the row's own log scale factor; 0 on a tip row.
 *   extant_tj = 1 unless tip row t's code at j contains the death state: a compact tip, state < stateCount and != deathState; a tip held
 *               as partials, partial[category 0][j][deathState] == 0.
 *   below_ij  = sum of extant over the tip rows under i;  incl_ij = below_ij >= sum_t extant_tj.
 *   term_ij   = (log site_ij + Lambda_ij) + logw_i where incl_ij, else -inf.
 *   outLogPattern[j] = log sum_i exp(term_ij) by a running-maximum log-sum-exp over the rows in list order: (m, s) starts at (-inf, 0);
 *               a term above m makes s = s exp(m - term) + 1 and m = term, any other adds exp(term - m) to s; the result is m + log s,
 *               -inf where no row is included.  The reference forms the sum in linear space, which underflows on large trees; where it
 *               does not, exp(outLogPattern[j]) is its cumLike[j].  A term that is NaN or +inf makes the pattern's value NaN.
 *   outNodeLogTerms [nodeCount][patternCount] or NULL: term_ij.
 *   outSum (may be NULL) = sum_j patternWeight_j outLogPattern[j]: per 256 patterns by a fixed tree, then those sums in ascending order.
 *   flags: none is defined; it must be 0.
 * Nothing of the instance changes (buffers that the 4-state walk left unstored are materialised, as for beagleGetPartials; tips with a
 * folded emission table get their partials); a held-back pre-order list stays held unless it writes a listed buffer.  No atomics on
 * values: two calls return the same bits.  The rows are walked whole; a call whose scratch (Lambda and the extant count of the rows
 * pending at once, and with outNodeLogTerms a stage of every row) would pass 256 MiB is run in chunks of patterns
 * (BEAGLE_MI355_NODEPATTERN_CHUNK=<patterns> in the environment, read at every call: tests).  On the sharded handle every
 * shard fills its own pattern columns — the bits per pattern are those of one instance — and outSum adds the shards' sums in shard order.
 * 2..255 states, any category count.  BEAGLE_ERROR_OUT_OF_RANGE for a bad index, a row that is not post-order, deathState outside
 * [0, stateCount), flags != 0, nodeCount < 1, nodes, nodeLogWeights or outLogPattern NULL, a buffer nothing was ever written to;
 * BEAGLE_ERROR_NO_IMPLEMENTATION on an instance with pattern partitions or BASTA buffers or more than 255 states;
 * BEAGLE_ERROR_FLOATING_POINT when the sum is not finite (the outputs are still written); BEAGLE_ERROR_OUT_OF_MEMORY when the scratch
 * cannot be had.  An extension: no BEAST class calls it today (ALSBeagleTreeLikelihood.calculateLogLikelihood throws). */
int beagleMi355NodePatternLikelihoods(int instance, const int* nodes, const double* nodeLogWeights, int nodeCount, int deathState,
                                      int categoryWeightsIndex, int stateFrequenciesIndex, int flags, double* outLogPattern,
                                      double* outNodeLogTerms, double* outSum);
/* out4 = {beagleMi355NodePatternLikelihoods calls since creation, rows they walked, patterns they found included in no row, buffers
 * materialised for them} (the sum over the shards of a sharded handle). */
int beagleMi355NodePatternStats(int instance, long* out4);
/* Marginal node state posteriors P(state of node i = s | pattern): ONE call behind a pruning pass and a pre-order pass — what
 * NodePosteriorTreeLikelihood.calculatePosteriors computes from a getPartials and a getNodeMatrix per node and host loops over nodes x
 * patterns x states^2 (oldevomodel/treelikelihood/NodePosteriorTreeLikelihood.java:119-235), from the partials where they are.
 *   nodes [nodeCount][2] = {post(i), pre(i)}.  post(i): a compact tip's states (a state >= stateCount counts as all ones), a tip's
 *          partials, an internal node's partials, stored or left unstored by the 4-state walk.  pre(i): a partials buffer a pre-order list
 *          wrote — at the root what setRootPrePartials / setPartials put there.  A node may be listed more than once.
 *   flags: none is defined; it must be 0.
 * For row r, pattern p and state s, with w the weights of categoryWeightsIndex:
 *   m[s]         = sum_c (pre_c[p][s] * post_c[p][s]) * w_c, c upwards from 0.0, every product rounded on its own (no fused multiply-add);
 *   Z            = sum_s m[s], s upwards from 0.0;
 *   posterior[s] = m[s] / Z.
 * Z is the pattern's likelihood up to its scale factors at every node, so the ratio needs no matrix and no scale buffer: scaled partials
 * are read as they are.  The reference reads one category's matrices and so is meaningful with ONE category, where this is its value; the
 * category-weighted marginal is this library's extension.
 * Outputs — any may be NULL, not all:
 *   outPosteriors [nodeCount][patternCount][stateCount].
 *   outMapStates [nodeCount][patternCount]: the first s with the strictly largest posterior (drawChoice's rule under useMAP);
 *   outMapProbabilities [nodeCount][patternCount]: that posterior.
 *   outStateTotals [nodeCount][stateCount] = sum_p patternWeight_p posterior[p][s]: per 64 patterns by a fixed tree (v[i] += v[i + off]
 *          for off = 32, 16 .. 1; patterns past the end count 0.0), then those sums in ascending order from 0.0.  No atomics: two calls
 *          return the same bits.
 *   outCategoryPosteriors [patternCount][categoryCount], of the FIRST listed row (every node gives the same measure up to rounding):
 *          n_c = (sum_s pre_c[p][s] * post_c[p][s]) * w_c, s upwards from 0.0;  D = sum_c n_c, c upwards from 0.0;  entry = n_c / D.
 * A pattern of a row whose Z (for the categories: D) is 0 or not finite makes the call return BEAGLE_ERROR_FLOATING_POINT: every output
 * is still written, that (row, pattern) is NaN with MAP state 0, and it is left out of no total — the row's totals are NaN too.
 * Nothing of the instance changes (buffers that the 4-state walk left unstored are materialised, as for beagleGetPartials; tips with a
 * folded emission table get their partials; a held-back pre-order list runs first).  The rows are cut into launches whose descriptors
 * fit a quarter of the staging ring and whose output scratch stays within 256 MiB (BEAGLE_MI355_NODE_POSTERIOR_CHUNK=<rows> in the
 * environment, read at every call: tests); the bits do not depend on the cut, nor on the order of the list.  On the sharded handle
 * every shard fills its own pattern columns — the bits per pattern are those of one instance — and outStateTotals adds the shards' sums
 * in shard order.  2..255 states, any category count.
 * BEAGLE_ERROR_OUT_OF_RANGE for a bad index, a pre(i) that holds tip states or was never written, a post(i) never written, flags != 0,
 * nodes NULL, nodeCount < 1, every output NULL; BEAGLE_ERROR_NO_IMPLEMENTATION on an instance with pattern partitions or BASTA buffers
 * or more than 255 states; BEAGLE_ERROR_OUT_OF_MEMORY when the scratch cannot be had.  An extension: no BEAST class calls it today
 * (NodePosteriorTreeLikelihood is deprecated and runs on the Java cores only). */
int beagleMi355NodePosteriors(int instance, const int* nodes, int nodeCount, int categoryWeightsIndex, int flags,
                              double* outPosteriors, unsigned char* outMapStates, double* outMapProbabilities,
                              double* outStateTotals, double* outCategoryPosteriors);
/* out4 = {beagleMi355NodePosteriors calls since creation, node rows they covered, operands materialised for them, kernel launches}
 * (one shard's counters on a sharded handle: every shard runs the same rows).  Operands materialised: the distinct unstored buffers
 * among a call's listed ones when it arrived (a node listed twice counts once) — whether the held-back pre-order list that ran first
 * or the call itself then gave them real data. */
int beagleMi355NodePosteriorStats(int instance, long* out4);
/* Placement scores: for every (new sequence q, candidate attachment k), lnL(tree with q attached at k) - lnL(tree) over the sites kept,
 * in ONE call behind a pruning pass and a pre-order pass.  The reference's online inference (src/dr/app/realtime:
 * CheckPointTreeModifier.incorporateAdditionalTaxa :434-800, SimpleDistanceMatrix.calculatePairwiseDistance :63-93) places a new taxon next
 * to the existing taxon with the smallest p-distance; this is the likelihood that heuristic stands in for.
 *   candidates [candidateCount][7] = {parentPre, siblingPost, siblingMatrix, childPost, upperMatrix, lowerMatrix, pendantMatrix}.  The
 *          first four are the buffers of a pre-order operation for the branch; the last three are matrices the caller forms with
 *          updateTransitionMatrices in spare slots: P(parent -> attachment point), P(attachment point -> child), P(attachment point ->
 *          new tip).  siblingPost and siblingMatrix may both be BEAGLE_OP_NONE (no sibling factor), upperMatrix may be BEAGLE_OP_NONE
 *          (identity): {pre(root), NONE, NONE, post(root), NONE, P(x), pendant} is an attachment above the root.  siblingPost and
 *          childPost: a compact tip's states (a state >= stateCount counts as all ones), a tip's partials, an internal node's partials,
 *          stored or left unstored by the 4-state walk.
 *   sitePatterns [siteCount]: the pattern of each alignment site; -1 skips the site.
 *   queryCodes [queryCount][siteCount]: the code of each query at each site; 255 = missing, the site adds exactly 0.0.
 *   codeTable [codeCount][stateCount]: the emission row of each code (a state: a unit row; an ambiguity: several ones; any reals).
 *   flags: none is defined; it must be 0.
 * With M[a][b] = P(a -> b), w the weights of categoryWeightsIndex and g_x the row of code x, per candidate k, pattern p, category c:
 *   s_c(a) = sum_b Msib_c[a][b] post_sib,c,p(b)  (1 without a sibling);   u_c(a) = pre_parent,c,p(a) s_c(a);
 *   t_c(a) = sum_a' u_c(a') Mup_c[a'][a]  (u_c without an upper matrix);  l_c(a) = sum_b Mlow_c[a][b] post_child,c,p(b);
 *   e_c(a) = t_c(a) l_c(a);   D_p = sum_c w_c sum_a e_c(a);   N_p,x = sum_c w_c sum_a e_c(a) sum_b Mpend_c[a][b] g_x(b);
 *   T_k[p][x] = log(N_p,x / D_p);   score[q][k] = sum over the sites i kept of T_k[sitePatterns[i]][queryCodes[q][i]].
 * Every per-pattern scale factor of the three partials cancels in N / D, so no scale buffer is named and rescaled instances work as
 * they are.  Pattern weights are not read.  The score is formed as sum_j n[q][j] T_k[j] over j = p codeCount + x with n the exact
 * (integer) number of kept sites of q with pattern p and code x: segments of 8192 entries, each ascending from 0.0, then the segments
 * ascending from 0.0; a term with n = 0 is left out, so an entry of T that no site of q uses never reaches q's score.  The order
 * depends on (patternCount, codeCount) alone: two calls, a permuted or split candidate list and any chunk size give the same bits.
 *   outScores [queryCount][candidateCount];  outLogTable (may be NULL) [candidateCount][patternCount][codeCount] = T.
 * N = 0 gives -inf (an impossible observation, no error).  A pattern of a candidate whose D is 0 or not finite makes the call return
 * BEAGLE_ERROR_FLOATING_POINT after everything is written: that row of T is NaN, and so is every score that uses it.
 * Nothing of the instance changes (buffers that the 4-state walk left unstored are materialised, as for beagleGetPartials; tips with a
 * folded emission table get their partials; a held-back pre-order list runs first).  Candidates are cut into launches whose log table
 * stays within 256 MiB and queries into launches whose counts do (BEAGLE_MI355_PLACEMENT_CHUNK=<candidates>,
 * BEAGLE_MI355_PLACEMENT_QUERY_CHUNK=<queries> in the environment, read at every call: tests).  2..255 states, any category count.
 * BEAGLE_ERROR_OUT_OF_RANGE, before anything runs, for a bad buffer, matrix or weights index, a buffer never written, a sibling named
 * without its matrix, a pattern index >= patternCount or < -1, a code >= codeCount other than 255, codeCount > 255, flags != 0, a NULL
 * input or a count < 1.  BEAGLE_ERROR_NO_IMPLEMENTATION — deliberately out of scope — on an instance with pattern partitions, on an
 * instance with BASTA buffers, on a sharded handle, and with more than 255 states.  BEAGLE_ERROR_OUT_OF_MEMORY when the scratch
 * cannot be had.  An extension: no BEAST class calls it today. */
int beagleMi355PlacementScores(int instance, const int* candidates, int candidateCount, int categoryWeightsIndex,
                               const int* sitePatterns, int siteCount, const unsigned char* queryCodes, int queryCount,
                               const double* codeTable, int codeCount, int flags, double* outScores, double* outLogTable);
/* out4 = {beagleMi355PlacementScores calls since creation, candidates they covered, operands materialised for them, kernel launches}.
 * Operands materialised: the distinct unstored buffers among a call's listed ones when it arrived. */
int beagleMi355PlacementStats(int instance, long* out4);
/* Regraft scores: for every candidate attachment k, lnL(T' with a pruned subtree hung at k) - lnL(T'), in ONE call behind a pruning pass
 * and a pre-order pass over T', the tree without the subtree.  The reference's Gibbs tree operator (src/dr/evomodel/operators/
 * GibbsPruneAndRegraft.java: gibbsProposal :89-160, prunedGibbsProposal :162-269) edits the tree twice and evaluates the whole
 * likelihood once per candidate; everything those likelihoods are made of is resident after one gradient pass over T'.
 *   candidates [candidateCount][7] = {parentPre, siblingPost, siblingMatrix, childPost, upperMatrix, lowerMatrix, pendantMatrix}: the
 *          rows of beagleMi355PlacementScores, with the same rules — siblingPost and siblingMatrix may both be BEAGLE_OP_NONE,
 *          upperMatrix may be BEAGLE_OP_NONE, {pre(root), NONE, NONE, post(root), NONE, P(x), pendant} is an attachment above the root;
 *          siblingPost and childPost: compact tip states, a tip's partials, a tip behind an emission table, an internal node's
 *          partials, stored or left unstored by the 4-state walk.  pendantMatrix: P(attachment point -> the subtree's root); the Gibbs
 *          operator keeps the height of the subtree's parent, so its list names one.
 *   subtreeBuffer: the post-order buffer of the pruned subtree's root, of any of those kinds (a pruned tip: its compact states, a
 *          state >= stateCount counting as all ones).
 *   subtreeCumulativeScaleIndex: a scale buffer that holds the subtree's accumulated scale factors, or BEAGLE_OP_NONE.
 *   flags: none is defined; it must be 0.
 * With s, u, t, l and e as for beagleMi355PlacementScores and w the weights of categoryWeightsIndex, per candidate k, pattern p,
 * category c:
 *   q_c(a) = sum_b Mpend_c[a][b] post_sub,c,p(b);   D_p = sum_c w_c sum_a e_c(a);   N_p = sum_c w_c sum_a e_c(a) q_c(a);
 *   R_k[p] = log(N_p / D_p) + logscale_sub[p];      score[k] = sum_p patternWeight_p R_k[p].
 * logscale_sub is there only when a scale buffer is named: the value beagleGetLogScaleFactors returns for it, whichever form the
 * instance keeps.  lnL(T' with the subtree at k) = lnL(T') + score[k].  Every per-pattern scale factor of the three partials of T'
 * cancels in N / D, so rescaled instances work as they are.  The pattern weights are the instance's own (beagleSetPatternWeights).
 * The score is summed over segments of 64 patterns, each ascending from 0.0, then the segments ascending from 0.0; a pattern of
 * weight 0 is left out, so its -inf or NaN never reaches the score.  The order depends on patternCount alone: two calls, a permuted
 * or split candidate list and any chunk size give the same bits.
 *   outScores [candidateCount];  outPatternLogRatios (may be NULL) [candidateCount][patternCount] = R.
 * N = 0 gives -inf (an impossible attachment, no error).  A pattern of a candidate whose D is 0 or not finite makes the call return
 * BEAGLE_ERROR_FLOATING_POINT after everything is written: that R is NaN, and so is every score that uses it (at a pattern of weight 0
 * no score does: that R is NaN and the call succeeds).
 * Nothing of the instance changes (buffers that the 4-state walk left unstored are materialised, as for beagleGetPartials; tips with a
 * folded emission table get their partials; a held-back pre-order list runs first).  Candidates are cut into launches whose log ratios
 * stay within 256 MiB (BEAGLE_MI355_REGRAFT_CHUNK=<candidates> in the environment, read at every call: tests).  2..255 states, any
 * category count.
 * BEAGLE_ERROR_OUT_OF_RANGE, before anything runs, for a bad buffer, matrix, weights or scale index, a buffer never written (the
 * subtree's included), a sibling named without its matrix, flags != 0, a NULL input, a count < 1, or an instance without pattern
 * weights.  BEAGLE_ERROR_NO_IMPLEMENTATION — deliberately out of scope — on an instance with pattern partitions, on an instance with
 * BASTA buffers, on a sharded handle, and with more than 255 states.  BEAGLE_ERROR_OUT_OF_MEMORY when the scratch cannot be had (a
 * pendant vector of the subtree's size per DISTINCT pendant matrix).  An extension: no BEAST class calls it today. */
int beagleMi355RegraftScores(int instance, const int* candidates, int candidateCount, int subtreeBuffer,
                             int subtreeCumulativeScaleIndex, int categoryWeightsIndex, int flags, double* outScores,
                             double* outPatternLogRatios);
/* out4 = {beagleMi355RegraftScores calls since creation, candidates they covered, operands materialised for them, kernel launches}.
 * Operands materialised: the distinct unstored buffers among a call's listed ones (the subtree's included) when it arrived. */
int beagleMi355RegraftStats(int instance, long* out4);
/* Markov jumps: ONE call that draws the ancestral states as beagleMi355SampleAncestralStates does and, for every register k, row
 * r >= 1 and pattern p, forms the expected number of registered substitutions (a count register) or the expected reward (a reward
 * register) on row r's branch, conditioned on the drawn parent and child states — what MarkovJumpsBeagleTreeLikelihood.hookCalculation
 * computes inside traverseSample with useUniformization = false (MarkovJumpsBeagleTreeLikelihood.java:429-567).
 *   nodes, nodeCount, categoryWeightsIndex, stateFrequenciesIndex, seed, flags: as for beagleMi355SampleAncestralStates; the states
 *          and categories are the bytes that call returns.  outStates [nodeCount][patternCount] and outRateCategories [patternCount]
 *          may be NULL here.
 *   branchTimes[r]: parent height - child height;  branchRates[r] (NULL: all 1.0).  Row 0 (the root) is ignored.
 *   eigenIndex, categoryRatesIndex: the eigen system and the category rates rate_c the registers and times are formed from.
 *   registers: registerCount (1..8) matrices of S x S doubles R_k;  registerFlags[k] (NULL: all 0) = BEAGLE_MI355_JUMPS_REWARDS for a
 *          reward register, | BEAGLE_MI355_JUMPS_SCALE_BY_TIME to divide by branchRate * categoryRate (scaleByTime).
 * Count register: rateReg = Q o R with R's diagonal 0 (MarkovJumpsSubstitutionModel.setRegistration / makeRateRegistrationMatrix),
 * Q = U diag(lambda) U^-1 formed on the device from eigen system eigenIndex — the engine keeps no Q of its own, so Q equals the
 * reference's getInfinitesimalMatrix up to rounding.  Reward register: rateReg = diag(R[i][i]) (only the diagonal is read).
 * M_k = U^-1 rateReg_k U (PRECOMPUTE).  With c = category[p], i = state[parent(r)][p], j = state[r][p],
 * tau = (branchTimes[r] * branchRates[r]) * rate_c (substTime * branchRate * rate, :499/:533 — the bits of the engine's transition
 * distance when row r's matrix was built from edge length branchRate * time):
 *   rate_c > 0: A[a][b] = |la - lb| < 1e-7 ? e^(la tau) tau : (e^(la tau) - e^(lb tau)) / (la - lb);  J = U ((A o M_k) U^-1);
 *               V = J[i][j] / P_r[c][i][j] with P_r the instance's matrix of row r (hookCalculation divides by getMatrix);
 *               SCALE_BY_TIME: V = V / (branchRates[r] * rate_c)   (MarkovJumpsCore.computeCondStatMarkovJumpsPrecompute)
 *   rate_c <= 0: V = 0, except a reward register with SCALE_BY_TIME: V = (i == j) ? branchTimes[r] : 0 (:553-559).
 *   row 0: V = 0.
 * Outputs (any may be NULL, not all three; all deterministic — two identical calls give identical bits):
 *   outJumps [K][nodeCount][patternCount] = V (the <tag>_base trait);
 *   outPatternTotals [K][patternCount] = sum over rows 1 .. nodeCount-1 in row order (the c_<tag>[p] column, :640-654);
 *   outRowTotals [K][nodeCount] = sum over the instance's patterns, unweighted (TreeTrait.SumAcrossArrayD: the <tag>_sum trait).
 * The sharded handle (resource G+1) returns one instance's states, categories, outJumps and outPatternTotals byte for byte;
 * outRowTotals there is the shards' sums added in shard order (equal to one instance's to rounding).
 * Errors: those of beagleMi355SampleAncestralStates, and BEAGLE_ERROR_OUT_OF_RANGE for registerCount outside 1..8, an unknown
 * register-flag bit, a bad eigenIndex or categoryRatesIndex, branchTimes or registers NULL, or all three jump outputs NULL;
 * BEAGLE_ERROR_NO_IMPLEMENTATION on an EIGEN_COMPLEX instance or one with more than one pattern partition;
 * BEAGLE_ERROR_FLOATING_POINT when a draw failed or some V is not finite — everything else is still written. */
#define BEAGLE_MI355_JUMPS_REWARDS       1
#define BEAGLE_MI355_JUMPS_SCALE_BY_TIME 2
int beagleMi355SampleMarkovJumps(int instance, const int* nodes, int nodeCount, const double* branchTimes, const double* branchRates,
                                 int eigenIndex, int categoryRatesIndex, int categoryWeightsIndex, int stateFrequenciesIndex,
                                 const double* registers, const int* registerFlags, int registerCount, unsigned long long seed, int flags,
                                 unsigned char* outStates, int* outRateCategories, double* outJumps, double* outPatternTotals,
                                 double* outRowTotals);
/* Markov jumps by uniformization: ONE call that draws the ancestral states as beagleMi355SampleMarkovJumps does (same keys: the same
 * seed gives the same states) and then, for every simulant s, row r >= 1 and pattern p, SAMPLES an endpoint-conditioned
 * substitution history on row r's branch — what MarkovJumpsBeagleTreeLikelihood.computeSampledMarkovJumpsForBranch computes with
 * useUniformization = true (MarkovJumpsBeagleTreeLikelihood.java:473-509; UniformizedSubstitutionModel, SubordinatedProcess,
 * UniformizedStateHistory.simulateConditionalOnEndingState).  No eigen system is read, so it works on EIGEN_COMPLEX instances.
 *   nodes, nodeCount, branchTimes, branchRates, categoryRatesIndex, categoryWeightsIndex, stateFrequenciesIndex, registers,
 *          registerFlags, registerCount, seed, flags, outStates, outRateCategories, outJumps, outPatternTotals, outRowTotals: as for
 *          beagleMi355SampleMarkovJumps (layouts and summation orders included).
 *   nodeHeights[r]: row r's node height (only read for histories).
 *   infinitesimalMatrix: Q, S x S row-major (getInfinitesimalMatrix).  mu = max_i -Q_ii, R = I + Q / mu (entry by entry: Q/mu, then
 *          +1 on the diagonal); R^n = R^(n-1) R summed over the inner index in ascending order, no FMA (MarkovJumpsCore.matrixMultiply).
 *   simulantCount: 1..1024; the value is the mean over simulants (summed in simulant order, then / simulantCount).
 * With i = state[parent(r)][p], j = state[r][p], c = category[p], tau = (branchTimes[r] * branchRates[r]) * rate_c, P_ij = the
 * instance's matrix of row r [c][i][j], and u_q = the q-th number of the history's stream (below):
 *   n: the table holds R^0 .. R^(N-1), N = min(1000, ceil(lambda + 20 sqrt(lambda)) + 40), lambda = mu * the largest tau of the call
 *          (every row >= 1 and category with rate_c > 0).  cdf = 0, scale = 1, eff = mu tau; for n = 0, 1, ...: while u_0 >= cdf:
 *          n > 0: scale = scale * eff; n > 1: scale = scale / n; cdf = cdf + ((exp(-eff) * scale) * R^n[i][j]) / P_ij
 *          (SubordinatedProcess.drawNumberOfChanges).  Reaching n = N is the reference's fallback after maxTries
 *          (RETURN_UNIFORMLY_DISTRIBUTED_EVENT): one change i -> j at f = u_1 when i != j, none otherwise; it is counted into
 *          *outFallbacks and is not an error.
 *   n = 0, or n = 1 with i == j: no change.  n = 1 with i != j: one change at f = u_1.
 *   n >= 2: spacings E_q = -log(1 - u_q), q = 1..n+1, S_m = E_1 + .. + E_m, jump m at f_m = S_m / S_(n+1) (the order statistics of n
 *          uniforms).  State draw m = 1..n-1 from the current state cur: weights R[cur][k] * R^(n-m)[k][j], drawn with u_(n+1+m) as
 *          beagleMi355SampleAncestralStates draws (randomChoicePDF); a draw k != cur is a change at f_m.  Then, if cur != j, a change to
 *          j at f_n.  f is the fraction of tau from the parent.
 *   Register values per simulant, over the real changes in time order from 0.0, with t = f * tau: a count register adds
 *          R_k[from][to] (its diagonal is never read); a reward register adds R_k[from][from] * (t - t_previous) per change, then
 *          R_k[j'][j'] * (tau - t_last) for the final state j' (t_previous starts at 0).  SCALE_BY_TIME divides the mean by
 *          branchRates[r] * rate_c.  rate_c <= 0: the rule of beagleMi355SampleMarkovJumps, and no change.  Row 0: 0.
 *   Every register of a simulant reads the SAME history: "all jumps" = "upper" + "lower" in every sample.
 * Random numbers: the history of (s, r, p) has the stream z = SplitMix64's output for key = (s * nodeCount + r) * globalP + p (p the
 * pattern of the whole alignment), from the state seed ^ 0x6A09E667F3BCC909, as a 64-bit integer; u_q is SplitMix64's (q + 1)-th
 * output from the state z, as beagleMi355SampleAncestralStates forms its numbers.
 * Histories (simulantCount == 1 and nodeHeights non-NULL; asked for when any of outEventCounts, outEventHeights, outEventStates,
 * outEventTotal is non-NULL):
 *   outEventCounts [nodeCount][patternCount]: the real changes of each (row, pattern);
 *   events ordered by pattern, then node-list row, then time from the parent: outEventHeights[e] = h_parent + f * (h_child - h_parent)
 *          (nodeHeights of row r's parent row and of row r: rescaleTimesOfEvents), outEventStates[2e], [2e + 1] = from, to;
 *   *outEventTotal: the number of events (always written when non-NULL).  More than eventCapacity: no event is written, everything
 *          else is, and the call returns BEAGLE_ERROR_OUT_OF_RANGE — the draws are keyed, so a second call with a larger buffer is exact.
 * The sharded handle (resource G+1) returns one instance's states, categories, outJumps, outPatternTotals, event counts and events
 * byte for byte (a shard's events follow the earlier shards'); outRowTotals is the shards' sums added in shard order.
 * Errors: BEAGLE_ERROR_OUT_OF_RANGE for registerCount outside 1..8, an unknown register-flag bit, simulantCount outside 1..1024,
 * infinitesimalMatrix NULL or not finite or with mu not > 0, histories asked for with simulantCount > 1 or without nodeHeights, all
 * outputs NULL, a bad categoryRatesIndex, the errors of beagleMi355SampleAncestralStates, and a full event buffer (above);
 * BEAGLE_ERROR_NO_IMPLEMENTATION with more than one pattern partition; BEAGLE_ERROR_FLOATING_POINT when a draw failed, P_ij of a
 * drawn pair is not finite and > 0, or some value is not finite — everything else is still written. */
int beagleMi355SampleMarkovJumpsUniformized(int instance, const int* nodes, int nodeCount, const double* branchTimes,
                                            const double* branchRates, const double* nodeHeights, const double* infinitesimalMatrix,
                                            int categoryRatesIndex, int categoryWeightsIndex, int stateFrequenciesIndex,
                                            const double* registers, const int* registerFlags, int registerCount, int simulantCount,
                                            unsigned long long seed, int flags, unsigned char* outStates, int* outRateCategories,
                                            double* outJumps, double* outPatternTotals, double* outRowTotals, int* outEventCounts,
                                            long long eventCapacity, double* outEventHeights, unsigned char* outEventStates,
                                            long long* outEventTotal, long long* outFallbacks);
/* Codon robust counts ("renaissance counting", the per-site and per-branch dN/dS of CodonPartitionedRobustCounting): ONE call that
 * draws the ancestral states of the three codon-position instances, joins them into codon states and gathers, for every register k,
 * row r >= 1 and site p, the Minin-Suchard conditional mean count on row r's branch of the 64-state product chain of the three
 * nucleotide models — what CodonPartitionedRobustCounting.computeAllExpectedCounts computes from three getStatesForNode read-backs
 * and one MarkovJumpsCore table per branch and labelling (CodonPartitionedRobustCounting.java:216-307, ProductChainSubstitutionModel).
 *   instances [3]: codon positions 1, 2, 3 — three DIFFERENT ordinary 4-state instances on one device with the same pattern count P
 *          and one pattern partition each.  Patterns are sites: the reference requires uncompressed patterns (:138-146).
 *   nodes [3][nodeCount][3]: nodes + q * nodeCount * 3 is position q's node list exactly as beagleMi355SampleAncestralStates takes it
 *          ({bufferIndex, matrixIndex, parentRow}, row 0 the root); the parentRow columns of the three lists must agree.
 *   categoryWeightsIndices [3], stateFrequenciesIndices [3], seeds [3], flags (BEAGLE_MI355_ANCESTRAL_MAP): per position, as for that
 *          call.  Position q's states are byte for byte what beagleMi355SampleAncestralStates(instances[q], nodes[q], nodeCount,
 *          categoryWeightsIndices[q], stateFrequenciesIndices[q], seeds[q], flags, ..) returns (same keys, same numbers); one shared
 *          seed would give three identical alignments identical draws.  Rate categories of the instances are drawn and otherwise unused.
 *   branchLengths [nodeCount]: tau_r = branch rate x time of row r's branch in the product chain's time; row 0 is ignored.
 *   eigenVectors U, inverseEigenVectors U^-1 [64][64] row-major, eigenValues lambda [64] (real), infinitesimalMatrix Q [64][64]: the
 *          product chain (ProductChainSubstitutionModel.java:301-362); state = s0 * 16 + s1 * 4 + s2, first position most significant.
 *          Q is the SUPPLIED matrix, not one formed from the eigen system.  There are no rate categories (:81-87).
 *   registers [registerCount][64][64], registerCount 1..8: R_k; the diagonal is never read (taken as 0).
 *   includeRows [nodeCount] or NULL (all): rows with includeRows[r] != 0 enter outSiteTotals (includeExternalBranches /
 *          includeInternalBranches); nothing else depends on it.
 * Tables: rateReg_k = Q o R_k (MarkovJumpsSubstitutionModel.java:84-131), M_k = U^-1 (rateReg_k U); per row r >= 1 with tau = tau_r:
 *   A[a][b] = |la - lb| < 1e-7 ? e^(la tau) tau : (e^(la tau) - e^(lb tau)) / (la - lb);  J = U ((A o M_k) U^-1)
 *          (MarkovJumpsCore.java:84-103, 198-221);
 *   P = |U (diag(e^(lambda tau)) U^-1)| entry by entry, the products e^(la tau) * U^-1[a][j] first (BaseSubstitutionModel.java:206-240):
 *          the product chain's own matrix, not an instance's;  Cond_k,r = J / P entry by entry.  Row 0: 0.
 * Every product is rounded on its own (no fused multiply-add) and every sum runs over its inner index in ascending order from 0.0.
 * Outputs (any may be NULL, not all four; all deterministic — two identical calls give identical bits, and asking for fewer
 * outputs does not change the bits of the others):
 *   outStates [3][nodeCount][P] bytes or NULL: the three draws;
 *   outCounts [K][nodeCount][P] = Cond_k,r[codon of parent(r) at p][codon of r at p], row 0: 0;
 *   outSiteTotals [K][P] = sum over the included rows 1 .. nodeCount-1 in row order from 0.0;
 *   outBranchTotals [K][nodeCount] = sum over the sites: per workgroup of 256 consecutive sites a wave's 64 by an xor-shuffle tree
 *          (distances 32 .. 1), the four waves in wave order, then the workgroups in ascending order; row 0: 0;
 *   outTables [K][nodeCount][64][64] = Cond.
 * A zero-length branch leaves 0/0 off the diagonal of its table, as in the reference; the gather only reads its diagonal there, which
 * is 0 — that is not an error.  BEAGLE_ERROR_FLOATING_POINT when a draw failed or a GATHERED value is not finite; everything else is
 * still written.  BEAGLE_ERROR_OUT_OF_RANGE for a NULL input, nodeCount < 1, registerCount outside 1..8, an unknown flag bit, all
 * four double outputs NULL, parent rows that disagree, the same instance named twice, and every error of
 * beagleMi355SampleAncestralStates; BEAGLE_ERROR_NO_IMPLEMENTATION for a state count other than 4, differing pattern counts,
 * differing devices, the sharded handle (resource G+1) and an instance with more than one pattern partition.
 * The instances are left as they were found: plans, partials, scale buffers and the likelihood path stay bit for bit.
 * Out of scope: useUniformization = "true" for robust counting (sampled codon histories), sharded and partitioned instances, product
 * chains other than 4 x 4 x 4.  An extension: no BEAST class calls it today. */
int beagleMi355RobustCounts(const int* instances, const int* nodes, int nodeCount, const int* categoryWeightsIndices,
                            const int* stateFrequenciesIndices, const unsigned long long* seeds, int flags, const double* branchLengths,
                            const double* eigenVectors, const double* inverseEigenVectors, const double* eigenValues,
                            const double* infinitesimalMatrix, const double* registers, int registerCount,
                            const unsigned char* includeRows, unsigned char* outStates, double* outCounts, double* outSiteTotals,
                            double* outBranchTotals, double* outTables);
/* Unconditioned counts: one unconditional Gillespie history per (length row l, site s) of a chain with stateCount (2..64) states —
 * StateHistory.simulateUnconditionalOnEndingState (StateHistory.java:324-354) as CodonPartitionedRobustCounting
 * .fillInUnconditionalTraitValues uses it (CodonPartitionedRobustCounting.java:619-647).  `instance` only names the device and the
 * stream: nothing of the instance is read.  lengthCount = 1 with the expected tree length gives the u_ column per site; lengthCount =
 * nodeCount with each branch's length is doUnconditionedPerBranch.  forceUnconditionalAverageRate needs nothing here: the caller
 * passes the averaged chain's Q and frequencies.
 *   infinitesimalMatrix Q [S][S] row-major, startFrequencies [S], lengths [lengthCount] (each finite and >= 0), registers [K][S][S].
 * The history: cur = a draw from startFrequencies; t = 0; while t < length: rate = -Q[cur][cur]; a state with rate <= 0 ends the
 * history; t = t + (-1.0 * log(1 - u)) / rate (MathUtils.nextExponential); if still t < length, next = a draw from Q's row cur with
 * its own entry set to 0, register k adds R_k[cur][next], cur = next.  The value of register k is that sum over the jumps in time
 * order from 0.0 — for the reference's 0/1 registers it equals getTotalRegisteredCounts.  Both draws are randomChoicePDF as
 * beagleMi355SampleAncestralStates restates it (U = u * total, the fall-through rule included).  Length 0: all values 0.
 * Random numbers (stateless): the history of (l, s) has the stream z = SplitMix64's output for key l * siteCount + s from the state
 * seed ^ 0xBB67AE8584CAA73B, as a 64-bit integer; u_q = SplitMix64's (q + 1)-th output from state z as (x >> 11) * 2^-53; u_0 draws
 * the start state, u_(2m+1) waiting time m, u_(2m+2) the state after it.
 *   outCounts [K][lengthCount][siteCount] or NULL;  outTotals [K][lengthCount] or NULL = the sum over the sites in the fixed order of
 *   beagleMi355RobustCounts' outBranchTotals.  Not both NULL.  The bits depend on the seed alone.
 * A history is cut after 100 000 jumps (a caller's Q x length that would never finish): its value is what it had, everything else is
 * written, and the call returns BEAGLE_ERROR_FLOATING_POINT — as it does when a draw's total weight is not finite and > 0.
 * BEAGLE_ERROR_OUT_OF_RANGE for a NULL input, stateCount outside 2..64, registerCount outside 1..8, a Q or length that is not finite,
 * a negative length, lengthCount or siteCount below 1, or both outputs NULL; BEAGLE_ERROR_NO_IMPLEMENTATION on the sharded handle.
 * An extension: no BEAST class calls it today. */
int beagleMi355SimulateUnconditionedCounts(int instance, int stateCount, const double* infinitesimalMatrix,
                                           const double* startFrequencies, const double* lengths, int lengthCount, int siteCount,
                                           const double* registers, int registerCount, unsigned long long seed, double* outCounts,
                                           double* outTotals);
/* Complete histories: ONE call that simulates a substitution history on every branch, down the tree — what
 * dr.app.beagle.tools.CompleteHistorySimulator.simulate computes with one StateHistory.simulateUnconditionalOnEndingState per (branch,
 * site) in Java (CompleteHistorySimulator.java:384-496, StateHistory.java:324-354): the history on a branch starts from the parent's
 * realised state, its ending state is the child's state, and every registered jump process keeps its realised value per (branch, site).
 * It reads the instance's state count, the category rates, category weights and state frequencies at the given indices and nothing
 * else: no matrices, no partials, no patterns — siteCount is free, updatePartials and updateTransitionMatrices need never have been
 * called, a partitioned instance is served like any other, and the instance is left exactly as found.
 *   nodes: nodeCount triples {outRow, qIndex, parentRow} in pre-order — row 0 is the root {outRow, ignored, -1}, every other row names
 *          the generator it evolves under (0 .. qCount-1) and a parentRow smaller than its own index.  outRow as in
 *          beagleMi355SimulateSequences: the row of outStates that receives the node's states, -1 for "not wanted", every value >= 0 at
 *          most once.
 *   branchLengths [nodeCount]: the operational time of row r's branch = branch rate x height difference (:483-486); finite, >= 0; row 0
 *          is ignored.  nodeHeights [nodeCount] or NULL: only read for outEventHeights.
 *   infinitesimalMatrices [qCount][S][S] row-major, qCount >= 1, every entry finite: one generator for the whole tree is qCount = 1, the
 *          reference's branchSpecificLambda one generator per distinct branch value.
 *   registers [registerCount][S][S], registerCount 1..8; registerFlags[k] (NULL: all 0) = BEAGLE_MI355_JUMPS_REWARDS for a reward
 *          register, no other bit (the reference parses scaleByTime and ignores it, :286).
 *   flags: none is defined; it must be 0.  inRootStates, inRateCategories (NULL: drawn): as in beagleMi355SimulateSequences.
 * The rule.  Category c of site s: inRateCategories[s], else (categoryCount > 1) a draw from the category weights, else 0.  Root state:
 * inRootStates[s], else a draw from the state frequencies.  Row r >= 1: tau = rate_c * branchLengths[r], cur = the parent's state at the
 * site, t = 0.0; while t < tau: rate = -Q[cur][cur]; a state with rate <= 0 ends the history; t = t + (-1.0 * log(1 - u)) / rate
 * (MathUtils.nextExponential); if still t < tau, next = a draw from Q's row cur with its own entry taken as 0 — a jump cur -> next at t —
 * and cur = next.  The child's state is cur.  tau = 0 (a zero-length branch, a zero-rate category): no jump, the parent's state.
 * A draw over w_0 .. w_{n-1} is MathUtils.randomChoicePDF in its CUMULATIVE form: cum_i = cum_{i-1} + w_i from cum_{-1} = 0.0 in index
 * order (one IEEE addition each), total = cum_{n-1}, U = u * total, the result is the first i with U < cum_i, and where there is none
 * THE LARGEST INDEX WITH w_i > 0.  (The subtract-and-test walk of beagleMi355SampleAncestralStates agrees with it except where the two
 * roundings differ in the last bit; this call and its host restatement both use the cumulative form.)  A total that is not finite
 * and > 0: the root state or category is 0, a history ends where it is, everything else is written and the call returns
 * BEAGLE_ERROR_FLOATING_POINT.  A history is cut after 100 000 jumps: the state at the cut is the child's state, its values are what
 * they had reached (a reward gets no final term), everything else is written and the call returns BEAGLE_ERROR_FLOATING_POINT.
 * Register k of (row r, site s), summed over the history in time order from 0.0: a count register adds R_k[from][to] per jump — with
 * integer entries (the reference's 0/1 registers) getTotalRegisteredCounts exactly; a reward register adds R_k[cur][cur] * (t - t_prev)
 * per jump and R_k[cur][cur] * (tau - t_last) at the end (beagleMi355SampleMarkovJumpsUniformized's definition; getTotalReward up to
 * the order of the additions).  Every product is rounded on its own (no fused multiply-add).
 * Random numbers (stateless): the history of (row r, site s of the whole call) has the stream z = SplitMix64's output for key
 * r * siteCount + s from the state seed ^ 0x3C6EF372FE94F82B, as a 64-bit integer; u_q = SplitMix64's (q + 1)-th output from state z as
 * (x >> 11) * 2^-53.  Row 0: u_0 draws the root state, u_1 the category.  Row r >= 1: u_(2m) is waiting time m, u_(2m+1) the state
 * after it.  The bytes depend on the seed alone: not on the launch shape, not on the chunks the sites are processed in
 * (BEAGLE_MI355_HIST_CHUNK_SITES=<n> overrides their size, rounded up to a multiple of 256), not on the number of GPUs.
 * Outputs (each may be NULL, not all of them; asking for fewer does not change the bits of the others):
 *   outStates [1 + max outRow][siteCount] bytes, outRateCategories [siteCount]: as in beagleMi355SimulateSequences;
 *   outValues [K][nodeCount][siteCount], row 0 all zero;
 *   outRowTotals [K][nodeCount] = the sum over the sites (the reference's sumAcrossSites) in the fixed order of
 *          beagleMi355RobustCounts' outBranchTotals: per block of 256 consecutive sites a wave's 64 by an xor-shuffle tree (distances
 *          32 .. 1), the four waves in wave order, then the blocks in ascending order; row 0: 0;
 *   outSiteTotals [K][siteCount] = the sum over rows 1 .. nodeCount-1 in row order from 0.0.
 * Events, when any of outEventCounts, outEventHeights, outEventStates, outEventTotal is not NULL: outEventCounts [nodeCount][siteCount]
 * = the jumps of every history; the events are ordered by site, then row, then time; outEventStates[2e], [2e+1] = event e's from and to
 * states; outEventHeights[e] = h_parent + (t / tau) * (h_child - h_parent) (needs nodeHeights); *outEventTotal is always written.  More
 * events than eventCapacity: no event is written, everything else is, and the call returns BEAGLE_ERROR_OUT_OF_RANGE — a second call
 * with a buffer of *outEventTotal events is exact, because the streams are keyed.
 * The sharded handle (resource G+1) splits the SITES into contiguous ranges; every shard gets everything else.  States, categories,
 * values, site totals, event counts and events come back byte for byte as from one instance (a shard's events follow the earlier
 * shards'); the row totals are the shards' sums — each in the order above, its blocks counted from its first site — added in shard order.
 * BEAGLE_ERROR_OUT_OF_RANGE for a NULL nodes, branchLengths, infinitesimalMatrices or registers, nodeCount, siteCount or qCount below 1,
 * a bad rates, weights or frequencies index, a qIndex outside 0..qCount-1, a parent row that is not earlier than the row itself, an
 * outRow below -1 or used twice, a Q or length that is not finite, a negative length, an unknown register-flag bit, registerCount
 * outside 1..8, non-zero flags, an input state >= stateCount or category outside 0..categoryCount-1, outEventHeights without
 * nodeHeights, a negative eventCapacity, all outputs NULL; BEAGLE_ERROR_NO_IMPLEMENTATION for a state count outside 2..64 and on a
 * BASTA instance.  An extension: no BEAST class calls it today. */
int beagleMi355SimulateCompleteHistories(int instance, const int* nodes, int nodeCount, int siteCount, const double* branchLengths,
                                         const double* nodeHeights, const double* infinitesimalMatrices, int qCount,
                                         int categoryRatesIndex, int categoryWeightsIndex, int stateFrequenciesIndex,
                                         const double* registers, const int* registerFlags, int registerCount, unsigned long long seed,
                                         int flags, const unsigned char* inRootStates, const int* inRateCategories,
                                         unsigned char* outStates, int* outRateCategories, double* outValues, double* outRowTotals,
                                         double* outSiteTotals, int* outEventCounts, long long eventCapacity, double* outEventHeights,
                                         unsigned char* outEventStates, long long* outEventTotal);
/* Tip error models (SequenceErrorModel, HypermutantErrorModel, ambiguity codes): a tip whose partials are a LOOKUP.
 *   codes [patternCount]: the observed code of every pattern; a code outside 0..codeCount-1 is missing (all ones, a factor of one).
 *   emission [codeCount][stateCount]: emission[k * S + i] = the tip's partial for true state i at a pattern whose code is k.
 * The tip's partials are partials[c][p][i] = emission[codes[p]][i] in every category — what beagleSetTipPartials would have been given.
 * codes == NULL keeps the codes of the previous call and replaces the table (codeCount as in that call): the per-proposal call, codeCount * S
 * doubles through the pinned staging ring.  With codes the call does for the tip what beagleSetTipStates does, on the codes.
 * codeCount <= S: the tip stays a compact tip and every operation list that names it reads, instead of its branch matrix M, the
 * product shadow[c][i][k] = sum_j M[c][i][j] * emission[k][j] (j ascending, no fused multiply-add; columns k >= codeCount zero), which
 * one small launch in front of the list writes into a slot of the engine's own — on every beagleUpdatePartials[ByPartition] call, since
 * the matrix or the table may have changed.  codeCount > S, a list that uses one matrix index for such a tip and for another child, and
 * every call that reads a tip's partials as data (beagleUpdatePrePartials[ByPartition], the edge and cross-product differentials,
 * beagleMi355SampleAncestralStates, both Markov-jump calls, beagleMi355NodeHeightDerivatives: every such tip; beagleGetPartials, ...Batch,
 * ...Pinned: that tip) have the device write the partials buffer out from codes and table: from then on the tip is what
 * beagleSetTipPartials leaves behind, written again whenever its table changes, until a call with codes chooses again.
 * beagleGetTipStates returns the codes (one outside the table: codeCount).  A later beagleSetTipStates, beagleSetTipPartials or
 * beagleSetPartials on the tip drops the emission.  One emission per tip for the whole instance, whatever its pattern partitions.
 * The sharded handle splits the codes by pattern and gives every shard the table.
 * Errors: BEAGLE_ERROR_OUT_OF_RANGE for codeCount outside 1..255, a bad tip index, emission NULL, codes NULL on a tip without codes or
 * with another codeCount than they came with; BEAGLE_ERROR_NO_IMPLEMENTATION on a BASTA instance. */
int beagleMi355SetTipEmission(int instance, int tipIndex, const int* codes, int codeCount, const double* emission);
/* out4 = {tips folded into their branch matrices now, tips written out as partials now, fold launches since creation, tips turned from
 * the first kind into the second since creation} (shard 0 of a sharded handle). */
int beagleMi355TipEmissionStats(int instance, long* out4);
/* For the JNI shim: getPartials / getSiteLogLikelihoods whose result STAYS in the engine's pinned host buffer — *outPinned,
 * *outCount doubles, valid until the next call on the instance — so that it reaches the Java array with one copy
 * (Set<Type>ArrayRegion) instead of two.  BEAGLE_ERROR_NO_IMPLEMENTATION on the sharded instance: use the ordinary call. */
int beagleMi355GetPartialsPinned(int instance, int bufferIndex, int scaleIndex, const double** outPinned, long* outCount);
int beagleMi355GetSiteLogLikelihoodsPinned(int instance, const double** outPinned, long* outCount);
/* Block until everything enqueued for the instance has completed. */
int beagleMi355Synchronize(int instance);
/* Engine-side timing of the hot kernel: HIP events recorded on the instance's stream around
 * the pruning launches of every updatePartials call while enabled; returns accumulated milliseconds and the
 * number of launches since the last reset. */
int beagleMi355KernelTimer(int instance, int enable, double* outMillis, long* outLaunches);
/* enable = N > 1 brackets every N-th updatePartials call only (an event pair costs the stream two barrier packets, ~12 us of
 * an evaluation): milliseconds and launches then cover those calls; beagleMi355KernelTimerCalls returns how many updatePartials
 * calls were bracketed since it was last asked (and resets the count) — the divisor for "kernel time per evaluation". */
int beagleMi355KernelTimerCalls(int instance, long* outCalls);
/* How many calculateRootLogLikelihoods calls of this instance (shard 0 of a sharded handle) were answered by the pattern walk itself —
 * a one-launch walk of an unpartitioned 4-state instance is held back until the next call, and when that call asks for the root
 * log-likelihood of the walk's last result the slice that computes it finishes the evaluation (no root kernel, no read-back of
 * the root's partials).  BEAGLE_MI355_NO_ROOT_FUSION=1 switches the holding off.  Since instance creation. */
int beagleMi355RootFusedCount(int instance, long* outCount);
/* beagleGetSiteLogLikelihoods (and its pinned form below) calls since instance creation that found the site values ALREADY ON THE HOST: a
 * caller that reads them after every whole-alignment root sum — BeagleTreeLikelihood.java:1050 does — has them sent to a pinned buffer right
 * behind the root's kernel, before it asks (two such reads in a row switch it on, a sum nobody reads the values of switches it off;
 * the values are those of the stream-ordered download, bit for bit).  BEAGLE_MI355_NO_SITE_PREFETCH=1 at creation: never. */
int beagleMi355SitePrefetchCount(int instance, long* outCount);
/* Forget what the (enabled) kernel timer and the walk counters have gathered so far — no synchronisation, no allocation: for a
 * caller that has just synchronised the stream itself and wants the measurement to start here (bench.py: between its warm-up
 * and its timed steps, without giving the device an idle gap to drop its clocks in). */
int beagleMi355KernelTimerRestart(int instance);
/* Traffic counters of the 4-state pattern walk since the last beagleMi355KernelTimer call: out[0] micro-operations,
 * [1] partials buffers stored, [2] partials buffers read from memory, [3] tip-state vectors read, [4] scale-factor
 * vectors read, [5] walk launches, [6] scale-factor vectors written, [7] walk launches that ran the assembly loop.  bench.py turns them into the
 * bytes the design has to move (roofline.achieved). */
int beagleMi355WalkStats(int instance, long* out8);
/* The one-launch pattern walk (4 states) since instance creation.  out[0]: workgroups whose wait for the slices they read from ran
 * out and that computed those slices themselves (kernels_walk4.hip: the launch cannot deadlock whatever order the hardware
 * dispatches workgroups in; on gfx950 the count stays 0); out[1]: that wait's limit in microseconds (BEAGLE_MI355_WALK_SPIN_US at
 * creation, default 20 000); out[2]: folded reciprocal vectors in use by read-mode programs (one per stored node instead of one
 * per node: DESIGN.md 4.1); out[3]: how many times such vectors were (re)built from the per-node factors. */
int beagleMi355WalkHealth(int instance, long* out4);
/* Repeated sub-patterns (4 states): clades of compact tips evaluated once per distinct sub-pattern.  Since the last
 * beagleMi355KernelTimer / KernelTimerRestart call — out[0]: class rows evaluated (a micro-operation of a class-table program over
 * a clade of D classes counts D; divided by the pattern count: full-width micro-operations), out[1]: operands read from a class
 * table, out[2]: class-table programs run (clades, counted per evaluation).  Since creation — out[3]: bytes of the table arena and
 * of the tables' row vectors and representative tip rows, out[4]: clades indexed on the host, out[5]: host microseconds spent on
 * indices and tables.  Since the last timer call again — out[6]: micro-operations with BOTH children read from class tables, out[7]:
 * table operands of micro-operations that are not stored themselves (steps of a memory definition).  Since creation — out[8]: bytes
 * of host memory the class indices take, out[9]: times they were dropped at their capacity (a chain of topology moves).  All zero where
 * the feature is off (BEAGLE_MI355_NO_REPEATS=1, small buffers, write-mode evaluations). */
int beagleMi355RepeatStats(int instance, long* out10);
/* ... and of those class-table programs the SUB-RUNS: plain clades inside a definition that cannot be taken from a table as a whole — the
 * clades hanging off the path of a memory definition that is evaluated from memory (DESIGN.md 4.1 "Tables inside memory definitions").
 * Since the last beagleMi355KernelTimer / KernelTimerRestart call — out[0]: sub-runs taken, counted per evaluation (they are among
 * beagleMi355RepeatStats' out[2]), out[1]: the full-width micro-operations they took out of the walk.  Both zero with
 * BEAGLE_MI355_NO_MEMDEF_TABLES=1 and wherever beagleMi355RepeatStats reports zeros. */
int beagleMi355RepeatSubRunStats(int instance, long* out2);
/* Class-table operands as the device programs of the assembly loop read them (4 states), since the last beagleMi355KernelTimer /
 * KernelTimerRestart call — out[0]: micro-operations whose FIRST child is read from a class table, out[1]: those that come directly
 * behind a micro-operation whose own first child is read from memory, out[2]: those directly behind a micro-operation with a fused
 * cherry (the two neighbours whose loads lie between a table child's class ids and its rows), out[3]: the largest class count of a
 * table read.  All zero where the feature is off or another kernel runs the programs. */
int beagleMi355TableOperandStats(int instance, long* out4);
/* How the one-launch walks of a 4-state instance were run since its creation: out[0] launches on TICKETS (the program's slices form
 * a forest: only the slices without dependencies get workgroups, the workgroup that arrives last at a slice above runs it — nobody
 * waits; the default), out[1] launches on dependency FLAGS (every slice its own workgroups, which poll: programs whose slices do not
 * form a forest, or BEAGLE_MI355_NO_WALK_TICKETS=1), out[2] / out[3]: slices with workgroups of their own / slices in all, last launch;
 * out[4]: micro-operations that were not part of a device program because their consumer evaluated them inside its own stage (nodes over
 * two compact tips: DESIGN.md 4.1 "fused cherries"; BEAGLE_MI355_NO_CHERRY_FUSION=1: none), out[5]: micro-operations planned, both since
 * the last beagleMi355KernelTimer call; out[6]: accumulateScaleFactors calls since creation that were answered from the per-slice products of
 * factors a write-mode walk had just left behind (BEAGLE_MI355_NO_SLICE_SUMS=1: none); out[7]: calculateRootLogLikelihoodsByPartition
 * calls since creation that the top slices of the partitions finished inside the walk's own launch (4 states, up to eight partitions;
 * BEAGLE_MI355_NO_ROOT_PARTS_FUSION=1: none).  out8 holds eight values. */
int beagleMi355WalkLaunchInfo(int instance, long* out8);
/* The gradient pass (4 states) since instance creation.  A pre-order list without scale indices is held back until a call needs
 * what it writes (or changes what it reads): out[0] lists that ran together with the edge derivatives that followed them (one
 * sweep per tree level; sums and sums of squares), out[1] lists that ran operation by operation, out[2] edge-derivative calls
 * answered from a held list WITHOUT writing a pre-order partial (sums only; the list stays held), out[3] held lists that had
 * to run after all because a later call touched their buffers. */
int beagleMi355GradientStats(int instance, long* out4);
/* The instance's dimensions, for wrappers that have to size what a whole-array output defines (the JNI shim):
 * out8 = {tipCount, partialsBufferCount, stateCount, patternCount, categoryCount, matrixBufferCount, scaleBufferCount, partitionCount}. */
int beagleMi355GetDimensions(int instance, int* out8);
/* Bytes of HBM currently allocated by the instance. */
long beagleMi355DeviceBytes(int instance);

/* ---- BASTA: the structured-coalescent approximation (beagle/basta/BastaJNIWrapper.java; the natives
 * BeagleBastaLikelihoodDelegate calls on an ordinary instance).  The arithmetic restates the reference's pure-Java twin,
 * GenericBastaLikelihoodDelegate.peelPartials / reduceWithinInterval / reduceAcrossIntervals.
 *
 * A BASTA instance has patternCount 1 and categoryCount 1 (anything else: BEAGLE_ERROR_NO_IMPLEMENTATION from every call below,
 * as on the sharded handle, and as from every other call below before the first AllocateCoalescentBuffers).  A "partial" is S
 * doubles.  Once an instance has BASTA buffers, beagleSetPartials / beagleGetPartials (scale index ignored) address THEM: S
 * doubles in, S doubles out.  Population sizes travel through beagleSetStateFrequencies(populationSizesIndex, sizes) and are
 * stored as given; matrices through beagleUpdateTransitionMatrices / beagleSetTransitionMatrix as ever.
 * BEAGLE_ERROR_OUT_OF_RANGE for an index outside the allocation, a negative in1, an interval number >= maxCoalescentIntervalCount,
 * intervals that do not start at 0, decrease, or do not end at operationCount.
 *
 * (Re)size the instance's BASTA state: partialsBufferCount vectors and coalescentBufferCount (5: probabilities, e, f, g, h)
 * interval-indexed buffers.  initial != 0: everything zero.  initial == 0 (the caller's buffer numbers outgrew the allocation):
 * the vectors stored so far are kept.  threadCount is ignored. */
int beagleBastaAllocateCoalescentBuffers(int instance, int coalescentBufferCount, int maxCoalescentIntervalCount,
                                         int partialsBufferCount, int initial, int threadCount);
/* operations: operationCount tuples {dest, in1, matrix1, in2, matrix2, acc1, acc2, intervalNumber}; intervals: intervalCount offsets
 * into the list, the first 0 and the last operationCount (intervalCount - 1 intervals).  Per operation left = M1 p[in1]; with
 * in2 < 0, p[dest] = left; otherwise right = M2 p[in2], entry_i = left_i right_i / size_i, prob = sum_i entry_i, p[dest] = entry / prob,
 * p[acc1] = left, p[acc2] = right, probabilities[intervalNumber] = prob.  The probabilities are zeroed first.  Operations of one
 * interval are independent; an operation may read what an earlier interval wrote.  The number of kernel launches does not depend
 * on the number of intervals when every vector the list writes is written once and read by one operation of a later interval
 * (the reference's numbering); any other list runs one launch per interval.  Returns when the work is enqueued. */
int beagleBastaUpdatePartials(int instance, const int* operations, int operationCount, const int* intervals, int intervalCount,
                              int populationSizesIndex, int coalescentProbabilityIndex);
/* Per interval k (its number n = the interval number of its first operation): e, f, g, h [n] = sums over its operations, in list order,
 * and their one or two children of p[in], p[in]^2, p[acc], p[acc]^2 per state; sum = sum_s (e_s^2 - f_s + g_s^2 - h_s) / size_s;
 * logL_k = -intervalLengths[k] sum / 4 + (probabilities[n] != 0 ? log probabilities[n] : 0).  outLogLikelihood[0] += sum_k logL_k,
 * the terms added in a fixed order (two calls give the same bits).  Needs coalescentBufferCount >= 5.  A list equal to the one the
 * device already holds (the usual case: the list just given to beagleBastaUpdatePartials) is not uploaded again.
 * BEAGLE_ERROR_FLOATING_POINT when the sum is NaN (outLogLikelihood untouched). */
int beagleBastaAccumulatePartials(int instance, const int* operations, int operationCount, const int* intervals, int intervalCount,
                                  const double* intervalLengths, int populationSizesIndex, int coalescentProbabilityIndex,
                                  double* outLogLikelihood);
/* Buffer `index` of the coalescent buffers: the one that held the probabilities in the last update (index 0 before any) as
 * maxCoalescentIntervalCount doubles, any other as [maxCoalescentIntervalCount][S] doubles; beagleBastaGetBufferLength says which. */
int beagleBastaGetBuffer(int instance, int index, double* out);
int beagleBastaGetBufferLength(int instance, int index);
/* out4 = {uploads of an operation list so far, updates run as one launch, updates run interval by interval, partialsBufferCount}. */
int beagleBastaStats(int instance, long* out4);
/* Draw a deme for every lineage at every sub-interval boundary, replicateCount times, in one call (an extension: BastaJNIWrapper has no
 * native for it; what BastaLikelihood.traverseSampleByCoalescentIntervals computes from one getPartials and one getTransitionMatrices per
 * branch-interval operation, BastaLikelihood.java:755-943).  operations / intervals: the list of beagleBastaUpdatePartials, staged and
 * compared as beagleBastaAccumulatePartials does it (a list equal to the resident one is not uploaded again).  The vectors and matrices
 * are read as they stand: call beagleBastaUpdatePartials first.
 *
 * The rule.  A vector nothing in the list reads is a ROOT (the reference's lists have one: `dest` of the last operation); its state is
 * drawn from the weights p[root]_i f_i, f = the frequencies at stateFrequenciesIndex.  Then the operations are visited from the last
 * interval to the first.  With s the state already drawn for the operation's `dest`, each input (in1 with matrix1, and in2 with matrix2
 * when in2 >= 0) gets a state drawn from
 *     w_j = M[s][j] p[in]_j,      M the matrix as stored (as beagleGetTransitionMatrix returns it):
 * the S terms whose sum beagleBastaUpdatePartials forms as left_s / right_s, so the draw is the exact conditional under the approximation
 * the likelihood itself makes; at a coalescence the two children are drawn independently given s.  THIS ORIENTATION IS THE DEFAULT: it is
 * the one consistent with the likelihood, and what the reference's node-by-node route computes from the untransposed exp(Qt)
 * (BastaLikelihood.java:1036-1038, 1086-1091).  The reference's interval-by-interval route indexes the stored (transposed) matrix the
 * other way round (:938), which differs for an asymmetric Q; BEAGLE_MI355_BASTA_STATES_AS_WRITTEN selects that reading,
 *     w_j = M[j][s] p[in]_j,
 * so that a literal restatement of :911-943 can be compared bit for bit.
 * Fixed tips: an input vector with exactly one positive entry gives that entry's index without a draw (:846-867, applied to any input).
 * Draws: randomChoicePDF's rule with U = u * total, the largest index of a positive weight when rounding lets the walk fall through, as
 * beagleMi355SampleAncestralStates; BEAGLE_MI355_ANCESTRAL_MAP: the first index of the strict maximum instead.  The uniform of vector b
 * in replicate r is the (b + 1)-th output of the SplitMix64 stream whose state is the (r + 1)-th output of the stream of `seed`, its top
 * 53 bits: a state depends on the seed, the replicate and the buffer number only, not on how the call is cut into launches.
 *
 * Outputs (each may be NULL, not all):
 *   outStates    [replicateCount][partialsBufferCount]: the state of every vector, 255 for one the list neither reads nor writes; acc1 /
 *                acc2 of a coalescence get the state of the input they were formed from.  Copied out in chunks of replicates.
 *   outOccupancy [intervalCount - 1][S]: over all replicates, the number of input vectors of interval k's operations in state i
 *                (lineages per deme at the young end of the interval).
 *   outChanges   [S][S]: over all replicates and all inputs, the number with `dest` state a and input state b.
 * Both count arrays are integer sums (64-bit on the device) returned as doubles: exact, whatever the order.
 * The number of launches is the depth of the list in coalescences (beagleBastaStatesStats), per chunk of replicates.
 * BEAGLE_ERROR_NO_IMPLEMENTATION: the sharded handle, an instance without BASTA buffers, a list in which a vector is written twice, read
 * by two operations, or read in the interval that writes it.  BEAGLE_ERROR_OUT_OF_RANGE: replicateCount < 1, a bad index, unknown flag
 * bits, S > 255, no output.  BEAGLE_ERROR_FLOATING_POINT: a draw met a total that is not finite and positive; the outputs are still
 * written, with state 0 there. */
#define BEAGLE_MI355_BASTA_STATES_AS_WRITTEN 2
int beagleBastaSampleStates(int instance, const int* operations, int operationCount, const int* intervals, int intervalCount,
                            int stateFrequenciesIndex, int replicateCount, unsigned long long seed, int flags,
                            unsigned char* outStates, double* outOccupancy, double* outChanges);
/* out4 = {beagleBastaSampleStates calls so far, kernel launches of the last one per chunk of replicates (its depth in coalescences),
 * chunks of replicates of the last one, chains of the last one}. */
int beagleBastaStatesStats(int instance, long* out4);
/* The gradient of the log-density beagleBastaAccumulatePartials returns, with respect to the migration rates and the population sizes, in
 * one call (an extension, as beagleBastaSampleStates: the reference does not define what BastaJNIWrapper's gradient natives compute — its
 * GRADIENT-mode reduction calls the likelihood native — but it does pin the arithmetic of the pure-Java delegate,
 * GenericBastaLikelihoodDelegate.peelPartialsGrad :443-534, peelPopSizeSGrad :536-603, reduceWithinIntervalGrad :680-753,
 * reduceAcrossIntervalsGrad / ...GradPopSize :622-678).  The Java code carries S^2 tangent vectors per buffer forwards, O(N S^4); the same
 * numbers come out of ONE adjoint sweep at the cost of a likelihood, O(N S^2), and that is what this call runs.  It reads the vectors,
 * matrices and coalescent probabilities as beagleBastaUpdatePartials of the same list left them, forms e, f, g, h itself (as
 * beagleBastaAccumulatePartials does: beagleBastaGetBuffer reads the same afterwards), and uploads no list that is already resident.
 *
 * The rule.  For an operation {dest, in1, m1, in2, m2, acc1, acc2, number} of list interval k: V[x] the stored vector of buffer x,
 * theta_i = 1 / size_i, J = probabilities[number], len_k = intervalLengths[k], t_k = intervalDistances[k] (the rate-scaled length the
 * interval's matrices were formed with, TransitionMatrixOperation.time), e and g the sums of the interval's start and end vectors as
 * beagleBastaAccumulatePartials forms them.  For a one-input operation acc1 == dest, so "the end vector of side 0" is V[acc1] in both
 * kinds of operation.  The log-density is
 *     L = sum_k [ -len_k / 4 sum_i (e_i^2 - f_i + g_i^2 - h_i) theta_i + log J_k ].
 * Lambda[x] = dL / dV[x] with every buffer treated as free.  With c_k = (-len_k / 2) theta (a vector), walking the list in reverse:
 *     start vectors (in1, in2) receive the direct term  c_k (e_k - V[x]),   end vectors (acc1, acc2)  c_k (g_k - V[x]);
 *     one-input operation:  Lambda[dest] = (what its reader left, 0 for a root) + the end term;
 *                           Lambda[in1]  = M1^T Lambda[dest] + the start term;
 *     coalescence:          w = ((Lambda[dest] - <Lambda[dest], V[dest]>) + 1) / J        (Lambda[dest]: what its reader left, 0 for a root)
 *                           Lambda[acc1] = (w V[acc2]) theta + the end term,   Lambda[acc2] = (w V[acc1]) theta + the end term,
 *                           Lambda[in1]  = M1^T Lambda[acc1] + the start term,  Lambda[in2] = M2^T Lambda[acc2] + the start term.
 * (M^T x)_j = sum_i M[i][j] x_i and <x, y> = sum_i x_i y_i run in index order from 0; products are rounded before they are added (no
 * fused multiply-add), so Lambda is a function of the inputs alone, bit for bit.  The outputs:
 *     outPopulationSizes [S], with respect to theta (the reference's intermediate; d/dN_a = -G_a / N_a^2 is the caller's chain rule):
 *         G[a] = sum_k ( (-len_k / 4) (((e^2 - f) + g^2) - h)_{k,a} + sum over the interval's coalescences of (w_a V[acc1]_a) V[acc2]_a )
 *     outMigration [S * S], row-major a * S + b, the reference's first-order form dP ~ t P E_ab (for the stored, transposed matrices:
 *         row b += t * row a):      W[a][b] = sum_k sum over the interval's operations and their sides of (t_k V[acc]_a) Lambda[acc]_b
 *     outAdjoints [partialsBufferCount * S]: Lambda, 0 for a buffer the list does not touch.
 * Inside an interval the operations are added in list order (side 0 before side 1), then the intervals in index order
 * from 0: the same bits on every call, whatever the launch geometry.
 * The chain rule to the rates (StructuredCoalescentLikelihoodGradient.java:134-154) is the caller's too.
 *
 * Two defects of the reference are NOT part of the contract.  MigrationRateGradientDispatch.clearStorage is empty (:274) while
 * peelPartialsGrad accumulates with += into stale storage (:508), so a second Java call returns other numbers: the contract is what a
 * FIRST call on zeroed storage computes.  And `sizesOffset *= sizesOffset * stateCount` (:496, :570) is 0 for the only offset ever
 * passed (0), which is what is restated.
 *
 * intervalDistances may be NULL when outMigration is NULL.  Each output may be NULL, not all.  flags: none defined, pass 0.
 * Kernel launches: one per level of coalescences plus four (e-h and their total, the two reductions); beagleBastaGradientStats.
 * BEAGLE_ERROR_NO_IMPLEMENTATION: the sharded handle, an instance without BASTA buffers, more than 256 states, a list
 * beagleBastaSampleStates refuses.  BEAGLE_ERROR_OUT_OF_RANGE: a bad index, no operation, no output, no lengths, unknown flag bits,
 * coalescentBufferCount < 5.  BEAGLE_ERROR_FLOATING_POINT: a returned value is not finite (a coalescence with J = 0); the outputs are
 * written then too, and in no other case but success. */
int beagleBastaGradient(int instance, const int* operations, int operationCount, const int* intervals, int intervalCount,
                        const double* intervalLengths, const double* intervalDistances, int populationSizesIndex,
                        int coalescentProbabilityIndex, int flags, double* outPopulationSizes, double* outMigration, double* outAdjoints);
/* out4 = {beagleBastaGradient calls so far, kernel launches of the last one, its levels of coalescences, its chains}. */
int beagleBastaGradientStats(int instance, long* out4);
/* The gradient natives of BastaJNIWrapper: not built, BEAGLE_ERROR_NO_IMPLEMENTATION (the gradient: beagleBastaGradient). */
int beagleBastaUpdatePartialsGrad(int instance, const int* operations, int operationCount, const int* intervals, int intervalCount,
                                  int populationSizesIndex, int coalescentProbabilityIndex);
int beagleBastaUpdateTransitionMatricesGrad(int instance, const int* transitionMatrixIndices, const double* branchLengths, int count);
int beagleBastaAccumulatePartialsGrad(int instance, const int* operations, int operationCount, const int* intervals, int intervalCount,
                                      const double* intervalLengths, int populationSizesIndex, int coalescentProbabilityIndex,
                                      double* outGradient);

/* Function table: lets a host driver (host/tree_likelihood.cpp) or a test drive any engine
 * that implements this ABI (the HIP engine, or the CPU oracle under oracle/) through one type. */
typedef struct BeagleApi {
    const char* (*getVersion)(void);
    int (*createInstance)(int, int, int, int, int, int, int, int, int, const int*, int, long, long, BeagleInstanceDetails*);
    int (*finalizeInstance)(int);
    int (*setPatternWeights)(int, const double*);
    int (*setTipStates)(int, int, const int*);
    int (*setTipPartials)(int, int, const double*);
    int (*setPartials)(int, int, const double*);
    int (*getPartials)(int, int, int, double*);
    int (*getLogScaleFactors)(int, int, double*);
    int (*setEigenDecomposition)(int, int, const double*, const double*, const double*);
    int (*setStateFrequencies)(int, int, const double*);
    int (*setCategoryWeights)(int, int, const double*);
    int (*setCategoryRates)(int, const double*);
    int (*setTransitionMatrix)(int, int, const double*, double);
    int (*getTransitionMatrix)(int, int, double*);
    int (*updateTransitionMatrices)(int, int, const int*, const int*, const int*, const double*, int);
    int (*updatePartials)(int, const int*, int, int);
    int (*accumulateScaleFactors)(int, const int*, int, int);
    int (*removeScaleFactors)(int, const int*, int, int);
    int (*resetScaleFactors)(int, int);
    int (*copyScaleFactors)(int, int, int);
    int (*calculateRootLogLikelihoods)(int, const int*, const int*, const int*, const int*, int, double*);
    int (*getSiteLogLikelihoods)(int, double*);
    /* optional (NULL when the engine has no device memory): beagleMi355CalculateRootLogLikelihoodsDevice */
    int (*calculateRootLogLikelihoodsDevice)(int, int, int, int, int, void*);
    /* optional (NULL without a communicator layer): beagleMi355CalculateRootLogLikelihoodsAllReduce */
    int (*calculateRootLogLikelihoodsAllReduce)(int, int, int, int, int, double*);
} BeagleApi;

const BeagleApi* beagleGetApiTable(void);

/* The calls of a PARTITIONED instance's evaluation (MultiPartitionDataLikelihoodDelegate.java:800-1083), for a native caller that is
 * handed a table instead of linking the library (tools/host: the multi-partition call sequence in C++, as the single-partition one). */
typedef struct BeaglePartitionApi {
    int (*setCategoryRatesWithIndex)(int, int, const double*);
    int (*updateTransitionMatricesWithMultipleModels)(int, const int*, const int*, const int*, const int*, const int*, const double*, int);
    int (*updatePartialsByPartition)(int, const int*, int);
    int (*resetScaleFactorsByPartition)(int, int, int);
    int (*accumulateScaleFactorsByPartition)(int, const int*, int, int, int);
    int (*calculateRootLogLikelihoodsByPartition)(int, const int*, const int*, const int*, const int*, const int*, int, int, double*, double*);
} BeaglePartitionApi;
const BeaglePartitionApi* beagleGetPartitionApiTable(void);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* BEAGLE_MI355_H */
