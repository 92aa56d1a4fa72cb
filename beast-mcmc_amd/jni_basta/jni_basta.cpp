// jni_basta.cpp — libhmsbeagle-jni-bit.so: the seven `native` methods of beagle.basta.BastaJNIWrapper
// (src/beagle/basta/BastaJNIWrapper.java:36-94) as Java_beagle_basta_BastaJNIWrapper_<name> symbols, each a copy-in / copy-out
// wrapper over the beagleBasta* calls of include/beagle_mi355.h.
//
// BastaJNIImpl extends BeagleJNIImpl: the instance is created through libhmsbeagle-jni.so's createInstance and these natives
// take the same handle, so this library holds no state and links the engine library next to it ($ORIGIN rpath, build.py).
// BastaJNIWrapper loads it with System.loadLibrary("hmsbeagle-jni-bit").
//
// Arrays are copied as in csrc/jni_shim.cpp: what a call uses, not the whole array (BeagleBastaLikelihoodDelegate sizes its
// arrays exactly, other callers need not); an array shorter than that is BEAGLE_ERROR_OUT_OF_RANGE.  accumulateBastaPartials'
// `result` is in/out: entry 0 is read, the log-density added, and written back only when the call succeeded.
#include <stddef.h>

#include <vector>

#include "../../include/beagle_mi355.h"
#include "../csrc/jni_min.h"

namespace {

constexpr int BASTA_OP = 8;

// the first n entries of a Java array (false: the array is null or shorter)
bool readInts(JNIEnv* env, jintArray a, long n, std::vector<jint>& out) {
    if (!a || n < 0 || n > (long)jni::GetArrayLength(env, a)) return false;
    out.resize((size_t)n);
    if (n) jni::GetIntArrayRegion(env, a, 0, (jsize)n, out.data());
    return true;
}
bool readDoubles(JNIEnv* env, jdoubleArray a, long n, std::vector<jdouble>& out) {
    if (!a || n < 0 || n > (long)jni::GetArrayLength(env, a)) return false;
    out.resize((size_t)n);
    if (n) jni::GetDoubleArrayRegion(env, a, 0, (jsize)n, out.data());
    return true;
}

}  // namespace

#define BASTA_FN(ret, name) extern "C" JNIEXPORT ret JNICALL Java_beagle_basta_BastaJNIWrapper_##name

// allocateCoalescentBuffers (IIIIII)I
BASTA_FN(jint, allocateCoalescentBuffers)(JNIEnv*, jobject, jint instance, jint bufferCount, jint maxCoalescentIntervalCount,
                                          jint partialsBufferCount, jint initial, jint threadCount) {
    return beagleBastaAllocateCoalescentBuffers(instance, bufferCount, maxCoalescentIntervalCount, partialsBufferCount, initial, threadCount);
}

// getBastaBuffer (II[D)I
BASTA_FN(jint, getBastaBuffer)(JNIEnv* env, jobject, jint instance, jint index, jdoubleArray buffer) {
    const int n = beagleBastaGetBufferLength(instance, index);
    if (n < 0) return n;
    if (!buffer || n > (int)jni::GetArrayLength(env, buffer)) return BEAGLE_ERROR_OUT_OF_RANGE;
    std::vector<jdouble> out((size_t)n);
    const int rc = beagleBastaGetBuffer(instance, index, out.data());
    if (rc == BEAGLE_SUCCESS && n) jni::SetDoubleArrayRegion(env, buffer, 0, (jsize)n, out.data());
    return rc;
}

// updateBastaPartials (I[II[IIII)I
BASTA_FN(jint, updateBastaPartials)(JNIEnv* env, jobject, jint instance, jintArray operations, jint operationCount,
                                    jintArray intervals, jint intervalCount, jint populationSizeIndex, jint coalescentProbabilityIndex) {
    std::vector<jint> ops, iv;
    if (!readInts(env, operations, (long)operationCount * BASTA_OP, ops) || !readInts(env, intervals, intervalCount, iv))
        return BEAGLE_ERROR_OUT_OF_RANGE;
    return beagleBastaUpdatePartials(instance, ops.data(), operationCount, iv.data(), intervalCount, populationSizeIndex, coalescentProbabilityIndex);
}

// accumulateBastaPartials (I[II[II[DII[D)I
BASTA_FN(jint, accumulateBastaPartials)(JNIEnv* env, jobject, jint instance, jintArray operations, jint operationCount,
                                        jintArray intervals, jint intervalCount, jdoubleArray intervalLengths,
                                        jint populationSizesIndex, jint coalescentProbabilityIndex, jdoubleArray result) {
    std::vector<jint> ops, iv;
    std::vector<jdouble> lengths, out;
    if (!readInts(env, operations, (long)operationCount * BASTA_OP, ops) || !readInts(env, intervals, intervalCount, iv) ||
        !readDoubles(env, intervalLengths, intervalCount > 0 ? intervalCount - 1 : 0, lengths) || !readDoubles(env, result, 1, out))
        return BEAGLE_ERROR_OUT_OF_RANGE;
    const int rc = beagleBastaAccumulatePartials(instance, ops.data(), operationCount, iv.data(), intervalCount, lengths.data(),
                                                 populationSizesIndex, coalescentProbabilityIndex, out.data());
    if (rc == BEAGLE_SUCCESS) jni::SetDoubleArrayRegion(env, result, 0, 1, out.data());
    return rc;
}

// updateBastaPartialsGrad (I[II[IIII)I
BASTA_FN(jint, updateBastaPartialsGrad)(JNIEnv*, jobject, jint instance, jintArray, jint operationCount, jintArray, jint intervalCount,
                                        jint populationSizeIndex, jint coalescentProbabilityIndex) {
    return beagleBastaUpdatePartialsGrad(instance, nullptr, operationCount, nullptr, intervalCount, populationSizeIndex, coalescentProbabilityIndex);
}

// updateTransitionMatricesGrad (I[I[DI)I
BASTA_FN(jint, updateTransitionMatricesGrad)(JNIEnv*, jobject, jint instance, jintArray, jdoubleArray, jint count) {
    return beagleBastaUpdateTransitionMatricesGrad(instance, nullptr, nullptr, count);
}

// accumulateBastaPartialsGrad (I[II[II[DII[D)I
BASTA_FN(jint, accumulateBastaPartialsGrad)(JNIEnv*, jobject, jint instance, jintArray, jint operationCount, jintArray, jint intervalCount,
                                            jdoubleArray, jint populationSizeIndex, jint coalescentProbabilityIndex, jdoubleArray) {
    return beagleBastaAccumulatePartialsGrad(instance, nullptr, operationCount, nullptr, intervalCount, nullptr, populationSizeIndex,
                                             coalescentProbabilityIndex, nullptr);
}
