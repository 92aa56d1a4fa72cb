// jni_mds.cpp — the 14 `native` methods of dr.inference.multidimensionalscaling.NativeMDSSingleton (NativeMDSSingleton.java:
// 134-161) as Java_dr_inference_multidimensionalscaling_NativeMDSSingleton_<name> symbols, each a copy-in / copy-out wrapper
// over the mds* calls of include/mds_mi355.h.  They are instance methods (second argument: the singleton), and `initialize` is
// overloaded, so its two symbols carry the mangled argument signature.  NativeMDSSingleton loads the library with
// System.loadLibrary("mds2_jni") from java.library.path or -Dmds.library.path.
//
// Arrays are copied as in jni_basta.cpp: what a call uses and no more — D or N * D doubles of `locations`, N * N observations,
// one parameter.  Most natives return void, so a failure cannot be a code: a negative code from the C ABI, a null array or one
// shorter than the call needs raises java.lang.RuntimeException("<function>: <code>") through FindClass + ThrowNew and returns
// with no output written (NaN from getSumOfIncrements, null from getPairwiseData, the code from initialize / getInternalDimension).
#include <math.h>
#include <stddef.h>
#include <stdio.h>

#include <vector>

#include "../../include/mds_mi355.h"
#include "../csrc/jni_min.h"

namespace {

void raise(JNIEnv* env, const char* function, int code) {
    char message[96];
    snprintf(message, sizeof message, "%s: %d", function, code);
    jclass cls = jni::FindClass(env, "java/lang/RuntimeException");
    if (cls) jni::ThrowNew(env, cls, message);
}

// the first n entries of a Java array (false: the array is null or shorter)
bool readDoubles(JNIEnv* env, jdoubleArray a, long long n, std::vector<jdouble>& out) {
    if (!a || n < 0 || n > (long long)jni::GetArrayLength(env, a)) return false;
    out.resize((size_t)n);
    if (n) jni::GetDoubleArrayRegion(env, a, 0, (jsize)n, out.data());
    return true;
}

// N and D of an instance; a negative code raises
bool dimensions(JNIEnv* env, const char* function, int instance, long long& n, long long& d) {
    const int count = mdsGetLocationCount(instance), dim = count < 0 ? count : mdsGetInternalDimension(instance);
    if (count < 0 || dim < 0) {
        raise(env, function, count < 0 ? count : dim);
        return false;
    }
    n = count;
    d = dim;
    return true;
}

void simple(JNIEnv* env, const char* function, int rc) {
    if (rc < 0) raise(env, function, rc);
}

}  // namespace

#define MDS_FN(ret, name) extern "C" JNIEXPORT ret JNICALL Java_dr_inference_multidimensionalscaling_NativeMDSSingleton_##name

// initialize (IIJII)I
MDS_FN(jint, initialize__IIJII)(JNIEnv* env, jobject, jint dimensionCount, jint locationCount, jlong flags, jint deviceNumber, jint threads) {
    const int rc = mdsInitialize(dimensionCount, locationCount, flags, deviceNumber, threads);
    if (rc < 0) raise(env, "mdsInitialize", rc);
    return rc;
}

// initialize (IIIJII)I — the rows x columns layout: not built
MDS_FN(jint, initialize__IIIJII)(JNIEnv* env, jobject, jint dimensionCount, jint rowLocationCount, jint columnLocationCount, jlong flags,
                                 jint deviceNumber, jint threads) {
    const int rc = mdsInitializeLayout(dimensionCount, rowLocationCount, columnLocationCount, flags, deviceNumber, threads);
    if (rc < 0) raise(env, "mdsInitializeLayout", rc);
    return rc;
}

// updateLocations (II[D)V
MDS_FN(void, updateLocations)(JNIEnv* env, jobject, jint instance, jint index, jdoubleArray locations) {
    long long n, d;
    if (!dimensions(env, "mdsUpdateLocations", instance, n, d)) return;
    std::vector<jdouble> values;
    const long long need = index < 0 ? n * d : d;
    if (!readDoubles(env, locations, need, values)) return raise(env, "mdsUpdateLocations", MDS_ERROR_OUT_OF_RANGE);
    simple(env, "mdsUpdateLocations", mdsUpdateLocations(instance, index, values.data(), need));
}

// getSumOfIncrements (I)D
MDS_FN(jdouble, getSumOfIncrements)(JNIEnv* env, jobject, jint instance) {
    double sum = NAN;
    const int rc = mdsGetSumOfIncrements(instance, &sum);
    if (rc < 0) {
        raise(env, "mdsGetSumOfIncrements", rc);
        return NAN;
    }
    return sum;
}

// storeState, restoreState, acceptState, makeDirty (I)V
MDS_FN(void, storeState)(JNIEnv* env, jobject, jint instance) { simple(env, "mdsStoreState", mdsStoreState(instance)); }
MDS_FN(void, restoreState)(JNIEnv* env, jobject, jint instance) { simple(env, "mdsRestoreState", mdsRestoreState(instance)); }
MDS_FN(void, acceptState)(JNIEnv* env, jobject, jint instance) { simple(env, "mdsAcceptState", mdsAcceptState(instance)); }
MDS_FN(void, makeDirty)(JNIEnv* env, jobject, jint instance) { simple(env, "mdsMakeDirty", mdsMakeDirty(instance)); }

// setPairwiseData (I[D)V
MDS_FN(void, setPairwiseData)(JNIEnv* env, jobject, jint instance, jdoubleArray observations) {
    long long n, d;
    if (!dimensions(env, "mdsSetPairwiseData", instance, n, d)) return;
    std::vector<jdouble> values;
    if (!readDoubles(env, observations, n * n, values)) return raise(env, "mdsSetPairwiseData", MDS_ERROR_OUT_OF_RANGE);
    simple(env, "mdsSetPairwiseData", mdsSetPairwiseData(instance, values.data(), n * n));
}

// setParameters (I[D)V
MDS_FN(void, setParameters)(JNIEnv* env, jobject, jint instance, jdoubleArray parameters) {
    std::vector<jdouble> values;
    if (!readDoubles(env, parameters, 1, values)) return raise(env, "mdsSetParameters", MDS_ERROR_OUT_OF_RANGE);
    simple(env, "mdsSetParameters", mdsSetParameters(instance, values.data(), 1));
}

// getPairwiseData (I)[D
MDS_FN(jdoubleArray, getPairwiseData)(JNIEnv* env, jobject, jint instance) {
    long long n, d;
    if (!dimensions(env, "mdsGetPairwiseData", instance, n, d)) return nullptr;
    if (n * n > 0x7fffffffLL) {                                  // a Java array holds at most 2^31 - 1 entries
        raise(env, "mdsGetPairwiseData", MDS_ERROR_OUT_OF_RANGE);
        return nullptr;
    }
    std::vector<jdouble> values((size_t)(n * n));
    const int rc = mdsGetPairwiseData(instance, values.data(), n * n);
    if (rc < 0) {
        raise(env, "mdsGetPairwiseData", rc);
        return nullptr;
    }
    jdoubleArray out = jni::NewDoubleArray(env, (jsize)(n * n));
    if (!out) return nullptr;                                    // OutOfMemoryError is pending
    jni::SetDoubleArrayRegion(env, out, 0, (jsize)(n * n), values.data());
    return out;
}

// getLocationGradient (I[D)V
MDS_FN(void, getLocationGradient)(JNIEnv* env, jobject, jint instance, jdoubleArray gradient) {
    long long n, d;
    if (!dimensions(env, "mdsGetLocationGradient", instance, n, d)) return;
    if (!gradient || n * d > (long long)jni::GetArrayLength(env, gradient)) return raise(env, "mdsGetLocationGradient", MDS_ERROR_OUT_OF_RANGE);
    std::vector<jdouble> values((size_t)(n * d));
    const int rc = mdsGetLocationGradient(instance, values.data(), n * d);
    if (rc < 0) return raise(env, "mdsGetLocationGradient", rc);
    jni::SetDoubleArrayRegion(env, gradient, 0, (jsize)(n * d), values.data());
}

// getObservationGradient (I[D)V — not built
MDS_FN(void, getObservationGradient)(JNIEnv* env, jobject, jint instance, jdoubleArray) {
    simple(env, "mdsGetObservationGradient", mdsGetObservationGradient(instance, nullptr, 0));
}

// getInternalDimension (I)I
MDS_FN(jint, getInternalDimension)(JNIEnv* env, jobject, jint instance) {
    const int rc = mdsGetInternalDimension(instance);
    if (rc < 0) raise(env, "mdsGetInternalDimension", rc);
    return rc;
}
