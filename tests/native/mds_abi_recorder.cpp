// mds_abi_recorder.cpp — every function of include/mds_mi355.h as a recorder, for tests/test_mds_host.py: jni_mds.cpp is compiled
// with this file instead of the engine, each native is called through a Python JNIEnv, and the test reads what reached the C ABI.
// The instance it pretends to hold has N = 5 locations in D = 3 dimensions.  mdsRecorderFail(name, code) makes one function
// answer a code; outputs are recognisable: the sum 42.5, observation e = 1000 + e, gradient entry e = -(e + 1).
#include <string.h>

#include <map>
#include <string>
#include <vector>

#include "../../include/mds_mi355.h"

namespace {
struct Call {
    std::string name;
    std::vector<long long> scalars;
    long long length = -1;
    std::vector<double> data;
};
std::vector<Call> g_calls;
std::map<std::string, int> g_fail;
constexpr int N = 5, D = 3;

int record(const char* name, std::vector<long long> scalars, const double* data = nullptr, long long length = -1) {
    Call c;
    c.name = name;
    c.scalars = scalars;
    c.length = length;
    if (data && length > 0) c.data.assign(data, data + length);
    g_calls.push_back(c);
    auto it = g_fail.find(name);
    return it == g_fail.end() ? 0 : it->second;
}
}  // namespace

#define REC extern "C" __attribute__((visibility("default")))

REC void mdsRecorderReset() { g_calls.clear(); g_fail.clear(); }
REC void mdsRecorderFail(const char* name, int code) { g_fail[name] = code; }
REC int mdsRecorderCalls() { return (int)g_calls.size(); }
REC const char* mdsRecorderName(int i) { return g_calls[(size_t)i].name.c_str(); }
REC int mdsRecorderScalarCount(int i) { return (int)g_calls[(size_t)i].scalars.size(); }
REC long long mdsRecorderScalar(int i, int k) { return g_calls[(size_t)i].scalars[(size_t)k]; }
REC long long mdsRecorderLength(int i) { return g_calls[(size_t)i].length; }
REC void mdsRecorderData(int i, double* out) { memcpy(out, g_calls[(size_t)i].data.data(), g_calls[(size_t)i].data.size() * sizeof(double)); }

REC int mdsInitialize(int dimension, int locationCount, long long flags, int deviceNumber, int threads) {
    const int rc = record("mdsInitialize", {dimension, locationCount, flags, deviceNumber, threads});
    return rc ? rc : 7;
}
REC int mdsInitializeLayout(int dimension, int rows, int columns, long long flags, int deviceNumber, int threads) {
    record("mdsInitializeLayout", {dimension, rows, columns, flags, deviceNumber, threads});
    return MDS_ERROR_NO_IMPLEMENTATION;
}
REC int mdsFinalize(int instance) { return record("mdsFinalize", {instance}); }
REC int mdsUpdateLocations(int instance, int index, const double* values, long long length) {
    return record("mdsUpdateLocations", {instance, index}, values, length);
}
REC int mdsGetSumOfIncrements(int instance, double* outSum) {
    const int rc = record("mdsGetSumOfIncrements", {instance});
    if (!rc) *outSum = 42.5;
    return rc;
}
REC int mdsStoreState(int instance) { return record("mdsStoreState", {instance}); }
REC int mdsRestoreState(int instance) { return record("mdsRestoreState", {instance}); }
REC int mdsAcceptState(int instance) { return record("mdsAcceptState", {instance}); }
REC int mdsMakeDirty(int instance) { return record("mdsMakeDirty", {instance}); }
REC int mdsSetPairwiseData(int instance, const double* observations, long long length) {
    return record("mdsSetPairwiseData", {instance}, observations, length);
}
REC int mdsGetPairwiseData(int instance, double* out, long long length) {
    const int rc = record("mdsGetPairwiseData", {instance}, nullptr, length);
    if (!rc)
        for (long long e = 0; e < length; ++e) out[e] = 1000.0 + (double)e;
    return rc;
}
REC int mdsSetParameters(int instance, const double* parameters, long long length) {
    return record("mdsSetParameters", {instance}, parameters, length);
}
REC int mdsGetLocationGradient(int instance, double* out, long long length) {
    const int rc = record("mdsGetLocationGradient", {instance}, nullptr, length);
    if (!rc)
        for (long long e = 0; e < length; ++e) out[e] = -(double)(e + 1);
    return rc;
}
REC int mdsGetObservationGradient(int instance, double*, long long length) {
    record("mdsGetObservationGradient", {instance}, nullptr, length);
    return MDS_ERROR_NO_IMPLEMENTATION;
}
REC int mdsGetInternalDimension(int instance) {
    const int rc = record("mdsGetInternalDimension", {instance});
    return rc ? rc : D;
}
REC int mdsGetLocationCount(int instance) {
    const int rc = record("mdsGetLocationCount", {instance});
    return rc ? rc : N;
}
REC int mdsStats(int instance, long long*, int count) { return record("mdsStats", {instance, count}); }
