// abi_recorder.cpp — every beagle* function beast-mcmc_amd/csrc/jni_shim.cpp references, as a RECORDER.
// TEST INFRASTRUCTURE (tests/test_jni_marshalling.py): linked with jni_shim.cpp into a temporary shared object, on the CPU.
//
// Each function appends one record: its name, its scalar arguments in ABI order, and for each pointer argument in ABI order
// whether it was null and the first n entries behind it — n is what the TEST says the BEAGLE contract lets that call touch
// (rec_expect: one length per pointer argument of the next call; the table of lengths lives in the test, not here).  Output
// pointers are filled with n values that encode the pointer's position and the entry's (fill()), in/out pointers get that value
// ADDED.  The return code is what the test set beforehand (rec_set_rc).  beagleMi355GetDimensions answers the sizes the test
// chose; the two ...Pinned calls answer a buffer of the recorder's or BEAGLE_ERROR_NO_IMPLEMENTATION, by a switch.
// A wrapper that hands over a SHORTER buffer than the contract lets the library touch must fail its test, not take the test
// process down: the buffers are the wrapper's std::vectors, i.e. heap blocks, so malloc_usable_size bounds what is touched and the
// shortfall is recorded (rec_pointer_overrun; the test requires 0 everywhere).
#include <malloc.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/beagle_mi355.h"

namespace {
struct Ptr { int isNull = 1; long overrun = 0; std::vector<double> seen; };
struct Record { std::string name; std::vector<double> scalars; std::vector<Ptr> ptrs; };
std::vector<Record> g_records;
std::vector<long> g_expect;            // entries the next call may touch behind its pointer arguments, in ABI order
int g_rc = 0, g_pinned = 1;
int g_dims[8] = {0, 0, 0, 0, 0, 0, 0, 0};
std::vector<double> g_pinnedBuffer;

struct Call {
    Record r;
    explicit Call(const char* name) { r.name = name; }
    long expected() const { const size_t k = r.ptrs.size(); return k < g_expect.size() ? g_expect[k] : 0; }
    // entries of the n expected that the block behind p really has (n == 0: p need not be a heap block and is not touched)
    template <class T> long within(const T* p, Ptr& q) const {
        const long n = expected();
        if (!p || n <= 0) return 0;
        const long have = (long)(malloc_usable_size(const_cast<T*>(p)) / sizeof(T));
        if (have < n) q.overrun = n - have;
        return have < n ? have : n;
    }
    static double fill(size_t pointer, long entry) { return 1000.0 * (double)(pointer + 1) + (double)entry; }
    Call& s(double v) { r.scalars.push_back(v); return *this; }
    template <class T> Call& in(const T* p) {
        Ptr q; q.isNull = p == nullptr;
        const long n = within(p, q);
        for (long j = 0; j < n; j++) q.seen.push_back((double)p[j]);
        r.ptrs.push_back(q); return *this;
    }
    template <class T> Call& out(T* p, bool add = false) {
        Ptr q; q.isNull = p == nullptr;
        const size_t k = r.ptrs.size();
        const long n = within(p, q);
        for (long j = 0; j < n; j++) {
            if (add) { q.seen.push_back((double)p[j]); p[j] += (T)(fill(k, j) + 0.5); }
            else p[j] = (T)(fill(k, j) + (sizeof(T) == 8 ? 0.5 : 0.0));
        }
        r.ptrs.push_back(q); return *this;
    }
    template <class T> Call& inout(T* p) { return out(p, true); }
    int done() { g_records.push_back(r); g_expect.clear(); return g_rc; }
};
}  // namespace

extern "C" {
// ---- what the test drives the recorder with ----
__attribute__((visibility("default"))) void rec_reset(void) { g_records.clear(); g_expect.clear(); g_rc = 0; }
__attribute__((visibility("default"))) void rec_set_rc(int rc) { g_rc = rc; }
__attribute__((visibility("default"))) void rec_set_pinned(int on) { g_pinned = on; }
__attribute__((visibility("default"))) void rec_set_dims(const int* d8) { memcpy(g_dims, d8, sizeof g_dims); }
__attribute__((visibility("default"))) void rec_expect(const long* n, int count) { g_expect.assign(n, n + count); }
__attribute__((visibility("default"))) int rec_count(void) { return (int)g_records.size(); }
__attribute__((visibility("default"))) const char* rec_name(int i) { return g_records[i].name.c_str(); }
__attribute__((visibility("default"))) int rec_scalar_count(int i) { return (int)g_records[i].scalars.size(); }
__attribute__((visibility("default"))) double rec_scalar(int i, int k) { return g_records[i].scalars[k]; }
__attribute__((visibility("default"))) int rec_pointer_count(int i) { return (int)g_records[i].ptrs.size(); }
__attribute__((visibility("default"))) int rec_pointer_null(int i, int k) { return g_records[i].ptrs[k].isNull; }
__attribute__((visibility("default"))) long rec_pointer_overrun(int i, int k) { return g_records[i].ptrs[k].overrun; }
__attribute__((visibility("default"))) int rec_pointer_seen(int i, int k) { return (int)g_records[i].ptrs[k].seen.size(); }
__attribute__((visibility("default"))) double rec_pointer_value(int i, int k, int j) { return g_records[i].ptrs[k].seen[j]; }
__attribute__((visibility("default"))) double rec_fill(int pointer, long entry) { return Call::fill((size_t)pointer, entry); }

// ---- the ABI ----
const char* beagleGetVersion(void) { Call("beagleGetVersion").done(); return "9.8.7-recorder"; }
const char* beagleGetCitation(void) { Call("beagleGetCitation").done(); return "recorder citation\nsecond line"; }
BeagleResourceList* beagleGetResourceList(void) { static BeagleResourceList rl = {nullptr, 0}; return &rl; }
BeagleBenchmarkedResourceList* beagleGetBenchmarkedResourceList(int, int, int, int, int, const int*, int, long, long, int, int, int, long) {
    static BeagleBenchmarkedResourceList bl = {nullptr, 0}; return &bl;
}
int beagleCreateInstance(int tipCount, int partialsBufferCount, int compactBufferCount, int stateCount, int patternCount,
                         int eigenBufferCount, int matrixBufferCount, int categoryCount, int scaleBufferCount,
                         const int* resourceList, int resourceCount, long preferenceFlags, long requirementFlags,
                         BeagleInstanceDetails* returnInfo) {
    Call c("beagleCreateInstance");
    c.s(tipCount).s(partialsBufferCount).s(compactBufferCount).s(stateCount).s(patternCount).s(eigenBufferCount).s(matrixBufferCount)
        .s(categoryCount).s(scaleBufferCount).in(resourceList).s(resourceCount).s((double)preferenceFlags).s((double)requirementFlags);
    (void)returnInfo;
    return c.done();
}
int beagleFinalizeInstance(int i) { return Call("beagleFinalizeInstance").s(i).done(); }
int beagleSetCPUThreadCount(int i, int n) { return Call("beagleSetCPUThreadCount").s(i).s(n).done(); }
int beagleSetPatternWeights(int i, const double* w) { return Call("beagleSetPatternWeights").s(i).in(w).done(); }
int beagleSetPatternPartitions(int i, int k, const int* p) { return Call("beagleSetPatternPartitions").s(i).s(k).in(p).done(); }
int beagleSetTipStates(int i, int t, const int* s) { return Call("beagleSetTipStates").s(i).s(t).in(s).done(); }
int beagleGetTipStates(int i, int t, int* s) { return Call("beagleGetTipStates").s(i).s(t).out(s).done(); }
int beagleSetTipPartials(int i, int t, const double* p) { return Call("beagleSetTipPartials").s(i).s(t).in(p).done(); }
int beagleSetPartials(int i, int b, const double* p) { return Call("beagleSetPartials").s(i).s(b).in(p).done(); }
int beagleGetPartials(int i, int b, int sc, double* p) { return Call("beagleGetPartials").s(i).s(b).s(sc).out(p).done(); }
int beagleGetLogScaleFactors(int i, int sc, double* p) { return Call("beagleGetLogScaleFactors").s(i).s(sc).out(p).done(); }
int beagleSetEigenDecomposition(int i, int e, const double* u, const double* ui, const double* lam) {
    return Call("beagleSetEigenDecomposition").s(i).s(e).in(u).in(ui).in(lam).done();
}
int beagleSetStateFrequencies(int i, int k, const double* f) { return Call("beagleSetStateFrequencies").s(i).s(k).in(f).done(); }
int beagleSetCategoryWeights(int i, int k, const double* w) { return Call("beagleSetCategoryWeights").s(i).s(k).in(w).done(); }
int beagleSetCategoryRates(int i, const double* r) { return Call("beagleSetCategoryRates").s(i).in(r).done(); }
int beagleSetCategoryRatesWithIndex(int i, int k, const double* r) { return Call("beagleSetCategoryRatesWithIndex").s(i).s(k).in(r).done(); }
int beagleSetTransitionMatrix(int i, int m, const double* in, double padded) { return Call("beagleSetTransitionMatrix").s(i).s(m).in(in).s(padded).done(); }
int beagleSetDifferentialMatrix(int i, int m, const double* in) { return Call("beagleSetDifferentialMatrix").s(i).s(m).in(in).done(); }
int beagleGetTransitionMatrix(int i, int m, double* out) { return Call("beagleGetTransitionMatrix").s(i).s(m).out(out).done(); }
int beagleConvolveTransitionMatrices(int i, const int* a, const int* b, const int* r, int n) {
    return Call("beagleConvolveTransitionMatrices").s(i).in(a).in(b).in(r).s(n).done();
}
int beagleAddTransitionMatrices(int i, const int* a, const int* b, const int* r, int n) {
    return Call("beagleAddTransitionMatrices").s(i).in(a).in(b).in(r).s(n).done();
}
int beagleTransposeTransitionMatrices(int i, const int* a, const int* r, int n) {
    return Call("beagleTransposeTransitionMatrices").s(i).in(a).in(r).s(n).done();
}
int beagleUpdateTransitionMatrices(int i, int e, const int* p, const int* d1, const int* d2, const double* t, int n) {
    return Call("beagleUpdateTransitionMatrices").s(i).s(e).in(p).in(d1).in(d2).in(t).s(n).done();
}
int beagleUpdateTransitionMatricesWithMultipleModels(int i, const int* e, const int* r, const int* p, const int* d1, const int* d2,
                                                     const double* t, int n) {
    return Call("beagleUpdateTransitionMatricesWithMultipleModels").s(i).in(e).in(r).in(p).in(d1).in(d2).in(t).s(n).done();
}
int beagleUpdatePrePartials(int i, const int* ops, int n, int cum) { return Call("beagleUpdatePrePartials").s(i).in(ops).s(n).s(cum).done(); }
int beagleUpdatePrePartialsByPartition(int i, const int* ops, int n) { return Call("beagleUpdatePrePartialsByPartition").s(i).in(ops).s(n).done(); }
int beagleUpdatePartials(int i, const int* ops, int n, int cum) { return Call("beagleUpdatePartials").s(i).in(ops).s(n).s(cum).done(); }
int beagleUpdatePartialsByPartition(int i, const int* ops, int n) { return Call("beagleUpdatePartialsByPartition").s(i).in(ops).s(n).done(); }
int beagleWaitForPartials(int i, const int* d, int n) { return Call("beagleWaitForPartials").s(i).in(d).s(n).done(); }
int beagleAccumulateScaleFactors(int i, const int* s, int n, int cum) { return Call("beagleAccumulateScaleFactors").s(i).in(s).s(n).s(cum).done(); }
int beagleAccumulateScaleFactorsByPartition(int i, const int* s, int n, int cum, int part) {
    return Call("beagleAccumulateScaleFactorsByPartition").s(i).in(s).s(n).s(cum).s(part).done();
}
int beagleRemoveScaleFactors(int i, const int* s, int n, int cum) { return Call("beagleRemoveScaleFactors").s(i).in(s).s(n).s(cum).done(); }
int beagleRemoveScaleFactorsByPartition(int i, const int* s, int n, int cum, int part) {
    return Call("beagleRemoveScaleFactorsByPartition").s(i).in(s).s(n).s(cum).s(part).done();
}
int beagleResetScaleFactors(int i, int cum) { return Call("beagleResetScaleFactors").s(i).s(cum).done(); }
int beagleResetScaleFactorsByPartition(int i, int cum, int part) { return Call("beagleResetScaleFactorsByPartition").s(i).s(cum).s(part).done(); }
int beagleCopyScaleFactors(int i, int dst, int src) { return Call("beagleCopyScaleFactors").s(i).s(dst).s(src).done(); }
int beagleCalculateRootLogLikelihoods(int i, const int* b, const int* w, const int* f, const int* c, int n, double* out) {
    return Call("beagleCalculateRootLogLikelihoods").s(i).in(b).in(w).in(f).in(c).s(n).out(out).done();
}
int beagleCalculateRootLogLikelihoodsByPartition(int i, const int* b, const int* w, const int* f, const int* c, const int* p,
                                                 int partitionCount, int n, double* byPartition, double* out) {
    return Call("beagleCalculateRootLogLikelihoodsByPartition").s(i).in(b).in(w).in(f).in(c).in(p).s(partitionCount).s(n).out(byPartition).out(out).done();
}
int beagleGetSiteLogLikelihoods(int i, double* out) { return Call("beagleGetSiteLogLikelihoods").s(i).out(out).done(); }
int beagleSetRootPrePartials(int i, const int* b, const int* f, int n) { return Call("beagleSetRootPrePartials").s(i).in(b).in(f).s(n).done(); }
int beagleCalculateEdgeDifferentials(int i, const int* post, const int* pre, const int* d, const int* w, int n, double* o0, double* o1,
                                     double* o2) {
    return Call("beagleCalculateEdgeDifferentials").s(i).in(post).in(pre).in(d).in(w).s(n).out(o0).out(o1).out(o2).done();
}
int beagleCalculateCrossProductDifferentials(int i, const int* post, const int* pre, const int* r, const int* w, const double* t, int n,
                                             double* o1, double* o2) {
    return Call("beagleCalculateCrossProductDifferentials").s(i).in(post).in(pre).in(r).in(w).in(t).s(n).inout(o1).inout(o2).done();
}

// ---- the extensions the shim leans on ----
int beagleMi355GetDimensions(int, int* out8) { memcpy(out8, g_dims, sizeof g_dims); return BEAGLE_SUCCESS; }
static int pinned(Call& c, const double** outPinned, long* outCount) {
    const long n = g_expect.empty() ? 0 : g_expect[0];
    g_pinnedBuffer.assign((size_t)n + 8, -777.0);               // (longer than what it defines: the shim must copy n, not more)
    for (long j = 0; j < n; j++) g_pinnedBuffer[j] = Call::fill(0, j) + 0.5;
    *outPinned = g_pinnedBuffer.data(); *outCount = n;
    return c.done();
}
int beagleMi355GetPartialsPinned(int i, int b, int sc, const double** outPinned, long* outCount) {
    if (!g_pinned) return BEAGLE_ERROR_NO_IMPLEMENTATION;
    Call c("beagleMi355GetPartialsPinned"); c.s(i).s(b).s(sc);
    return pinned(c, outPinned, outCount);
}
int beagleMi355GetSiteLogLikelihoodsPinned(int i, const double** outPinned, long* outCount) {
    if (!g_pinned) return BEAGLE_ERROR_NO_IMPLEMENTATION;
    Call c("beagleMi355GetSiteLogLikelihoodsPinned"); c.s(i);
    return pinned(c, outPinned, outCount);
}
}
