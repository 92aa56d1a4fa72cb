// fake_jvm_basta.cpp — drives libhmsbeagle-jni.so and libhmsbeagle-jni-bit.so through their JNI natives without a JVM, the way
// beagle.basta.BastaJNIImpl does: the instance comes from Java_beagle_BeagleJNIWrapper_createInstance, the BASTA natives of the
// second library take the same handle.  The JNIEnv here is a table of its own with the four entries those natives may use
// (array length, int / double region get, double region set); every other slot aborts.
//
//   fake_jvm_basta <libhmsbeagle-jni.so> <libhmsbeagle-jni-bit.so> <fixture.txt>
// fixture: S T partialsBufferCount maxIntervals matrixCount nOps nIntervals | T x S tip vectors | S sizes | nMatrices, then per
// matrix its number and S x S entries | nOps x 8 ints | nIntervals offsets | nIntervals - 1 lengths.
// Prints "logL <hex float> <decimal>", "grad <rc> <rc> <rc>" and "probabilities <n> ...".
#include <dlfcn.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

typedef int32_t jint;
typedef int64_t jlong;
typedef double jdouble;
typedef void* jobject;
typedef const void* const* Table;
typedef Table JNIEnv;

struct IntArray { std::vector<jint> v; };
struct DoubleArray { std::vector<jdouble> v; };
// every Java array handed out below is one of these; `kind` tells the length function which
struct Array { int kind; IntArray i; DoubleArray d; };

static void forbidden() { fprintf(stderr, "a JNI function outside the four allowed ones was called\n"); abort(); }
static jint getArrayLength(JNIEnv*, jobject a) { Array* x = (Array*)a; return (jint)(x->kind == 0 ? x->i.v.size() : x->d.v.size()); }
static void getIntRegion(JNIEnv*, jobject a, jint start, jint len, jint* buf) {
    Array* x = (Array*)a;
    if (x->kind != 0 || start < 0 || (size_t)start + len > x->i.v.size()) abort();
    for (jint k = 0; k < len; k++) buf[k] = x->i.v[start + k];
}
static void getDoubleRegion(JNIEnv*, jobject a, jint start, jint len, jdouble* buf) {
    Array* x = (Array*)a;
    if (x->kind != 1 || start < 0 || (size_t)start + len > x->d.v.size()) abort();
    for (jint k = 0; k < len; k++) buf[k] = x->d.v[start + k];
}
static void setDoubleRegion(JNIEnv*, jobject a, jint start, jint len, const jdouble* buf) {
    Array* x = (Array*)a;
    if (x->kind != 1 || start < 0 || (size_t)start + len > x->d.v.size()) abort();
    for (jint k = 0; k < len; k++) x->d.v[start + k] = buf[k];
}

static Array* ints(const std::vector<jint>& v, size_t extra) { Array* a = new Array(); a->kind = 0; a->i.v = v; a->i.v.resize(v.size() + extra, -12345); return a; }
static Array* doubles(const std::vector<jdouble>& v, size_t extra) { Array* a = new Array(); a->kind = 1; a->d.v = v; a->d.v.resize(v.size() + extra, -1e300); return a; }

template <class F> static F sym(void* lib, const char* name) {
    void* p = dlsym(lib, name);
    if (!p) { fprintf(stderr, "missing symbol %s\n", name); exit(3); }
    return (F)p;
}
static double readDouble(FILE* f) { double x; if (fscanf(f, "%lf", &x) != 1) { fprintf(stderr, "short fixture\n"); exit(4); } return x; }
static int readInt(FILE* f) { int x; if (fscanf(f, "%d", &x) != 1) { fprintf(stderr, "short fixture\n"); exit(4); } return x; }
#define CHECK(call) do { const int rc__ = (call); if (rc__ != 0) { fprintf(stderr, "%s returned %d\n", #call, rc__); return 5; } } while (0)

int main(int argc, char** argv) {
    if (argc != 4) return 2;
    void* engine = dlopen(argv[1], RTLD_NOW | RTLD_GLOBAL);
    if (!engine) { fprintf(stderr, "%s\n", dlerror()); return 3; }
    void* basta = dlopen(argv[2], RTLD_NOW | RTLD_LOCAL);
    if (!basta) { fprintf(stderr, "%s\n", dlerror()); return 3; }
    FILE* f = fopen(argv[3], "r");
    if (!f) return 4;

    const void* table[229];
    for (int k = 0; k < 229; k++) table[k] = (const void*)&forbidden;
    table[171] = (const void*)&getArrayLength;
    table[203] = (const void*)&getIntRegion;
    table[206] = (const void*)&getDoubleRegion;
    table[214] = (const void*)&setDoubleRegion;
    Table tablePtr = table;
    JNIEnv* env = &tablePtr;

    const int S = readInt(f), T = readInt(f), nBuffers = readInt(f), maxIntervals = readInt(f), nMatrixSlots = readInt(f),
              nOps = readInt(f), nIntervals = readInt(f);
    typedef jint (*CreateFn)(JNIEnv*, jobject, jint, jint, jint, jint, jint, jint, jint, jint, jint, jobject, jint, jlong, jlong, jobject);
    typedef jint (*SetVecFn)(JNIEnv*, jobject, jint, jint, jobject);
    typedef jint (*SetMatFn)(JNIEnv*, jobject, jint, jint, jobject, jdouble);
    typedef jint (*FinalFn)(JNIEnv*, jobject, jint);
    const jint h = sym<CreateFn>(engine, "Java_beagle_BeagleJNIWrapper_createInstance")(
        env, nullptr, 0, nBuffers, 0, S, 1, 2, nMatrixSlots, 1, 1, nullptr, 0, 0, (jlong)(1 << 5), nullptr);
    if (h < 0) { fprintf(stderr, "createInstance returned %d\n", h); return 5; }
    typedef jint (*AllocFn)(JNIEnv*, jobject, jint, jint, jint, jint, jint, jint);
    CHECK(sym<AllocFn>(basta, "Java_beagle_basta_BastaJNIWrapper_allocateCoalescentBuffers")(env, nullptr, h, 5, maxIntervals, nBuffers, 1, -1));
    SetVecFn setPartials = sym<SetVecFn>(engine, "Java_beagle_BeagleJNIWrapper_setPartials");
    for (int t = 0; t < T; t++) {
        std::vector<jdouble> v(S);
        for (int s = 0; s < S; s++) v[s] = readDouble(f);
        CHECK(setPartials(env, nullptr, h, t, doubles(v, 3)));
    }
    std::vector<jdouble> sizes(S);
    for (int s = 0; s < S; s++) sizes[s] = readDouble(f);
    CHECK(sym<SetVecFn>(engine, "Java_beagle_BeagleJNIWrapper_setStateFrequencies")(env, nullptr, h, 0, doubles(sizes, 2)));
    const int nMatrices = readInt(f);
    SetMatFn setMatrix = sym<SetMatFn>(engine, "Java_beagle_BeagleJNIWrapper_setTransitionMatrix");
    for (int m = 0; m < nMatrices; m++) {
        const int number = readInt(f);
        std::vector<jdouble> v((size_t)S * S);
        for (auto& x : v) x = readDouble(f);
        CHECK(setMatrix(env, nullptr, h, number, doubles(v, 5), 1.0));
    }
    std::vector<jint> ops((size_t)nOps * 8), intervals(nIntervals);
    for (auto& x : ops) x = readInt(f);
    for (auto& x : intervals) x = readInt(f);
    std::vector<jdouble> lengths(nIntervals - 1);
    for (auto& x : lengths) x = readDouble(f);
    // arrays longer than what the counts say, as a caller that reuses its arrays has them
    Array* jOps = ints(ops, 40); Array* jIntervals = ints(intervals, 7); Array* jLengths = doubles(lengths, 9);
    typedef jint (*UpdateFn)(JNIEnv*, jobject, jint, jobject, jint, jobject, jint, jint, jint);
    typedef jint (*AccFn)(JNIEnv*, jobject, jint, jobject, jint, jobject, jint, jobject, jint, jint, jobject);
    CHECK(sym<UpdateFn>(basta, "Java_beagle_basta_BastaJNIWrapper_updateBastaPartials")(env, nullptr, h, jOps, nOps, jIntervals, nIntervals, 0, 0));
    Array* result = doubles(std::vector<jdouble>(1, 0.0), 2);
    CHECK(sym<AccFn>(basta, "Java_beagle_basta_BastaJNIWrapper_accumulateBastaPartials")(env, nullptr, h, jOps, nOps, jIntervals, nIntervals,
                                                                                        jLengths, 0, 0, result));
    printf("logL %a %.17g\n", result->d.v[0], result->d.v[0]);
    if (result->d.v[1] != -1e300) { fprintf(stderr, "result written past entry 0\n"); return 6; }
    const int g1 = sym<UpdateFn>(basta, "Java_beagle_basta_BastaJNIWrapper_updateBastaPartialsGrad")(env, nullptr, h, jOps, nOps, jIntervals, nIntervals, 0, 0);
    typedef jint (*MatGradFn)(JNIEnv*, jobject, jint, jobject, jobject, jint);
    const int g2 = sym<MatGradFn>(basta, "Java_beagle_basta_BastaJNIWrapper_updateTransitionMatricesGrad")(env, nullptr, h, jIntervals, jLengths, 1);
    const int g3 = sym<AccFn>(basta, "Java_beagle_basta_BastaJNIWrapper_accumulateBastaPartialsGrad")(env, nullptr, h, jOps, nOps, jIntervals, nIntervals,
                                                                                                     jLengths, 0, 0, result);
    printf("grad %d %d %d\n", g1, g2, g3);
    Array* probabilities = doubles(std::vector<jdouble>(maxIntervals, 0.0), 4);
    typedef jint (*GetFn)(JNIEnv*, jobject, jint, jint, jobject);
    CHECK(sym<GetFn>(basta, "Java_beagle_basta_BastaJNIWrapper_getBastaBuffer")(env, nullptr, h, 0, probabilities));
    printf("probabilities %d", maxIntervals);
    for (int k = 0; k < maxIntervals; k++) printf(" %a", probabilities->d.v[k]);
    printf("\n");
    CHECK(sym<FinalFn>(engine, "Java_beagle_BeagleJNIWrapper_finalize")(env, nullptr, h));
    return 0;
}
