// engine_basta.cpp — the BASTA structured-coalescent calls (include/beagle_mi355.h beagleBasta*): what
// BeagleBastaLikelihoodDelegate asks of its native library on top of an ordinary instance (one pattern, one category).
//
// State: a dense [buffer][S] array of vectors, separate from the pattern-major partials store (setPartials / getPartials of an
// instance that has it go here), and coalescentBufferCount interval-indexed buffers (coalescent probabilities, e, f, g, h).
//
// beagleBastaUpdatePartials runs a whole operation list in a number of launches that does not depend on the interval count.
// Operations of one interval are independent and an operation reads what earlier intervals wrote, so the list is a dependency
// graph over buffer indices; the reference's lists give every vector one writer and one reader (a lineage's buffer advances with
// every interval), which makes the graph a forest of chains that meet at coalescences.  analyse() checks exactly that — every
// buffer written at most once, every produced input written as a `dest` in an EARLIER interval and read by one operation — and
// then the list runs as ONE launch (kernels_basta.hip k_bastaUpdate<true>).  A list that is anything else still means what the
// interval order says, so it runs interval by interval (k_bastaUpdate<false>, a launch each): correct for every list, and never
// taken by a caller that numbers its buffers as the reference does.
//
// The 8-int list is the bulk of the traffic (16 MB at 1000 tips).  It is copied once into a pinned staging buffer and sent from
// there with one asynchronous copy; beagleBastaAccumulatePartials compares the list it is handed with the staged one — length,
// then contents (memcmp) — and uploads nothing when they are equal, which is what follows every beagleBastaUpdatePartials.
//
// beagleBastaSampleStates draws a deme for every vector of such a list from the stored vectors and matrices, any number of
// replicates in one call (kernels_basta_states.hip).  The dependency runs the other way — a vector's state needs its reader's —
// so the same forest is cut into chains by planStates() and run one launch per level of coalescences, per chunk of replicates.
//
// beagleBastaGradient walks the same chains with one adjoint vector per buffer (kernels_basta_gradient.hip) and reduces adjoints and
// vectors to the migration-rate and population-size gradients; the three gradient natives of BastaJNIWrapper stay unbuilt.
#include "engine_internal.h"

namespace mi355 {
namespace eng {

constexpr int BASTA_OP = 8;

struct Basta {
    int vectorCount = 0, maxIntervals = 0, bufferCount = 0, coalescentIndex = 0;
    double* vectors = nullptr;                           // [vectorCount][S]
    double* buffers = nullptr;                           // [bufferCount][maxIntervals * S]
    double* intervalLogL = nullptr;                      // [maxIntervals + 1] terms of the last accumulate, [maxIntervals]: their sum
    // the operation list and its intervals as last sent to the device
    int* hOps = nullptr; DevBuf dOps; size_t opsCap = 0; int opCount = -1;
    int* hIntervals = nullptr; DevBuf dIntervals; size_t intervalsCap = 0; int intervalCount = -1;
    double* hLengths = nullptr; DevBuf dLengths; size_t lengthsCap = 0;
    int* hLink = nullptr; DevBuf dLink, dTickets; size_t linkCap = 0;   // (hLink: [2 n link | n leaves])
    hipEvent_t sent = nullptr;                           // the last copy out of the pinned buffers
    std::vector<int> writer, writes, intervalOf;         // analyse()'s scratch
    long statUploads = 0, statChainCalls = 0, statIntervalCalls = 0;
    // beagleBastaSampleStates: the chains of the resident list (planStates; valid while planUpload == statUploads), its scratch
    // (scratch_layout.h BastaStatesLayout) and counters
    std::vector<int> steps, chains, levelStart;          // [step][4] | [chain][4], by level | the levels' first chains, then the chain count
    std::vector<int> chainAux, stepNumbers;              // what beagleBastaGradient needs besides: [chain][4] | [step] (kernels.h BastaGradientArgs)
    DevBuf dPlan; long planUpload = -1;                  // device: [steps | chains | chainAux | stepNumbers]
    DevBuf statesDev;
    long statStatesCalls = 0, statStatesLaunches = 0, statStatesChunks = 0;
    // beagleBastaGradient: interval lengths and distances as last sent ([2][intervals]), its scratch (scratch_layout.h
    // BastaGradientLayout) and counters
    double* hTimes = nullptr; DevBuf dTimes; size_t timesCap = 0;
    DevBuf gradientDev;
    long statGradientCalls = 0, statGradientLaunches = 0, statGradientLevels = 0;
};

namespace {

int bastaInstance(int instance, Instance** out) {
    if (mi355::isShardedHandle(instance)) return BEAGLE_ERROR_NO_IMPLEMENTATION;
    Instance* in = lookup(instance);
    if (!in) return BEAGLE_ERROR_UNINITIALIZED_INSTANCE;
    if (hipSetDevice(in->device) != hipSuccess) return BEAGLE_ERROR_GENERAL;
    if (in->P != 1 || in->C != 1) return BEAGLE_ERROR_NO_IMPLEMENTATION;
    *out = in;
    return 0;
}

// pinned host + device pair of at least `count` elements (grow-only; growing waits for the copies in flight).  `cap` is what both
// halves hold; it stays 0 when either allocation fails, so the next call starts over
template <class T> int growPair(Instance* in, T*& h, DevBuf& d, size_t& cap, size_t count) {
    if (cap >= count) return 0;
    HIP_TRY(hipStreamSynchronize(live(in)));
    if (h) hipHostFree(h);
    releaseDevice(in, d);
    h = nullptr; cap = 0;
    const size_t n = count + count / 4 + 64;
    HIP_TRY(hipHostMalloc((void**)&h, n * sizeof(T), hipHostMallocDefault));
    int rc = growDevice(in, d, n * sizeof(T), n * sizeof(T), Grow::SyncIfHeld); if (rc) return rc;
    cap = n;
    return 0;
}

int checkList(const Instance* in, const Basta* b, const int* ops, int opCount, const int* intervals, int intervalCount,
              int sizesIndex, int coalescentIndex) {
    if (opCount < 0 || intervalCount < 1 || (opCount > 0 && !ops) || !intervals) return BEAGLE_ERROR_OUT_OF_RANGE;
    if (badIndex(sizesIndex, in->eigenCount) || badIndex(coalescentIndex, b->bufferCount)) return BEAGLE_ERROR_OUT_OF_RANGE;
    // every operation belongs to one interval: offsets start at 0, do not decrease and end at the operation count
    if (intervals[0] != 0 || intervals[intervalCount - 1] != opCount) return BEAGLE_ERROR_OUT_OF_RANGE;
    for (int k = 1; k < intervalCount; k++) if (intervals[k] < intervals[k - 1]) return BEAGLE_ERROR_OUT_OF_RANGE;
    for (int k = 0; k < opCount; k++) {
        const int* op = ops + (size_t)k * BASTA_OP;
        if (badIndex(op[0], b->vectorCount) || badIndex(op[1], b->vectorCount) || badIndex(op[2], in->matrixCount) ||
            badIndex(op[5], b->vectorCount) || badIndex(op[7], b->maxIntervals)) return BEAGLE_ERROR_OUT_OF_RANGE;
        if (op[3] >= 0 && (badIndex(op[3], b->vectorCount) || badIndex(op[4], in->matrixCount) || badIndex(op[6], b->vectorCount)))
            return BEAGLE_ERROR_OUT_OF_RANGE;
    }
    return 0;
}

// Is the list a forest of chains (see the head of this file)?  Fills link = [n][2] {reader of the result or -1, inputs of that
// reader the list produces} and the starting operations.
bool analyse(Basta* b, const int* ops, int n, const int* intervals, int intervalCount, int* link, int* leaves, int* nLeaves) {
    b->writer.assign(b->vectorCount, -1); b->writes.assign(b->vectorCount, 0);
    b->intervalOf.resize(n);
    for (int t = 0; t + 1 < intervalCount; t++) for (int k = intervals[t]; k < intervals[t + 1]; k++) b->intervalOf[k] = t;
    for (int k = 0; k < n; k++) {
        const int* op = ops + (size_t)k * BASTA_OP;
        b->writer[op[0]] = k;
        if (++b->writes[op[0]] > 1) return false;
        if (op[3] >= 0) {
            if (++b->writes[op[5]] > 1 || ++b->writes[op[6]] > 1) return false;
            if (op[5] == op[0] || op[6] == op[0]) return false;
        }
    }
    for (int k = 0; k < n; k++) { link[2 * k] = -1; link[2 * k + 1] = 0; }
    std::vector<char> seen(b->vectorCount, 0);
    std::vector<int> produced(n, 0);
    for (int k = 0; k < n; k++) {
        const int* op = ops + (size_t)k * BASTA_OP;
        for (int side = 0; side < 2; side++) {
            const int x = op[side ? 3 : 1];
            if (x < 0) continue;
            if (b->writes[x] == 0) continue;                 // not written by this list: what the caller stored
            const int w = b->writer[x];
            if (w < 0 || ops[(size_t)w * BASTA_OP] != x) return false;          // an accumulation buffer read back
            if (b->intervalOf[w] >= b->intervalOf[k]) return false;            // written later, or in the same interval
            if (seen[x]) return false;                       // a second reader
            seen[x] = 1;
            link[2 * w] = k;
            produced[k]++;
        }
    }
    *nLeaves = 0;
    for (int k = 0; k < n; k++) {
        if (link[2 * k] >= 0) link[2 * k + 1] = produced[link[2 * k]];
        if (produced[k] == 0) leaves[(*nLeaves)++] = k;
    }
    return true;
}

// the list and its intervals on the device: nothing is sent when they are what the device already holds
int sendList(Instance* in, Basta* b, const int* ops, int n, const int* intervals, int intervalCount, bool* fresh) {
    const size_t opInts = (size_t)n * BASTA_OP;
    const bool same = b->opCount == n && b->intervalCount == intervalCount &&
                      memcmp(b->hIntervals, intervals, (size_t)intervalCount * sizeof(int)) == 0 &&
                      (opInts == 0 || memcmp(b->hOps, ops, opInts * sizeof(int)) == 0);
    *fresh = !same;
    if (same) return 0;
    HIP_TRY(hipEventSynchronize(b->sent));                   // (the previous list has left the pinned buffers)
    b->opCount = b->intervalCount = -1;
    int rc = growPair(in, b->hOps, b->dOps, b->opsCap, opInts + 1); if (rc) return rc;
    rc = growPair(in, b->hIntervals, b->dIntervals, b->intervalsCap, (size_t)intervalCount); if (rc) return rc;
    if (opInts) memcpy(b->hOps, ops, opInts * sizeof(int));
    memcpy(b->hIntervals, intervals, (size_t)intervalCount * sizeof(int));
    hipStream_t s = live(in);
    if (opInts) HIP_TRY(hipMemcpyAsync(b->dOps.p, b->hOps, opInts * sizeof(int), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(b->dIntervals.p, b->hIntervals, (size_t)intervalCount * sizeof(int), hipMemcpyHostToDevice, s));
    HIP_TRY(hipEventRecord(b->sent, s));
    b->opCount = n; b->intervalCount = intervalCount;
    b->statUploads++;
    return 0;
}

// The chains of beagleBastaSampleStates and their steps (kernels.h BastaStatesArgs) for a list analyse() accepts in which, moreover, no
// vector — one the caller stored included — is read twice: every vector then has one state.  false: not such a list.
bool planStates(Basta* b, const int* ops, int n, const int* intervals, int intervalCount) {
    std::vector<int> link((size_t)2 * n), leaves(n);
    int nLeaves = 0;
    if (!analyse(b, ops, n, intervals, intervalCount, link.data(), leaves.data(), &nLeaves)) return false;
    std::vector<char> read(b->vectorCount, 0);
    std::vector<int> down((size_t)2 * n, -1);                // per operation: the operations that wrote in1 / in2
    for (int k = 0; k < n; k++) {
        const int* op = ops + (size_t)k * BASTA_OP;
        for (int side = 0; side < 2; side++) {
            const int x = op[side ? 3 : 1];
            if (x < 0) continue;
            if (read[x]) return false;
            read[x] = 1;
            if (b->writes[x]) down[(size_t)2 * k + side] = b->writer[x];
        }
    }
    b->steps.clear(); b->chains.clear(); b->levelStart.clear(); b->chainAux.clear(); b->stepNumbers.clear();
    std::vector<int> level, next;                           // 4 * operation + 2 * (second input) + (its dest is a root)
    for (int k = 0; k < n; k++)
        if (link[2 * k] < 0) {                                               // nothing reads its result: a root
            level.push_back(4 * k + 1);
            if (ops[(size_t)k * BASTA_OP + 3] >= 0) level.push_back(4 * k + 3);
        }
    while (!level.empty()) {
        b->levelStart.push_back((int)b->chains.size() / 4);
        for (int c : level) {
            int k = c >> 2, side = (c >> 1) & 1;
            const int firstStep = (int)(b->steps.size() / 4);
            const int flags = (c & 1 ? mi355::BASTA_CHAIN_ROOT | (side == 0 ? mi355::BASTA_CHAIN_STORES_ROOT : 0) : 0);
            const int top = ops[(size_t)k * BASTA_OP];
            {
                const int* op = ops + (size_t)k * BASTA_OP;
                for (int v : {op[3] >= 0 ? op[side ? 5 : 6] : -1, op[7], side, 0}) b->chainAux.push_back(v);
            }
            for (;;) {
                const int* op = ops + (size_t)k * BASTA_OP;
                for (int v : {op[side ? 3 : 1], op[side ? 4 : 2], op[3] >= 0 ? op[side ? 6 : 5] : -1, b->intervalOf[k]}) b->steps.push_back(v);
                b->stepNumbers.push_back(ops[(size_t)intervals[b->intervalOf[k]] * BASTA_OP + 7]);      // (where e, f, g, h of the interval live)
                const int w = down[(size_t)2 * k + side];
                if (w < 0) break;                                            // what the caller stored
                if (ops[(size_t)w * BASTA_OP + 3] >= 0) { next.push_back(4 * w); next.push_back(4 * w + 2); break; }      // its chains: the next level
                k = w; side = 0;
            }
            for (int v : {firstStep, (int)(b->steps.size() / 4) - firstStep, top, flags}) b->chains.push_back(v);
        }
        level.swap(next); next.clear();
    }
    b->levelStart.push_back((int)b->chains.size() / 4);
    return true;
}

// the chains of the resident list on the device, planned and sent when the list has changed since
int residentPlan(Instance* in, Basta* b, const int* ops, int n, const int* intervals, int intervalCount) {
    if (b->planUpload == b->statUploads) return 0;
    b->planUpload = -1;
    if (!planStates(b, ops, n, intervals, intervalCount)) return BEAGLE_ERROR_NO_IMPLEMENTATION;
    hipStream_t s = live(in);
    size_t bytes = 0;
    for (const std::vector<int>* v : {&b->steps, &b->chains, &b->chainAux, &b->stepNumbers}) bytes += v->size() * sizeof(int);
    int rc = growDevice(in, b->dPlan, bytes, bytes, Grow::SyncIfHeld); if (rc) return rc;
    size_t at = 0;
    for (const std::vector<int>* v : {&b->steps, &b->chains, &b->chainAux, &b->stepNumbers}) {      // (16-byte records first)
        HIP_TRY(hipMemcpyAsync(b->dPlan.p + at, v->data(), v->size() * sizeof(int), hipMemcpyHostToDevice, s));
        at += v->size() * sizeof(int);
    }
    HIP_TRY(hipStreamSynchronize(s));                        // (the vectors are the plan's host copy: free to change from here on)
    b->planUpload = b->statUploads;
    return 0;
}

}  // namespace

int bastaSetPartials(Instance* in, int bufferIndex, const double* inPartials) {
    Basta* b = in->basta;
    if (badIndex(bufferIndex, b->vectorCount) || !inPartials) return BEAGLE_ERROR_OUT_OF_RANGE;
    return upload(in, b->vectors + (size_t)bufferIndex * in->S, inPartials, (size_t)in->S * sizeof(double));
}

int bastaGetPartials(Instance* in, int bufferIndex, double* outPartials) {
    Basta* b = in->basta;
    if (badIndex(bufferIndex, b->vectorCount) || !outPartials) return BEAGLE_ERROR_OUT_OF_RANGE;
    return download(in, outPartials, b->vectors + (size_t)bufferIndex * in->S, (size_t)in->S * sizeof(double));
}

void bastaFree(Instance* in) {
    Basta* b = in->basta;
    if (!b) return;
    if (in->stream) hipStreamSynchronize(in->stream);
    // (device memory is on the instance's allocation list and goes with it)
    if (b->hOps) hipHostFree(b->hOps);
    if (b->hIntervals) hipHostFree(b->hIntervals);
    if (b->hLengths) hipHostFree(b->hLengths);
    if (b->hLink) hipHostFree(b->hLink);
    if (b->hTimes) hipHostFree(b->hTimes);
    if (b->sent) hipEventDestroy(b->sent);
    delete b;
    in->basta = nullptr;
}

}  // namespace eng
}  // namespace mi355

using namespace mi355::eng;

extern "C" {

int beagleBastaAllocateCoalescentBuffers(int instance, int coalescentBufferCount, int maxCoalescentIntervalCount,
                                         int partialsBufferCount, int initial, int threadCount) {
    (void)threadCount;
    Instance* in = nullptr;
    int rc = bastaInstance(instance, &in); if (rc) return rc;
    if (coalescentBufferCount < 1 || maxCoalescentIntervalCount < 1 || partialsBufferCount < 1) return BEAGLE_ERROR_OUT_OF_RANGE;
    if (in->heldPre.held) { rc = executeHeldPre(in); if (rc) return rc; }
    const size_t S = (size_t)in->S;
    Basta* old = in->basta;
    Basta* b = old;
    if (!b) {
        b = new Basta();
        if (hipEventCreateWithFlags(&b->sent, hipEventDisableTiming) != hipSuccess) { delete b; return BEAGLE_ERROR_GENERAL; }
    }
    double* vectors = nullptr; double* buffers = nullptr; double* terms = nullptr;
    const size_t vBytes = (size_t)partialsBufferCount * S * sizeof(double);
    const size_t bBytes = (size_t)coalescentBufferCount * maxCoalescentIntervalCount * S * sizeof(double);
    const size_t tBytes = ((size_t)maxCoalescentIntervalCount + 1) * sizeof(double);
    rc = devAlloc(in, (void**)&vectors, vBytes);
    if (!rc) rc = devAlloc(in, (void**)&buffers, bBytes);
    if (!rc) rc = devAlloc(in, (void**)&terms, tBytes);
    if (rc) { if (!old) { hipEventDestroy(b->sent); delete b; } return rc; }
    hipStream_t s = live(in);
    HIP_TRY(hipMemsetAsync(vectors, 0, vBytes, s));
    HIP_TRY(hipMemsetAsync(buffers, 0, bBytes, s));
    HIP_TRY(hipMemsetAsync(terms, 0, tBytes, s));
    if (old && !initial && old->vectors)                     // a growing call keeps what setPartials (and the last update) stored
        HIP_TRY(hipMemcpyAsync(vectors, old->vectors, std::min(vBytes, (size_t)old->vectorCount * S * sizeof(double)), hipMemcpyDeviceToDevice, s));
    if (old) {
        HIP_TRY(hipStreamSynchronize(s));
        devFree(in, old->vectors); devFree(in, old->buffers); devFree(in, old->intervalLogL);
    }
    b->vectors = vectors; b->buffers = buffers; b->intervalLogL = terms;
    b->vectorCount = partialsBufferCount; b->maxIntervals = maxCoalescentIntervalCount; b->bufferCount = coalescentBufferCount;
    b->coalescentIndex = 0;
    in->basta = b;
    return BEAGLE_SUCCESS;
}

int beagleBastaUpdatePartials(int instance, const int* operations, int operationCount, const int* intervals, int intervalCount,
                              int populationSizesIndex, int coalescentProbabilityIndex) {
    Instance* in = nullptr;
    int rc = bastaInstance(instance, &in); if (rc) return rc;
    Basta* b = in->basta;
    if (!b) return BEAGLE_ERROR_NO_IMPLEMENTATION;
    rc = checkList(in, b, operations, operationCount, intervals, intervalCount, populationSizesIndex, coalescentProbabilityIndex);
    if (rc) return rc;
    if (in->heldPre.held) { rc = executeHeldPre(in); if (rc) return rc; }
    const int n = operationCount;
    bool fresh = false;
    rc = sendList(in, b, operations, n, intervals, intervalCount, &fresh); if (rc) return rc;
    // the chains of the list (3 n ints, staged and sent like the list itself)
    if (b->linkCap < (size_t)3 * n + 1) {
        HIP_TRY(hipStreamSynchronize(live(in)));
        if (b->hLink) hipHostFree(b->hLink);
        releaseDevice(in, b->dLink); releaseDevice(in, b->dTickets);
        b->hLink = nullptr; b->linkCap = 0;
        const size_t cap = 3 * ((size_t)n + n / 4 + 64);
        HIP_TRY(hipHostMalloc((void**)&b->hLink, cap * sizeof(int), hipHostMallocDefault));
        rc = growDevice(in, b->dLink, cap * sizeof(int), cap * sizeof(int), Grow::SyncIfHeld); if (rc) return rc;
        rc = growDevice(in, b->dTickets, cap / 3 * sizeof(unsigned), cap / 3 * sizeof(unsigned), Grow::SyncIfHeld); if (rc) return rc;
        b->linkCap = cap;
    }
    HIP_TRY(hipEventSynchronize(b->sent));
    int nLeaves = 0;
    const bool forest = n > 0 && analyse(b, operations, n, intervals, intervalCount, b->hLink, b->hLink + (size_t)2 * n, &nLeaves);
    b->coalescentIndex = coalescentProbabilityIndex;
    double* coalescent = b->buffers + (size_t)coalescentProbabilityIndex * b->maxIntervals * in->S;
    const double* sizes = in->freqs + (size_t)populationSizesIndex * in->S;
    hipStream_t s = live(in);
    HIP_TRY(hipMemsetAsync(coalescent, 0, (size_t)b->maxIntervals * sizeof(double), s));
    if (forest) {
        HIP_TRY(hipMemcpyAsync(b->dLink.p, b->hLink, (size_t)3 * n * sizeof(int), hipMemcpyHostToDevice, s));
        HIP_TRY(hipEventRecord(b->sent, s));
        HIP_TRY(hipMemsetAsync(b->dTickets.p, 0, (size_t)n * sizeof(unsigned), s));
    }
    CallTimer timer(in);
    rc = timer.start(); if (rc) return rc;
    int launches = 0;
    if (forest) {
        mi355::launchBastaChains(s, b->dOps.as<int>(), b->dLink.as<int>(), b->dLink.as<int>() + (size_t)2 * n, nLeaves, b->dTickets.as<unsigned>(), in->matrices, b->vectors, sizes, coalescent, in->S);
        launches = 1;
        b->statChainCalls++;
    } else {
        for (int t = 0; t + 1 < intervalCount; t++) {
            const int count = intervals[t + 1] - intervals[t];
            if (count <= 0) continue;
            mi355::launchBastaInterval(s, b->dOps.as<int>(), intervals[t], count, in->matrices, b->vectors, sizes, coalescent, in->S);
            launches++;
        }
        if (n > 0) b->statIntervalCalls++;
    }
    rc = timer.stop(launches); if (rc) return rc;
    HIP_TRY(hipGetLastError());
    return BEAGLE_SUCCESS;
}

int beagleBastaAccumulatePartials(int instance, const int* operations, int operationCount, const int* intervals, int intervalCount,
                                  const double* intervalLengths, int populationSizesIndex, int coalescentProbabilityIndex,
                                  double* outLogLikelihood) {
    Instance* in = nullptr;
    int rc = bastaInstance(instance, &in); if (rc) return rc;
    Basta* b = in->basta;
    if (!b) return BEAGLE_ERROR_NO_IMPLEMENTATION;
    rc = checkList(in, b, operations, operationCount, intervals, intervalCount, populationSizesIndex, coalescentProbabilityIndex);
    if (rc) return rc;
    if (!outLogLikelihood || (intervalCount > 1 && !intervalLengths)) return BEAGLE_ERROR_OUT_OF_RANGE;
    if (b->bufferCount < 5 || intervalCount - 1 > b->maxIntervals) return BEAGLE_ERROR_OUT_OF_RANGE;      // probabilities, e, f, g, h
    if (in->heldPre.held) { rc = executeHeldPre(in); if (rc) return rc; }
    bool fresh = false;
    rc = sendList(in, b, operations, operationCount, intervals, intervalCount, &fresh); if (rc) return rc;
    const int nIntervals = intervalCount - 1;
    rc = growPair(in, b->hLengths, b->dLengths, b->lengthsCap, (size_t)nIntervals + 1); if (rc) return rc;
    HIP_TRY(hipEventSynchronize(b->sent));
    if (nIntervals) memcpy(b->hLengths, intervalLengths, (size_t)nIntervals * sizeof(double));
    hipStream_t s = live(in);
    if (nIntervals) HIP_TRY(hipMemcpyAsync(b->dLengths.p, b->hLengths, (size_t)nIntervals * sizeof(double), hipMemcpyHostToDevice, s));
    HIP_TRY(hipEventRecord(b->sent, s));
    // e, f, g, h: the four lowest buffers that do not hold the coalescent probabilities
    double* efgh[4]; int at = 0;
    const size_t stride = (size_t)b->maxIntervals * in->S;
    for (int k = 0; k < b->bufferCount && at < 4; k++) if (k != coalescentProbabilityIndex) efgh[at++] = b->buffers + k * stride;
    double* total = b->intervalLogL + b->maxIntervals;
    mi355::launchBastaReduce(s, b->dOps.as<int>(), b->dIntervals.as<int>(), nIntervals, b->dLengths.as<double>(), b->vectors,
                             in->freqs + (size_t)populationSizesIndex * in->S, b->buffers + coalescentProbabilityIndex * stride,
                             efgh[0], efgh[1], efgh[2], efgh[3], b->intervalLogL, total, in->S);
    HIP_TRY(hipGetLastError());
    double logL = 0.0;
    rc = download(in, &logL, total, sizeof(double)); if (rc) return rc;
    if (in->asyncError) { const int e = in->asyncError.exchange(0); if (e) return e; }
    if (std::isnan(logL)) return BEAGLE_ERROR_FLOATING_POINT;
    outLogLikelihood[0] += logL;
    return BEAGLE_SUCCESS;
}

int beagleBastaGetBuffer(int instance, int index, double* out) {
    Instance* in = nullptr;
    int rc = bastaInstance(instance, &in); if (rc) return rc;
    Basta* b = in->basta;
    if (!b) return BEAGLE_ERROR_NO_IMPLEMENTATION;
    if (badIndex(index, b->bufferCount) || !out) return BEAGLE_ERROR_OUT_OF_RANGE;
    const size_t stride = (size_t)b->maxIntervals * in->S;
    const size_t count = index == b->coalescentIndex ? (size_t)b->maxIntervals : stride;
    return download(in, out, b->buffers + index * stride, count * sizeof(double));
}

int beagleBastaGetBufferLength(int instance, int index) {
    Instance* in = nullptr;
    int rc = bastaInstance(instance, &in); if (rc) return rc;
    Basta* b = in->basta;
    if (!b) return BEAGLE_ERROR_NO_IMPLEMENTATION;
    if (badIndex(index, b->bufferCount)) return BEAGLE_ERROR_OUT_OF_RANGE;
    return index == b->coalescentIndex ? b->maxIntervals : b->maxIntervals * in->S;
}

int beagleBastaStats(int instance, long* out4) {
    Instance* in = nullptr;
    int rc = bastaInstance(instance, &in); if (rc) return rc;
    Basta* b = in->basta;
    if (!b) return BEAGLE_ERROR_NO_IMPLEMENTATION;
    if (!out4) return BEAGLE_ERROR_OUT_OF_RANGE;
    out4[0] = b->statUploads; out4[1] = b->statChainCalls; out4[2] = b->statIntervalCalls; out4[3] = (long)b->vectorCount;
    return BEAGLE_SUCCESS;
}

int beagleBastaSampleStates(int instance, const int* operations, int operationCount, const int* intervals, int intervalCount,
                            int stateFrequenciesIndex, int replicateCount, unsigned long long seed, int flags,
                            unsigned char* outStates, double* outOccupancy, double* outChanges) {
    Instance* in = nullptr;
    int rc = bastaInstance(instance, &in); if (rc) return rc;
    Basta* b = in->basta;
    if (!b) return BEAGLE_ERROR_NO_IMPLEMENTATION;
    if (replicateCount < 1 || (flags & ~(BEAGLE_MI355_ANCESTRAL_MAP | BEAGLE_MI355_BASTA_STATES_AS_WRITTEN)) || in->S > 255 ||
        (!outStates && !outOccupancy && !outChanges)) return BEAGLE_ERROR_OUT_OF_RANGE;
    rc = checkList(in, b, operations, operationCount, intervals, intervalCount, stateFrequenciesIndex, b->coalescentIndex);
    if (rc) return rc;
    if (operationCount < 1) return BEAGLE_ERROR_OUT_OF_RANGE;
    if (in->heldPre.held) { rc = executeHeldPre(in); if (rc) return rc; }
    const int n = operationCount, S = in->S;
    const size_t V = (size_t)b->vectorCount, nIntervals = (size_t)intervalCount - 1;
    bool fresh = false;
    rc = sendList(in, b, operations, n, intervals, intervalCount, &fresh); if (rc) return rc;
    hipStream_t s = live(in);
    rc = residentPlan(in, b, operations, n, intervals, intervalCount); if (rc) return rc;
    const int levels = (int)b->levelStart.size() - 1;
    // replicates per pass: whole waves, at most 256 MiB of states (BEAGLE_MI355_BASTA_STATES_CHUNK=<n>: tests of chunk independence)
    const size_t R = (size_t)replicateCount;
    const size_t wanted = std::min<size_t>(std::max<size_t>(64, (256ull << 20) / V / 64 * 64), (size_t)65535 * 64);
    const size_t chunk = chunkSites("BEAGLE_MI355_BASTA_STATES_CHUNK", 64, wanted, R);
    const mi355::scratch::BastaStatesLayout L(V, chunk, nIntervals, (size_t)S, outStates != nullptr);
    rc = growScratch(in, b->statesDev, L.bytes()); if (rc) return rc;
    char* base = b->statesDev.p;
    mi355::BastaStatesArgs a{};
    a.steps = b->dPlan.as<int4>(); a.chains = b->dPlan.as<int4>() + b->steps.size() / 4;
    a.matrices = in->matrices; a.partials = b->vectors; a.freqs = in->freqs + (size_t)stateFrequenciesIndex * S;
    a.states = L.states.at(base);
    a.occupancy = outOccupancy ? L.occupancy.at(base) : nullptr;
    a.changes = outChanges ? L.changes.at(base) : nullptr;
    a.error = L.error.at(base);
    a.seed = seed; a.S = S; a.stride = (int)chunk;
    a.map = (flags & BEAGLE_MI355_ANCESTRAL_MAP) != 0; a.asWritten = (flags & BEAGLE_MI355_BASTA_STATES_AS_WRITTEN) != 0;
    uint8_t* dStage = L.stage.at(base);
    HIP_TRY(hipMemsetAsync(base + L.occupancy.offset, 0, L.bytes() - L.occupancy.offset, s));      // counters and the error word
    long chunks = 0;
    CallTimer timer(in);
    for (size_t r0 = 0; r0 < R; r0 += chunk, chunks++) {
        a.r0 = (int)r0; a.count = (int)std::min(chunk, R - r0);
        HIP_TRY(hipMemsetAsync(a.states, 0xFF, L.states.bytes(), s));
        rc = timer.start(); if (rc) return rc;               // (a timed call: a pair around every chunk's launches, not its copy-out)
        for (int lv = 0; lv < levels; lv++)
            mi355::launchBastaStates(s, a, b->levelStart[lv], b->levelStart[lv + 1] - b->levelStart[lv]);
        rc = timer.stop(levels); if (rc) return rc;
        HIP_TRY(hipGetLastError());
        if (outStates) {
            mi355::launchBastaStatesTranspose(s, a.states, (int)V, (int)chunk, a.count, dStage);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(outStates + r0 * V, dStage, (size_t)a.count * V, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));                // (the next chunk overwrites the stage)
        }
    }
    b->statStatesCalls++; b->statStatesLaunches = levels; b->statStatesChunks = chunks;
    // the counters and the error word in one copy
    const size_t tailWords = L.occupancy.count + L.changes.count + 1;
    std::vector<unsigned long long> tail(tailWords);
    rc = download(in, tail.data(), base + L.occupancy.offset, L.bytes() - L.occupancy.offset); if (rc) return rc;
    if (in->asyncError) { const int e = in->asyncError.exchange(0); if (e) return e; }
    if (outOccupancy) for (size_t i = 0; i < L.occupancy.count; i++) outOccupancy[i] = (double)tail[i];
    if (outChanges) for (size_t i = 0; i < L.changes.count; i++) outChanges[i] = (double)tail[L.occupancy.count + i];
    unsigned err = 0;
    memcpy(&err, &tail[L.occupancy.count + L.changes.count], sizeof(unsigned));
    return err ? BEAGLE_ERROR_FLOATING_POINT : BEAGLE_SUCCESS;
}

int beagleBastaStatesStats(int instance, long* out4) {
    Instance* in = nullptr;
    int rc = bastaInstance(instance, &in); if (rc) return rc;
    Basta* b = in->basta;
    if (!b) return BEAGLE_ERROR_NO_IMPLEMENTATION;
    if (!out4) return BEAGLE_ERROR_OUT_OF_RANGE;
    out4[0] = b->statStatesCalls; out4[1] = b->statStatesLaunches; out4[2] = b->statStatesChunks;
    out4[3] = b->planUpload == b->statUploads ? (long)b->chains.size() / 4 : 0;
    return BEAGLE_SUCCESS;
}

int beagleBastaGradient(int instance, const int* operations, int operationCount, const int* intervals, int intervalCount,
                        const double* intervalLengths, const double* intervalDistances, int populationSizesIndex,
                        int coalescentProbabilityIndex, int flags, double* outPopulationSizes, double* outMigration, double* outAdjoints) {
    Instance* in = nullptr;
    int rc = bastaInstance(instance, &in); if (rc) return rc;
    Basta* b = in->basta;
    if (!b) return BEAGLE_ERROR_NO_IMPLEMENTATION;
    if (flags != 0 || (!outPopulationSizes && !outMigration && !outAdjoints)) return BEAGLE_ERROR_OUT_OF_RANGE;
    rc = checkList(in, b, operations, operationCount, intervals, intervalCount, populationSizesIndex, coalescentProbabilityIndex);
    if (rc) return rc;
    if (operationCount < 1 || !intervalLengths || (outMigration && !intervalDistances)) return BEAGLE_ERROR_OUT_OF_RANGE;
    if (b->bufferCount < 5 || intervalCount - 1 > b->maxIntervals) return BEAGLE_ERROR_OUT_OF_RANGE;      // probabilities, e, f, g, h
    if (in->S > mi355::BASTA_GRADIENT_MAX_STATES) return BEAGLE_ERROR_NO_IMPLEMENTATION;
    if (in->heldPre.held) { rc = executeHeldPre(in); if (rc) return rc; }
    const int n = operationCount, S = in->S, nIntervals = intervalCount - 1;
    const size_t V = (size_t)b->vectorCount, entries = (size_t)S * S + S;
    bool fresh = false;
    rc = sendList(in, b, operations, n, intervals, intervalCount, &fresh); if (rc) return rc;
    rc = residentPlan(in, b, operations, n, intervals, intervalCount); if (rc) return rc;
    // lengths, then distances, through the pinned pair
    rc = growPair(in, b->hTimes, b->dTimes, b->timesCap, (size_t)2 * nIntervals); if (rc) return rc;
    HIP_TRY(hipEventSynchronize(b->sent));
    memcpy(b->hTimes, intervalLengths, (size_t)nIntervals * sizeof(double));
    if (intervalDistances) memcpy(b->hTimes + nIntervals, intervalDistances, (size_t)nIntervals * sizeof(double));
    hipStream_t s = live(in);
    HIP_TRY(hipMemcpyAsync(b->dTimes.p, b->hTimes, (size_t)(intervalDistances ? 2 : 1) * nIntervals * sizeof(double), hipMemcpyHostToDevice, s));
    HIP_TRY(hipEventRecord(b->sent, s));
    const mi355::scratch::BastaGradientLayout L(V, (size_t)nIntervals, (size_t)S);
    rc = growScratch(in, b->gradientDev, L.bytes()); if (rc) return rc;
    char* base = b->gradientDev.p;
    // e, f, g, h: the four lowest buffers that do not hold the coalescent probabilities, formed as beagleBastaAccumulatePartials forms them
    double* efgh[4]; int at = 0;
    const size_t stride = (size_t)b->maxIntervals * S;
    for (int k = 0; k < b->bufferCount && at < 4; k++) if (k != coalescentProbabilityIndex) efgh[at++] = b->buffers + k * stride;
    mi355::BastaGradientArgs a{};
    a.steps = b->dPlan.as<int4>(); a.chains = a.steps + b->steps.size() / 4; a.chainAux = a.chains + b->chains.size() / 4;
    a.stepNumbers = reinterpret_cast<const int*>(a.chainAux + b->chainAux.size() / 4);
    a.ops = b->dOps.as<int>(); a.intervals = b->dIntervals.as<int>();
    a.matrices = in->matrices; a.partials = b->vectors; a.sizes = in->freqs + (size_t)populationSizesIndex * S;
    a.coalescent = b->buffers + coalescentProbabilityIndex * stride;
    a.e = efgh[0]; a.f = efgh[1]; a.g = efgh[2]; a.h = efgh[3];
    a.lengths = b->dTimes.as<double>(); a.distances = intervalDistances ? b->dTimes.as<double>() + nIntervals : nullptr;
    a.adjoints = L.adjoints.at(base); a.w = L.w.at(base); a.parts = L.parts.at(base); a.out = L.out.at(base);
    a.S = S;
    const int levels = (int)b->levelStart.size() - 1;
    CallTimer timer(in);
    rc = timer.start(); if (rc) return rc;
    mi355::launchBastaReduce(s, a.ops, a.intervals, nIntervals, a.lengths, b->vectors, a.sizes, a.coalescent, efgh[0], efgh[1], efgh[2], efgh[3],
                             b->intervalLogL, b->intervalLogL + b->maxIntervals, S);
    HIP_TRY(hipMemsetAsync(a.adjoints, 0, L.adjoints.bytes(), s));           // (a vector the list does not touch, a root coalescence's dest)
    for (int lv = 0; lv < levels; lv++) mi355::launchBastaGradientSweep(s, a, b->levelStart[lv], b->levelStart[lv + 1] - b->levelStart[lv]);
    mi355::launchBastaGradientReduce(s, a, nIntervals);
    const int launches = levels + 4;                         // the levels, the two launches behind e, f, g, h and the two reductions
    rc = timer.stop(launches); if (rc) return rc;
    HIP_TRY(hipGetLastError());
    b->statGradientCalls++; b->statGradientLaunches = launches; b->statGradientLevels = levels;
    std::vector<double> out(entries), adjoints(outAdjoints ? V * S : 0);
    if (outAdjoints) HIP_TRY(hipMemcpyAsync(adjoints.data(), a.adjoints, adjoints.size() * sizeof(double), hipMemcpyDeviceToHost, s));
    rc = download(in, out.data(), a.out, entries * sizeof(double)); if (rc) return rc;
    if (in->asyncError) { const int e = in->asyncError.exchange(0); if (e) return e; }
    bool finite = true;
    if (outMigration) for (size_t i = 0; i < (size_t)S * S; i++) { outMigration[i] = out[i]; finite = finite && std::isfinite(out[i]); }
    if (outPopulationSizes) for (int i = 0; i < S; i++) { outPopulationSizes[i] = out[(size_t)S * S + i]; finite = finite && std::isfinite(out[(size_t)S * S + i]); }
    if (outAdjoints) for (size_t i = 0; i < adjoints.size(); i++) { outAdjoints[i] = adjoints[i]; finite = finite && std::isfinite(adjoints[i]); }
    return finite ? BEAGLE_SUCCESS : BEAGLE_ERROR_FLOATING_POINT;
}

int beagleBastaGradientStats(int instance, long* out4) {
    Instance* in = nullptr;
    int rc = bastaInstance(instance, &in); if (rc) return rc;
    Basta* b = in->basta;
    if (!b) return BEAGLE_ERROR_NO_IMPLEMENTATION;
    if (!out4) return BEAGLE_ERROR_OUT_OF_RANGE;
    out4[0] = b->statGradientCalls; out4[1] = b->statGradientLaunches; out4[2] = b->statGradientLevels;
    out4[3] = b->planUpload == b->statUploads ? (long)b->chains.size() / 4 : 0;
    return BEAGLE_SUCCESS;
}

int beagleBastaUpdatePartialsGrad(int instance, const int* operations, int operationCount, const int* intervals, int intervalCount,
                                  int populationSizesIndex, int coalescentProbabilityIndex) {
    (void)instance; (void)operations; (void)operationCount; (void)intervals; (void)intervalCount; (void)populationSizesIndex; (void)coalescentProbabilityIndex;
    return BEAGLE_ERROR_NO_IMPLEMENTATION;
}

int beagleBastaUpdateTransitionMatricesGrad(int instance, const int* transitionMatrixIndices, const double* branchLengths, int count) {
    (void)instance; (void)transitionMatrixIndices; (void)branchLengths; (void)count;
    return BEAGLE_ERROR_NO_IMPLEMENTATION;
}

int beagleBastaAccumulatePartialsGrad(int instance, const int* operations, int operationCount, const int* intervals, int intervalCount,
                                      const double* intervalLengths, int populationSizesIndex, int coalescentProbabilityIndex,
                                      double* outGradient) {
    (void)instance; (void)operations; (void)operationCount; (void)intervals; (void)intervalCount; (void)intervalLengths;
    (void)populationSizesIndex; (void)coalescentProbabilityIndex; (void)outGradient;
    return BEAGLE_ERROR_NO_IMPLEMENTATION;
}

}  // extern "C"
