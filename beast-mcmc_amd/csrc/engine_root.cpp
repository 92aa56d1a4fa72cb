// engine_root.cpp — the calls that observe a likelihood: root sums (plain, by partition, left on the device, all-reduced over the
// ranks of a communicator), the polled result page they arrive through, and the site log-likelihoods with their prefetch.
#include "engine_internal.h"

using mi355::shardedStates;
using mi355::shardedCategories;
using namespace mi355::eng;

namespace {

// The site log-likelihoods of the root sum just enqueued, on their way to the host before anybody asks (Instance::hSites): called by the
// whole-alignment root entry points right behind their last launch.  A caller that read the site values after each of the last two such
// sums (BeagleTreeLikelihood.java:1050 does after every one) is served; the copy is a kernel of the stream (k_hostCopies writing through
// the buffer's device mapping: the next evaluation's launches queue behind 800 KB of PCIe writes at the metric's size, ~20 us, which the
// caller's own traversal covers), its end an event.
int sitePrefetchAfterRoot(Instance* in) {
    if (!in->siteReadSinceRoot) in->siteReadStreak = 0;            // the sum before this one: nobody looked at its site values
    in->siteReadSinceRoot = false;
    const size_t bytes = (size_t)in->P * sizeof(double);
    if (!in->sitePrefetch || in->siteReadStreak < 2 || bytes > ((size_t)1 << 30)) return 0;
    if (!in->hSites) {
        if (hipHostMalloc((void**)&in->hSites, bytes, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess) { in->hSites = nullptr; in->sitePrefetch = false; (void)hipGetLastError(); return 0; }
        if (hipHostGetDevicePointer((void**)&in->hSitesDev, in->hSites, 0) != hipSuccess ||
            hipEventCreateWithFlags(&in->siteEvent, hipEventDisableTiming) != hipSuccess) { in->sitePrefetch = false; (void)hipGetLastError(); return 0; }
    }
    const unsigned blocks = (unsigned)((bytes + 4095) / 4096);
    mi355::HostCopyList L;
    L.n = 1;
    L.e[0].dst = in->hSitesDev; L.e[0].src = (const char*)in->siteLogL; L.e[0].bytes = (unsigned)bytes; L.e[0].firstBlock = 0;
    mi355::launchHostCopies(live(in), L, (int)blocks);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(in->siteEvent, live(in)));
    in->sitePrefetched = true;
    return 0;
}
// ... and the other end: true when `out` (nullable: the caller reads Instance::hSites itself) has the site values of the last root sum
bool sitePrefetchTake(Instance* in, double* out) {
    if (!in->siteReadSinceRoot) { in->siteReadStreak++; in->siteReadSinceRoot = true; }
    if (!in->sitePrefetched) return false;
    const auto t0 = std::chrono::steady_clock::now();
    unsigned spins = 0;
    hipError_t st;
    while ((st = hipEventQuery(in->siteEvent)) == hipErrorNotReady) {
        __builtin_ia32_pause();
        if ((++spins & 0xff) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(20)) { st = hipEventSynchronize(in->siteEvent); break; }
    }
    if (st != hipSuccess) { (void)hipGetLastError(); in->sitePrefetched = false; return false; }      // (the stream-ordered download then says what went wrong)
    if (out) memcpy(out, in->hSites, (size_t)in->P * sizeof(double));
    in->statSitePrefetched++;
    return true;
}

// What a root sum reads besides the root's partials, by index, into descriptor `d` (RootFused, RootFusedPart, RootPart: the same four
// fields): category weights, state frequencies, the cumulative scale buffer (BEAGLE_OP_NONE: none; made to exist) and whether that
// buffer holds raw factors.
template <class Desc>
int rootModel(Instance* in, int wIdx, int fIdx, int cumIdx, Desc* d) {
    if (badIndex(wIdx, in->eigenCount) || badIndex(fIdx, in->eigenCount) || (cumIdx != BEAGLE_OP_NONE && badIndex(cumIdx, in->scaleCount)))
        return BEAGLE_ERROR_OUT_OF_RANGE;
    d->catWeights = in->weights + (size_t)wIdx * in->C; d->freqs = in->freqs + (size_t)fIdx * in->S; d->cum = nullptr; d->cumIsRaw = 0;
    if (cumIdx != BEAGLE_OP_NONE) {
        int rc = ensureScale(in, cumIdx); if (rc) return rc;
        d->cum = in->scale[cumIdx]; d->cumIsRaw = in->scaleIsRaw[cumIdx];
    }
    return 0;
}

int rootEnqueue(Instance* in, int rootIdx, int wIdx, int fIdx, int cumIdx, int part, double* dOut,
                unsigned long long* flag = nullptr, unsigned long long seq = 0) {
    // part < 0: the whole pattern range
    in->sitePrefetched = false;                           // (whatever this sum writes into siteLogL, the host's copy is of the one before)
    if (badIndex(rootIdx, in->partialsCount)) return BEAGLE_ERROR_OUT_OF_RANGE;
    { int rcv = materializeVirtual(in, rootIdx); if (rcv) return rcv; }
    if (!in->partials[rootIdx] || badIndex(wIdx, in->eigenCount) ||
        badIndex(fIdx, in->eigenCount) || (part >= 0 && badIndex(part, in->partitionCount))) return BEAGLE_ERROR_OUT_OF_RANGE;
    const int pStart = part < 0 ? 0 : in->partStart[part], pEnd = part < 0 ? in->P : in->partEnd[part];
    if (pEnd <= pStart) {                                 // an empty partition (a shard that holds none of its patterns) contributes 0
        // (whatever its cumulative index: rootModel's checks come after this return, as they always have)
        HIP_TRY(hipMemsetAsync(dOut, 0, sizeof(double), live(in)));
        return 0;
    }
    mi355::RootFused rf;                                  // (the held walk's root slice takes all of it, the root kernels the model part)
    memset(&rf, 0, sizeof(rf));
    { int rc = rootModel(in, wIdx, fIdx, cumIdx, &rf); if (rc) return rc; }
    if (in->pendingWalk.valid && part < 0 && !in->tiled) {
        // the walk that computes this root is still held back: launch it with the root's slice finishing the evaluation
        const Instance::PendingWalk& pw = in->pendingWalk;
        int seg = -1;
        for (size_t i = 0; i < pw.finalStore.size(); i++) if (pw.finalStore[i] == rootIdx) seg = (int)i;
        // (a partitioned instance's walk — held for the by-partition root call — finishes this whole-range root only if the slice's
        // partition IS the whole range: otherwise live() launches the walk as it is and the plain root kernel below covers [0, P))
        if (seg >= 0 && in->partitionCount > 1) {
            const int k = pw.finalPart[(size_t)seg];
            if (in->partStart[k] != 0 || in->partEnd[k] != in->P) seg = -1;
        }
        if (seg >= 0) {
            rf.patternWeights = in->patternWeights; rf.siteLogL = in->siteLogL; rf.blockSums = in->blockSums; rf.counter = in->rootCounter;
            rf.out = dOut; rf.flag = flag; rf.seq = seq; rf.rootSeg = seg; rf.groups = (in->P + 127) / 128;
            return flushWalk(in, &rf);
        }
    }
    if (in->tiled) {
        mi355::launchRootSiteTiled(live(in), in->partials[rootIdx], rf.catWeights, rf.freqs, rf.cum, rf.cumIsRaw, in->patternWeights, in->siteLogL,
                                   in->blockSums, in->P, in->S, in->C, pStart, pEnd);
        mi355::launchRootFinal(live(in), in->blockSums, mi355::rootSiteTiledBlocks(pEnd - pStart), dOut, flag, seq);
    } else if (in->walk && in->fuseLaunches) {
        mi355::launchRootLogLikelihood4W(live(in), in->partials[rootIdx], rf.catWeights, rf.freqs, rf.cum, rf.cumIsRaw, in->patternWeights, in->siteLogL,
                                         in->blockSums, dOut, in->P, in->C, pStart, pEnd, flag, seq, in->rootCounter);
    } else {
        mi355::launchRootLogLikelihood(live(in), in->partials[rootIdx], rf.catWeights, rf.freqs, rf.cum, rf.cumIsRaw, in->patternWeights, in->siteLogL,
                                       in->blockSums, dOut, in->P, in->S, in->C, pStart, pEnd, flag, seq, in->fuseLaunches ? in->rootCounter : nullptr);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

// The last reduction kernel of a call writes its result and then `seq` into mapped host memory (Instance::hResult); the kernel
// is the last thing in the (in-order) stream, so seeing the number means everything before it has completed.  Polled — a stream
// synchronisation costs a wake-up per evaluation — for 20 ms, then blocking (a long evaluation, another rank's, or an error).
int waitResult(Instance* in, unsigned long long seq) {
    // (class indices a topology move left to build: a step of that work while the device computes — behind a full evaluation, which takes
    // longer than a pass over the patterns; a partial update's result is not kept waiting)
    if (!in->repeatQueue.empty() && in->lastPlanCached) repeatsIdle(in);
    volatile unsigned long long* flag = (volatile unsigned long long*)(in->hResult + 8);
    const auto t0 = std::chrono::steady_clock::now();
    unsigned spins = 0;
    while (*flag != seq) {
        __builtin_ia32_pause();
        if ((++spins & 0xfff) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(20)) break;
    }
    if (*flag != seq) HIP_TRY(hipStreamSynchronize(live(in)));
    if (*flag != seq) return BEAGLE_ERROR_GENERAL;
    std::atomic_thread_fence(std::memory_order_acquire);
    { const int rc = in->asyncError.exchange(0); if (rc) return rc; }
    return 0;
}

// How a root entry point ends: the sum goes to the caller, and a NaN is reported as an error
int finishSum(double v, double* outSum) {
    *outSum = v;
    return (v != v) ? BEAGLE_ERROR_FLOATING_POINT : BEAGLE_SUCCESS;
}
// ... by partition: the n values (to outByPartition unless they are there already: null) and their sum in index order
int finishSum(const double* values, int n, double* outByPartition, double* outSum) {
    double tot = 0.0;
    for (int k = 0; k < n; k++) { if (outByPartition) outByPartition[k] = values[k]; tot += values[k]; }
    return finishSum(tot, outSum);
}

}  // namespace

// per-partition root sums of ONE (single-GPU) instance left on the device: deviceOut[k], k < partitionCount
static int rootByPartitionDevice(int instance, const int* bufferIndices, const int* categoryWeightsIndices, const int* stateFrequenciesIndices,
                                 const int* cumulativeScaleIndices, const int* partitionIndices, int partitionCount, double* deviceOut) {
    GET_INSTANCE(instance);
    for (int k = 0; k < partitionCount; k++) {
        int rc = rootEnqueue(in, bufferIndices[k], categoryWeightsIndices[k], stateFrequenciesIndices[k], cumulativeScaleIndices[k],
                             partitionIndices[k], deviceOut + k);
        if (rc) return rc;
    }
    return 0;
}

namespace mi355 {
int publishAndWait(int instance, const double* dValues, int count, double* out) {
    GET_INSTANCE_KEEP_PENDING(instance);
    if (!dValues || !out || count < 1 || count > 480) return BEAGLE_ERROR_OUT_OF_RANGE;
    const unsigned long long seq = ++in->resultSeq;
    mi355::launchPublish(live(in), dValues, count, in->hResultDev + 16, (unsigned long long*)(in->hResultDev + 8), seq);
    HIP_TRY(hipGetLastError());
    { const int rcw = waitResult(in, seq); if (rcw) return rcw; }
    ringIdle(in);
    memcpy(out, in->hResult + 16, (size_t)count * sizeof(double));
    return BEAGLE_SUCCESS;
}
int takeAsyncError(int instance) {
    Instance* in = lookup(instance);
    if (!in) return BEAGLE_ERROR_UNINITIALIZED_INSTANCE;
    return in->asyncError.exchange(0);
}
}  // namespace mi355

extern "C" {

int beagleCalculateRootLogLikelihoods(int instance, const int* bufferIndices, const int* categoryWeightsIndices,
                                      const int* stateFrequenciesIndices, const int* cumulativeScaleIndices,
                                      int count, double* outSumLogLikelihood) {
    if (mi355::isShardedHandle(instance)) { if (count != 1) return BEAGLE_ERROR_NO_IMPLEMENTATION;
        double v = 0.0;
        const int rc = mi355::shardedRootReduce(instance, 1, [&](int h, double* dOut) { return beagleMi355CalculateRootLogLikelihoodsDevice(h, bufferIndices[0],
                              categoryWeightsIndices[0], stateFrequenciesIndices[0], cumulativeScaleIndices[0], dOut); }, &v);
        return rc ? rc : finishSum(v, outSumLogLikelihood); }
    GET_INSTANCE_KEEP_PENDING(instance);                      // (reads a post-order buffer: a held-back pre-order list writes none)
    if (count != 1) return BEAGLE_ERROR_NO_IMPLEMENTATION;   // BEAST always passes 1 (BeagleTreeLikelihood.java:1038)
    if (bufferIndices && heldWrites(in, bufferIndices[0])) { int rcp = executeHeldPre(in); if (rcp) return rcp; }
    // the reduction kernel writes the sum and then a sequence number into mapped host memory; the kernel is the last
    // thing in the (in-order) stream, so seeing the number means everything before it has completed
    const unsigned long long seq = ++in->resultSeq;
    int rc = rootEnqueue(in, bufferIndices[0], categoryWeightsIndices[0], stateFrequenciesIndices[0],
                         cumulativeScaleIndices[0], -1, in->hResultDev, (unsigned long long*)(in->hResultDev + 8), seq);
    if (rc) return rc;
    rc = sitePrefetchAfterRoot(in); if (rc) return rc;
    { const int rcw = waitResult(in, seq); if (rcw) return rcw; }
    ringIdle(in);   // everything staged so far has been consumed
    return finishSum(in->hResult[0], outSumLogLikelihood);
}

int beagleCalculateRootLogLikelihoodsByPartition(int instance, const int* bufferIndices, const int* categoryWeightsIndices,
                                      const int* stateFrequenciesIndices, const int* cumulativeScaleIndices,
                                      const int* partitionIndices, int partitionCount, int count,
                                      double* outByPartition, double* outSum) {
    if (mi355::isShardedHandle(instance)) { if (count != 1) return BEAGLE_ERROR_NO_IMPLEMENTATION;
        const int rc = mi355::shardedRootReduce(instance, partitionCount, [&](int h, double* dOut) { return rootByPartitionDevice(h, bufferIndices, categoryWeightsIndices,
                              stateFrequenciesIndices, cumulativeScaleIndices, partitionIndices, partitionCount, dOut); }, outByPartition);
        return rc ? rc : finishSum(outByPartition, partitionCount, nullptr, outSum); }
    GET_INSTANCE(instance);
    if (count != 1) return BEAGLE_ERROR_NO_IMPLEMENTATION;
    if (partitionCount < 1 || partitionCount > 512) return BEAGLE_ERROR_OUT_OF_RANGE;
    in->sitePrefetched = false; in->siteReadStreak = 0;          // (per-partition sums rewrite siteLogL piece by piece: always the stream-ordered download)
    if (!in->tiled && partitionCount <= 480) {
        // 4-state walk instances, up to eight partitions: 128-pattern groups with the assembly loop's lane map (k_rootSite4WParts) — and
        // when the walk that computes these roots is still held back (engine_walk.cpp launchWalk) and its last slices are exactly the
        // named roots, the slices' own epilogues do it: no root launch at all
        const bool groups128 = in->walk && in->fuseLaunches && partitionCount <= mi355::ROOT_MAX_PARTS;
        if (groups128 && in->pendingWalk.valid && in->fuseRootParts) {
            const Instance::PendingWalk& pw = in->pendingWalk;
            mi355::RootFusedParts rp;
            memset(&rp, 0, sizeof(rp));
            bool ok = (int)pw.sinkRows.size() == partitionCount && in->partitionCount > 1;
            int off = 0;
            for (int k = 0; k < partitionCount && ok; k++) {
                const int rootIdx = bufferIndices[k], wIdx = categoryWeightsIndices[k], fIdx = stateFrequenciesIndices[k], cumIdx = cumulativeScaleIndices[k], part = partitionIndices[k];
                if (badIndex(rootIdx, in->partialsCount) || badIndex(part, in->partitionCount)) { ok = false; break; }
                int seg = -1;
                for (int row : pw.sinkRows) if (pw.finalStore[(size_t)row] == rootIdx && pw.finalPart[(size_t)row] == part) seg = row;
                for (int j = 0; j < k; j++) if (rp.p[j].rootSeg == seg) seg = -1;                       // (a root named twice: the plain path)
                if (seg < 0) { ok = false; break; }
                mi355::RootFusedPart& q = rp.p[k];
                const int rc = rootModel(in, wIdx, fIdx, cumIdx, &q);
                if (rc == BEAGLE_ERROR_OUT_OF_RANGE) { ok = false; break; }      // (the plain path reports it)
                if (rc) return rc;
                q.rootSeg = seg; q.blockOff = off; q.groups = (std::max(0, in->partEnd[part] - in->partStart[part]) + 127) / 128;
                off += q.groups;
            }
            if (ok && off > 0) {
                rp.n = partitionCount; rp.totalGroups = off;
                const unsigned long long seq = ++in->resultSeq;
                mi355::RootFused rf;
                memset(&rf, 0, sizeof(rf));
                rf.rootSeg = -1;
                rf.patternWeights = in->patternWeights; rf.siteLogL = in->siteLogL; rf.blockSums = in->blockSums; rf.counter = in->rootCounter;
                rf.out = in->hResultDev + 16; rf.flag = (unsigned long long*)(in->hResultDev + 8); rf.seq = seq;
                if (!in->rootPartsDev) { int rca = devAlloc(in, (void**)&in->rootPartsDev, Instance::ROOT_PARTS_TABLES * sizeof(rp)); if (rca) return rca; }
                int table = -1;
                for (int t = 0; t < Instance::ROOT_PARTS_TABLES; t++)
                    if (in->rootPartsShadow[t].size() == sizeof(rp) && memcmp(in->rootPartsShadow[t].data(), &rp, sizeof(rp)) == 0) table = t;
                if (table < 0) {
                    table = in->rootPartsNext; in->rootPartsNext = (table + 1) % Instance::ROOT_PARTS_TABLES;
                    KeepWalkHeld keep(in);                           // (the held walk's own input)
                    const int rcu = upload(in, in->rootPartsDev + table, &rp, sizeof(rp));
                    if (rcu) return rcu;
                    in->rootPartsShadow[table].assign((const char*)&rp, (const char*)&rp + sizeof(rp));
                }
                rf.parts = in->rootPartsDev + table;
                in->statRootPartsFused++;
                { const int rcw = flushWalk(in, &rf); if (rcw) return rcw; }
                HIP_TRY(hipGetLastError());
                { const int rcw = waitResult(in, seq); if (rcw) return rcw; }
                ringIdle(in);
                return finishSum(in->hResult + 16, partitionCount, outByPartition, outSum);
            }
        }
        // all partitions in ONE pair of launches per eight of them, the sums written straight into mapped host memory behind a
        // sequence word the host polls (as calculateRootLogLikelihoods): no device-to-host copy, no stream synchronisation
        std::vector<mi355::RootParts> chunks((partitionCount + mi355::ROOT_MAX_PARTS - 1) / mi355::ROOT_MAX_PARTS);
        int blockOff = 0;
        for (int k = 0; k < partitionCount; k++) {
            const int rootIdx = bufferIndices[k], wIdx = categoryWeightsIndices[k], fIdx = stateFrequenciesIndices[k], cumIdx = cumulativeScaleIndices[k], part = partitionIndices[k];
            if (badIndex(rootIdx, in->partialsCount) || badIndex(part, in->partitionCount)) return BEAGLE_ERROR_OUT_OF_RANGE;
            { int rcv = materializeVirtual(in, rootIdx); if (rcv) return rcv; }
            if (!in->partials[rootIdx]) return BEAGLE_ERROR_OUT_OF_RANGE;
            mi355::RootParts& ch = chunks[k / mi355::ROOT_MAX_PARTS];
            mi355::RootPart& q = ch.p[k % mi355::ROOT_MAX_PARTS];
            ch.n = k % mi355::ROOT_MAX_PARTS + 1;
            q.root = in->partials[rootIdx];
            { int rc = rootModel(in, wIdx, fIdx, cumIdx, &q); if (rc) return rc; }
            q.pStart = in->partStart[part]; q.pEnd = in->partEnd[part]; q.blockOff = blockOff;
            blockOff += (std::max(0, q.pEnd - q.pStart) + (groups128 ? 127 : 255)) / (groups128 ? 128 : 256);
        }
        const unsigned long long seq = ++in->resultSeq;
        for (size_t c = 0; c < chunks.size(); c++) {
            const bool last = c + 1 == chunks.size();
            if (groups128)
                mi355::launchRootLogLikelihoodParts4W(live(in), chunks[c], in->patternWeights, in->siteLogL, in->blockSums, in->hResultDev + 16, in->P, in->C,
                                                      (unsigned long long*)(in->hResultDev + 8), seq, in->rootCounter);
            else
            mi355::launchRootLogLikelihoodParts(live(in), chunks[c], in->patternWeights, in->siteLogL, in->blockSums,
                                                in->hResultDev + 16 + c * mi355::ROOT_MAX_PARTS, in->P, in->S, in->C,
                                                last ? (unsigned long long*)(in->hResultDev + 8) : nullptr, seq, in->fuseLaunches ? in->rootCounter : nullptr);
        }
        HIP_TRY(hipGetLastError());
        { const int rcw = waitResult(in, seq); if (rcw) return rcw; }
        ringIdle(in);
        return finishSum(in->hResult + 16, partitionCount, outByPartition, outSum);
    }
    for (int k = 0; k < partitionCount; k++) {
        int rc = rootEnqueue(in, bufferIndices[k], categoryWeightsIndices[k], stateFrequenciesIndices[k],
                             cumulativeScaleIndices[k], partitionIndices[k], in->dResult + k);
        if (rc) return rc;
    }
    int rc = download(in, in->hResult, in->dResult, (size_t)partitionCount * sizeof(double));
    return rc ? rc : finishSum(in->hResult, partitionCount, outByPartition, outSum);
}

int beagleGetSiteLogLikelihoods(int instance, double* out) {
    if (mi355::isShardedHandle(instance)) {
        return mi355::shardedGetPerPatternDoubles(instance, out, 1, 1, [&](int h, double* v) { return beagleGetSiteLogLikelihoods(h, v); });
    }
    GET_INSTANCE(instance);
    if (!out) return BEAGLE_ERROR_OUT_OF_RANGE;
    if (sitePrefetchTake(in, out)) return BEAGLE_SUCCESS;         // (already on the host: Instance::hSites)
    return download(in, out, in->siteLogL, (size_t)in->P * sizeof(double));
}

int beagleMi355GetSiteLogLikelihoodsPinned(int instance, const double** outPinned, long* outCount) {
    if (mi355::isShardedHandle(instance)) return BEAGLE_ERROR_NO_IMPLEMENTATION;
    GET_INSTANCE(instance);
    if (!outPinned || !outCount) return BEAGLE_ERROR_OUT_OF_RANGE;
    const size_t bytes = (size_t)in->P * sizeof(double);
    if (sitePrefetchTake(in, nullptr)) { *outPinned = in->hSites; *outCount = in->P; return BEAGLE_SUCCESS; }      // (valid until the next root sum)
    if (bytes > RING_BYTES) return BEAGLE_ERROR_NO_IMPLEMENTATION;
    HIP_TRY(hipMemcpyAsync(in->hRing, in->siteLogL, bytes, hipMemcpyDeviceToHost, live(in)));     // (the ring is pinned; everything staged in it
    HIP_TRY(hipStreamSynchronize(live(in)));                                                      //  has been consumed once the stream is idle)
    in->ringHead = (bytes + 255) & ~(size_t)255;
    *outPinned = (const double*)in->hRing; *outCount = in->P;
    return BEAGLE_SUCCESS;
}

int beagleMi355CalculateRootLogLikelihoodsDevice(int instance, int bufferIndex, int categoryWeightsIndex,
                                                 int stateFrequenciesIndex, int cumulativeScaleIndex, void* deviceOut) {
    if (mi355::isShardedHandle(instance)) { return BEAGLE_ERROR_NO_IMPLEMENTATION; }
    GET_INSTANCE_KEEP_PENDING(instance);
    if (!deviceOut) return BEAGLE_ERROR_OUT_OF_RANGE;
    if (heldWrites(in, bufferIndex)) { int rcp = executeHeldPre(in); if (rcp) return rcp; }
    const int rc = rootEnqueue(in, bufferIndex, categoryWeightsIndex, stateFrequenciesIndex, cumulativeScaleIndex, -1, (double*)deviceOut);
    return rc ? rc : sitePrefetchAfterRoot(in);
}

// ---- one process per GPU: the collective inside the engine -------------------------------------------------------------
int beagleMi355GetCommUniqueId(void* out128) {
    static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId is 128 bytes");
    if (!out128) return BEAGLE_ERROR_OUT_OF_RANGE;
    ncclUniqueId id;
    if (ncclGetUniqueId(&id) != ncclSuccess) return BEAGLE_ERROR_GENERAL;
    memcpy(out128, &id, sizeof(id));
    return BEAGLE_SUCCESS;
}

int beagleMi355CommInit(int instance, const void* uniqueId128, int rank, int rankCount) {
    if (mi355::isShardedHandle(instance)) return BEAGLE_ERROR_NO_IMPLEMENTATION;      // (resource G+1 owns its own communicator)
    GET_INSTANCE(instance);
    if (!uniqueId128 || rankCount < 1 || rank < 0 || rank >= rankCount) return BEAGLE_ERROR_OUT_OF_RANGE;
    HIP_TRY(hipStreamSynchronize(live(in)));
    if (in->comm) { ncclCommDestroy(in->comm); in->comm = nullptr; in->commRanks = 0; }
    ncclUniqueId id;
    memcpy(&id, uniqueId128, sizeof(id));
    if (ncclCommInitRank(&in->comm, rankCount, id, rank) != ncclSuccess) { in->comm = nullptr; return BEAGLE_ERROR_GENERAL; }
    in->commRanks = rankCount;
    return BEAGLE_SUCCESS;
}

int beagleMi355CommInfo(int instance, int* outRanks) {
    if (!outRanks) return BEAGLE_ERROR_OUT_OF_RANGE;
    if (mi355::isShardedHandle(instance)) { *outRanks = mi355::shardedCommRanks(instance); return BEAGLE_SUCCESS; }
    Instance* in = lookup(instance);
    if (!in) return BEAGLE_ERROR_UNINITIALIZED_INSTANCE;
    int n = 0;
    if (in->comm && ncclCommCount(in->comm, &n) != ncclSuccess) return BEAGLE_ERROR_GENERAL;     // (what RCCL says, not what the caller asked for)
    *outRanks = n;
    return BEAGLE_SUCCESS;
}

int beagleMi355CalculateRootLogLikelihoodsAllReduce(int instance, int bufferIndex, int categoryWeightsIndex, int stateFrequenciesIndex,
                                                    int cumulativeScaleIndex, double* outGlobalSum) {
    if (mi355::isShardedHandle(instance)) return BEAGLE_ERROR_NO_IMPLEMENTATION;
    GET_INSTANCE_KEEP_PENDING(instance);
    if (!outGlobalSum) return BEAGLE_ERROR_OUT_OF_RANGE;
    if (!in->comm) return BEAGLE_ERROR_UNINITIALIZED_INSTANCE;
    if (heldWrites(in, bufferIndex)) { int rcp = executeHeldPre(in); if (rcp) return rcp; }
    int rc = rootEnqueue(in, bufferIndex, categoryWeightsIndex, stateFrequenciesIndex, cumulativeScaleIndex, -1, in->dResult);
    if (rc) return rc;
    // this shard's sum -> the sum over all ranks (RCCL over xGMI; a communicator of one rank still takes the call) -> the host's
    // mapped result words, all on the instance's stream
    if (ncclAllReduce(in->dResult, in->dResult, 1, ncclDouble, ncclSum, in->comm, live(in)) != ncclSuccess) return BEAGLE_ERROR_GENERAL;
    const unsigned long long seq = ++in->resultSeq;
    mi355::launchRootFinal(live(in), in->dResult, 1, in->hResultDev, (unsigned long long*)(in->hResultDev + 8), seq);
    HIP_TRY(hipGetLastError());
    rc = sitePrefetchAfterRoot(in); if (rc) return rc;          // (behind the publishing kernel: neither the collective nor the result waits for the copy)
    { const int rcw = waitResult(in, seq); if (rcw) return rcw; }
    ringIdle(in);
    return finishSum(in->hResult[0], outGlobalSum);
}

}  // extern "C"
