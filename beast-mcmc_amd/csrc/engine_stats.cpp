// engine_stats.cpp — the MI355X extensions that steer or observe an instance without computing anything: stream, synchronisation,
// the kernel timer, dimensions, counters.
#include "engine_internal.h"

using mi355::shardedStates;
using mi355::shardedCategories;
using namespace mi355::eng;

// the walk's counters since the last timer reset (beagleMi355WalkStats, beagleMi355WalkLaunchInfo)
static void resetWalkCounters(Instance* in) {
    in->statMicroOps = in->statStored = in->statMemReads = in->statTipReads = in->statScaleReads = in->statWalks = in->statScaleWrites = 0;
    in->statFastWalks = in->statFused = 0;
    in->statTableRows = in->statTableReads = in->statRepeatClades = in->statTwoTables = in->statUnstoredConsumers = 0;
    in->statSubRuns = in->statSubRunOps = 0;
    in->statTabFirst = in->statTabFirstBehindMem = in->statTabFirstBehindCherry = in->statTabMaxClasses = 0;
}

extern "C" {

// ---- MI355X extensions -----------------------------------------------------------------------
int beagleMi355SetStream(int instance, void* hipStream) {
    if (mi355::isShardedHandle(instance)) { return BEAGLE_ERROR_NO_IMPLEMENTATION; }
    GET_INSTANCE(instance);
    HIP_TRY(hipStreamSynchronize(live(in)));
    ringIdle(in);
    in->stream = hipStream ? (hipStream_t)hipStream : in->ownStream;
    return BEAGLE_SUCCESS;
}

int beagleMi355Synchronize(int instance) {
    if (mi355::isShardedHandle(instance)) { return mi355::shardedBroadcast(instance, [&](int h) { return beagleMi355Synchronize(h); }); }
    GET_INSTANCE_KEEP_PENDING(instance);                      // (a held-back pre-order list is not work in flight)
    HIP_TRY(hipStreamSynchronize(live(in)));
    ringIdle(in);
    return BEAGLE_SUCCESS;
}

int beagleMi355KernelTimer(int instance, int enable, double* outMillis, long* outLaunches) {
    if (mi355::isShardedHandle(instance)) {             // the slowest shard's kernel time, the launches of all
        std::mutex mu; double ms = 0.0; long launches = 0;
        const int rc = mi355::shardedBroadcast(instance, [&](int h) { double m = 0.0; long l = 0; const int r = beagleMi355KernelTimer(h, enable, &m, &l);
                                                                       std::lock_guard<std::mutex> g(mu); ms = std::max(ms, m); launches += l; return r; });
        if (outMillis) *outMillis = ms;
        if (outLaunches) *outLaunches = launches;
        return rc;
    }
    GET_INSTANCE(instance);
    HIP_TRY(hipStreamSynchronize(live(in)));
    ringIdle(in);
    for (size_t k = 0; k < in->eventsUsed; k++) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, in->events[k].first, in->events[k].second) == hipSuccess) in->timedMs += ms;
    }
    in->timedLaunches += in->pendingLaunches;
    in->pendingLaunches = 0;
    in->eventsUsed = 0;
    if (outMillis) *outMillis = in->timedMs;
    if (outLaunches) *outLaunches = in->timedLaunches;
    in->timedMs = 0.0; in->timedLaunches = 0;
    resetWalkCounters(in);
    in->timing = enable != 0;
    in->timingEvery = enable > 1 ? enable : 1; in->timingTick = 0;
    // event pairs for the calls to come are created here, not inside the region being timed
    while (enable && in->events.size() < 1024) {
        hipEvent_t a, b;
        HIP_TRY(hipEventCreate(&a)); HIP_TRY(hipEventCreate(&b));
        in->events.emplace_back(a, b);
    }
    return BEAGLE_SUCCESS;
}

int beagleMi355GetDimensions(int instance, int* out8) {
    if (!out8) return BEAGLE_ERROR_OUT_OF_RANGE;
    if (mi355::isShardedHandle(instance)) {
        memset(out8, 0, 8 * sizeof(int));
        out8[2] = shardedStates(instance); out8[3] = mi355::shardedPatternCount(instance); out8[4] = shardedCategories(instance);
        return out8[3] > 0 ? BEAGLE_SUCCESS : BEAGLE_ERROR_UNINITIALIZED_INSTANCE;
    }
    Instance* in = lookup(instance);
    if (!in) return BEAGLE_ERROR_UNINITIALIZED_INSTANCE;
    out8[0] = in->tipCount; out8[1] = in->partialsCount; out8[2] = in->S; out8[3] = in->P; out8[4] = in->C;
    out8[5] = in->matrixCount; out8[6] = in->scaleCount; out8[7] = in->partitionCount;
    return BEAGLE_SUCCESS;
}

int beagleMi355KernelTimerRestart(int instance) {
    if (mi355::isShardedHandle(instance)) { return mi355::shardedBroadcast(instance, [&](int h) { return beagleMi355KernelTimerRestart(h); }); }
    Instance* in = lookup(instance);
    if (!in) return BEAGLE_ERROR_UNINITIALIZED_INSTANCE;
    in->eventsUsed = 0; in->timedMs = 0.0; in->timedLaunches = 0; in->pendingLaunches = 0; in->timingTick = 0; in->timedCalls = 0;
    resetWalkCounters(in);
    return BEAGLE_SUCCESS;
}

int beagleMi355KernelTimerCalls(int instance, long* outCalls) {
    if (mi355::isShardedHandle(instance)) {             // shard 0's (every shard brackets the same calls)
        return mi355::shardedFirst(instance, [&](int h) { return beagleMi355KernelTimerCalls(h, outCalls); });
    }
    Instance* in = lookup(instance);
    if (!in || !outCalls) return BEAGLE_ERROR_UNINITIALIZED_INSTANCE;
    *outCalls = in->timedCalls;
    in->timedCalls = 0;
    return BEAGLE_SUCCESS;
}

int beagleMi355RootFusedCount(int instance, long* outCount) {
    if (mi355::isShardedHandle(instance)) {
        return mi355::shardedFirst(instance, [&](int h) { return beagleMi355RootFusedCount(h, outCount); });
    }
    Instance* in = lookup(instance);
    if (!in || !outCount) return BEAGLE_ERROR_UNINITIALIZED_INSTANCE;
    *outCount = in->statRootFused;
    return BEAGLE_SUCCESS;
}

int beagleMi355SitePrefetchCount(int instance, long* outCount) {
    if (mi355::isShardedHandle(instance)) {
        return mi355::shardedFirst(instance, [&](int h) { return beagleMi355SitePrefetchCount(h, outCount); });
    }
    Instance* in = lookup(instance);
    if (!in || !outCount) return BEAGLE_ERROR_UNINITIALIZED_INSTANCE;
    *outCount = in->statSitePrefetched;
    return BEAGLE_SUCCESS;
}

int beagleMi355WalkStats(int instance, long* out8) {
    if (mi355::isShardedHandle(instance)) {             // counters of shard 0 (every shard runs the same programs)
        return mi355::shardedFirst(instance, [&](int h) { return beagleMi355WalkStats(h, out8); });
    }
    Instance* in = lookup(instance);
    if (!in || !out8) return BEAGLE_ERROR_UNINITIALIZED_INSTANCE;
    out8[0] = in->statMicroOps; out8[1] = in->statStored; out8[2] = in->statMemReads; out8[3] = in->statTipReads;
    out8[4] = in->statScaleReads; out8[5] = in->statWalks; out8[6] = in->statScaleWrites; out8[7] = in->statFastWalks;
    return BEAGLE_SUCCESS;
}

int beagleMi355WalkHealth(int instance, long* out4) {
    if (mi355::isShardedHandle(instance)) {             // shard 0's
        return mi355::shardedFirst(instance, [&](int h) { return beagleMi355WalkHealth(h, out4); });
    }
    GET_INSTANCE_KEEP_PENDING(instance);
    if (!out4) return BEAGLE_ERROR_OUT_OF_RANGE;
    unsigned served = 0;
    if (in->walkSelfServed) { int rc = download(in, &served, in->walkSelfServed, sizeof(served)); if (rc) return rc; }
    out4[0] = (long)served; out4[1] = (long)(in->walkSpinLimit / 100ull); out4[2] = in->statFoldedVectors; out4[3] = in->statFoldBuilds;
    return BEAGLE_SUCCESS;
}

int beagleMi355RepeatStats(int instance, long* out10) {
    long* out6 = out10;
    if (mi355::isShardedHandle(instance)) {             // shard 0's
        return mi355::shardedFirst(instance, [&](int h) { return beagleMi355RepeatStats(h, out10); });
    }
    Instance* in = lookup(instance);
    if (!in || !out6) return BEAGLE_ERROR_UNINITIALIZED_INSTANCE;
    out10[6] = in->statTwoTables; out10[7] = in->statUnstoredConsumers;
    out10[8] = (long)in->repeatIndex.bytes(); out10[9] = in->statRepeatResets;
    size_t bytes = in->repeatArena ? (size_t)in->repeatArenas * in->C * in->P * 32 : 0;
    for (const auto& b : in->repeatPool) bytes += b.size;
    out6[0] = in->statTableRows; out6[1] = in->statTableReads; out6[2] = in->statRepeatClades;
    out6[3] = (long)bytes; out6[4] = in->repeatIndex.builds; out6[5] = in->statRepeatBuildUs;
    return BEAGLE_SUCCESS;
}

int beagleMi355RepeatSubRunStats(int instance, long* out2) {
    if (mi355::isShardedHandle(instance)) {             // shard 0's
        return mi355::shardedFirst(instance, [&](int h) { return beagleMi355RepeatSubRunStats(h, out2); });
    }
    Instance* in = lookup(instance);
    if (!in || !out2) return BEAGLE_ERROR_UNINITIALIZED_INSTANCE;
    out2[0] = in->statSubRuns; out2[1] = in->statSubRunOps;
    return BEAGLE_SUCCESS;
}

int beagleMi355TableOperandStats(int instance, long* out4) {
    if (mi355::isShardedHandle(instance)) {             // shard 0's
        return mi355::shardedFirst(instance, [&](int h) { return beagleMi355TableOperandStats(h, out4); });
    }
    Instance* in = lookup(instance);
    if (!in || !out4) return BEAGLE_ERROR_UNINITIALIZED_INSTANCE;
    out4[0] = in->statTabFirst; out4[1] = in->statTabFirstBehindMem; out4[2] = in->statTabFirstBehindCherry; out4[3] = in->statTabMaxClasses;
    return BEAGLE_SUCCESS;
}

int beagleMi355WalkLaunchInfo(int instance, long* out8) {
    if (mi355::isShardedHandle(instance)) {             // shard 0's
        return mi355::shardedFirst(instance, [&](int h) { return beagleMi355WalkLaunchInfo(h, out8); });
    }
    Instance* in = lookup(instance);
    if (!in || !out8) return BEAGLE_ERROR_UNINITIALIZED_INSTANCE;
    out8[0] = in->statTicketWalks; out8[1] = in->statFlagWalks; out8[2] = in->lastLaunchRows; out8[3] = in->lastLaunchSlices;
    out8[4] = in->statFused; out8[5] = in->statMicroOps; out8[6] = in->statSliceAccum; out8[7] = in->statRootPartsFused;
    return BEAGLE_SUCCESS;
}

int beagleMi355GradientStats(int instance, long* out4) {
    if (mi355::isShardedHandle(instance)) {             // counters of shard 0 (every shard is driven the same way)
        return mi355::shardedFirst(instance, [&](int h) { return beagleMi355GradientStats(h, out4); });
    }
    Instance* in = lookup(instance);
    if (!in || !out4) return BEAGLE_ERROR_UNINITIALIZED_INSTANCE;
    out4[0] = in->statFusedGradients; out4[1] = in->statPreLists; out4[2] = in->statWalkedGradients; out4[3] = in->statLateLists;
    return BEAGLE_SUCCESS;
}

long beagleMi355DeviceBytes(int instance) {
    if (mi355::isShardedHandle(instance)) {
        std::mutex mu; long total = 0;
        mi355::shardedBroadcast(instance, [&](int h) { const long b = beagleMi355DeviceBytes(h); std::lock_guard<std::mutex> l(mu); total += b; return 0; });
        return total;
    }
    Instance* in = lookup(instance);
    return in ? (long)in->deviceBytes : -1;
}

}  // extern "C"
