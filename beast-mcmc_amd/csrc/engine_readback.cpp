// engine_readback.cpp — partials and scale factors back to the host.
#include "engine_internal.h"

using mi355::shardedStates;
using mi355::shardedCategories;
using namespace mi355::eng;

// Read-back of `count` partials buffers (AncestralStateBeagleTreeLikelihood.java:414-542 reads every
// internal node once per logged sample): virtual buffers are materialised by ONE walk, every buffer is converted to the
// API layout [C][P][S] on the device with its scale factors folded in, and the device-to-host copies stream through a
// pinned bounce buffer, a chunk of buffers at a time, with one synchronisation per chunk.
// host-side copy of a chunk out of the pinned bounce buffer, on a few threads when it is large: the destination is the
// caller's array, usually touched for the first time here, and faulting its pages in is what bounds a single thread
// (profiles/r02_readback.json: the 1.28 GB sweep ran at 8 GB/s, below the node-by-node loop)
struct HostCopy {
    std::vector<std::thread> th;
    void start(char* dst, const char* src, size_t bytes) {
        const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
        const size_t k = bytes < ((size_t)8 << 20) ? 1 : std::min<size_t>(8, std::max<size_t>(1, hw / 2));
        if (k == 1) { memcpy(dst, src, bytes); return; }
        const size_t per = ((bytes / k) + 4095) & ~(size_t)4095;
        for (size_t i = 0; i * per < bytes; i++)
            th.emplace_back([=] { memcpy(dst + i * per, src + i * per, std::min(per, bytes - i * per)); });
    }
    void join() { for (auto& t : th) t.join(); th.clear(); }
    ~HostCopy() { join(); }
};

// out == nullptr (count must fit one chunk): the data is left in the pinned buffer exportHost[0] (beagleMi355GetPartialsPinned)
static int exportPartials(Instance* in, const int* bufferIndices, const int* scaleIndices, int count, double* out) {
    ReadSet reads(in);
    for (int k = 0; k < count; k++) {
        const int b = bufferIndices[k];
        if (badIndex(b, in->partialsCount)) return BEAGLE_ERROR_OUT_OF_RANGE;
        if (scaleIndices && scaleIndices[k] != BEAGLE_OP_NONE && badIndex(scaleIndices[k], in->scaleCount)) return BEAGLE_ERROR_OUT_OF_RANGE;
        if (foldedTip(in, b)) { const int rcd = demoteFoldedTip(in, b); if (rcd) return rcd; }      // (a tip with an emission table gets its partials: engine_tipemission.cpp)
        if (int bad = reads.pre(b)) return bad;              // (compact states are no partials to read back)
    }
    { int rc = reads.materialize(); if (rc) return rc; }
    const size_t elems = (size_t)in->C * in->P * in->S, bytes = elems * sizeof(double);
    // chunks of about 32 MiB, two in flight: while the device converts and copies chunk k + 1, the host empties chunk k
    const size_t chunk = std::max<size_t>(1, std::min<size_t>((size_t)count, ((size_t)32 << 20) / bytes));
    if (!out && (size_t)count > chunk) return BEAGLE_ERROR_OUT_OF_RANGE;
    if (in->exportBytes < chunk * bytes) {
        HIP_TRY(hipStreamSynchronize(live(in)));
        for (int k = 0; k < 2; k++) {
            releaseDevice(in, in->exportDev[k]);
            if (in->exportHost[k]) hipHostFree(in->exportHost[k]);
            in->exportHost[k] = nullptr;
        }
        in->exportBytes = 0;                               // (a failure below leaves it so: the next call starts over)
        for (int k = 0; k < 2; k++) {
            int rc = growDevice(in, in->exportDev[k], chunk * bytes, chunk * bytes, Grow::SyncIfHeld); if (rc) return rc;
            HIP_TRY(hipHostMalloc((void**)&in->exportHost[k], chunk * bytes, hipHostMallocDefault));
            if (!in->exportEvent[k]) HIP_TRY(hipEventCreateWithFlags(&in->exportEvent[k], hipEventDisableTiming));
        }
        in->exportBytes = chunk * bytes;
    }
    HostCopy copies[2];
    const size_t nChunks = ((size_t)count + chunk - 1) / chunk;
    auto chunkCount = [&](size_t c) { return std::min(chunk, (size_t)count - c * chunk); };
    for (size_t c = 0; c < nChunks; c++) {
        const int w = (int)(c & 1);
        copies[w].join();                                  // the host copy that was reading exportHost[w] (chunk c - 2)
        const size_t n = chunkCount(c);
        for (size_t k = 0; k < n; k++) {
            const int b = bufferIndices[c * chunk + k];
            if (!preOperand(in, b)) return BEAGLE_ERROR_OUT_OF_RANGE;
            const double* sc = nullptr; int raw = 0;
            if (scaleIndices && scaleIndices[c * chunk + k] != BEAGLE_OP_NONE) {
                int rc = ensureScale(in, scaleIndices[c * chunk + k]); if (rc) return rc;
                sc = in->scale[scaleIndices[c * chunk + k]]; raw = in->scaleIsRaw[scaleIndices[c * chunk + k]];
            }
            mi355::launchExportPartials(live(in), in->partials[b], sc, raw, in->exportDev[w].as<double>() + k * elems, in->P, in->S, in->C, in->tiled);
        }
        HIP_TRY(hipMemcpyAsync(in->exportHost[w], in->exportDev[w].p, n * bytes, hipMemcpyDeviceToHost, live(in)));
        HIP_TRY(hipEventRecord(in->exportEvent[w], live(in)));
        if (c >= 1 && out) {                               // chunk c - 1 has landed (or lands while this one is being produced)
            HIP_TRY(hipEventSynchronize(in->exportEvent[1 - w]));
            copies[1 - w].start((char*)(out + (c - 1) * chunk * elems), (const char*)in->exportHost[1 - w], chunkCount(c - 1) * bytes);
        }
    }
    const int last = (int)((nChunks - 1) & 1);
    HIP_TRY(hipEventSynchronize(in->exportEvent[last]));
    ringIdle(in);
    if (out) copies[last].start((char*)(out + (nChunks - 1) * chunk * elems), (const char*)in->exportHost[last], chunkCount(nChunks - 1) * bytes);
    copies[0].join(); copies[1].join();
    return BEAGLE_SUCCESS;
}

extern "C" {

int beagleGetPartials(int instance, int bufferIndex, int scaleIndex, double* outPartials) {
    if (mi355::isShardedHandle(instance)) {
        return mi355::shardedGetPerPatternDoubles(instance, outPartials, shardedStates(instance), shardedCategories(instance),
                                                  [&](int h, double* v) { return beagleGetPartials(h, bufferIndex, scaleIndex, v); });
    }
    GET_INSTANCE(instance);
    if (in->basta) return bastaGetPartials(in, bufferIndex, outPartials);
    return exportPartials(in, &bufferIndex, &scaleIndex, 1, outPartials);
}

// MI355X extension: `count` buffers in one call, out = [count][C][P][S]; scaleIndices may be NULL
int beagleMi355GetPartialsBatch(int instance, const int* bufferIndices, const int* scaleIndices, int count, double* outPartials) {
    if (mi355::isShardedHandle(instance)) {
        const size_t elems = (size_t)shardedCategories(instance) * mi355::shardedPatternCount(instance) * shardedStates(instance);
        for (int k = 0; k < count; k++) {
            const int rc = beagleGetPartials(instance, bufferIndices[k], scaleIndices ? scaleIndices[k] : BEAGLE_OP_NONE, outPartials + (size_t)k * elems);
            if (rc) return rc;
        }
        return BEAGLE_SUCCESS;
    }
    GET_INSTANCE(instance);
    if (count <= 0) return BEAGLE_SUCCESS;
    return exportPartials(in, bufferIndices, scaleIndices, count, outPartials);
}

// MI355X extensions for the JNI shim: the result stays in the engine's pinned bounce buffer (valid until the next call on the
// instance) and goes from there into the Java array with ONE copy.  Not for the sharded instance (NO_IMPLEMENTATION: the
// shim then takes the ordinary entry point).
int beagleMi355GetPartialsPinned(int instance, int bufferIndex, int scaleIndex, const double** outPinned, long* outCount) {
    if (mi355::isShardedHandle(instance)) return BEAGLE_ERROR_NO_IMPLEMENTATION;
    GET_INSTANCE(instance);
    if (!outPinned || !outCount) return BEAGLE_ERROR_OUT_OF_RANGE;
    const int rc = exportPartials(in, &bufferIndex, &scaleIndex, 1, nullptr);
    if (rc) return rc;
    *outPinned = in->exportHost[0]; *outCount = (long)in->C * in->P * in->S;
    return BEAGLE_SUCCESS;
}

int beagleGetLogScaleFactors(int instance, int scaleIndex, double* out) {
    if (mi355::isShardedHandle(instance)) {
        return mi355::shardedGetPerPatternDoubles(instance, out, 1, 1, [&](int h, double* v) { return beagleGetLogScaleFactors(h, scaleIndex, v); });
    }
    GET_INSTANCE(instance);
    if (badIndex(scaleIndex, in->scaleCount)) return BEAGLE_ERROR_OUT_OF_RANGE;
    int rc = ensureScale(in, scaleIndex); if (rc) return rc;
    rc = download(in, out, in->scale[scaleIndex], (size_t)in->P * sizeof(double)); if (rc) return rc;
    if (in->scaleIsRaw[scaleIndex]) for (int p = 0; p < in->P; p++) out[p] = log(out[p]);
    return BEAGLE_SUCCESS;
}

}  // extern "C"
