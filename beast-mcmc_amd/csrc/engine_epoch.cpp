// engine_epoch.cpp — branch matrices of epoch models in one call (include/beagle_mi355.h beagleMi355UpdateTransitionMatricesWithEpochs,
// beagleMi355EpochStats; kernels_epoch.hip): argument checks, the split of a list into launches, one packed upload and one launch per part.
#include "engine_internal.h"

using namespace mi355::eng;

constexpr size_t EPOCH_LAUNCH_BYTES = RING_BYTES / 4;               // bytes of packed input one launch may take from the staging ring

// entries of one launch at most (BEAGLE_MI355_EPOCH_CHUNK=<entries>, read at the call: fewer — tests of the split)
static size_t epochChunk() {
    if (const char* e = getenv("BEAGLE_MI355_EPOCH_CHUNK")) { const long v = atol(e); if (v > 0) return (size_t)v; }
    return SIZE_MAX;
}

// what needs no instance: the shape of the list and the lengths
static int checkEpochList(int S, const int* off, const int* segEig, const double* segLen, const int* slots, int count, int flags) {
    if (S > 64) return BEAGLE_ERROR_NO_IMPLEMENTATION;
    if (count < 0 || flags != 0) return BEAGLE_ERROR_OUT_OF_RANGE;
    if (count == 0) return BEAGLE_SUCCESS;                              // (nothing is read)
    if (!off || !segEig || !segLen || !slots) return BEAGLE_ERROR_OUT_OF_RANGE;
    if (off[0] != 0) return BEAGLE_ERROR_OUT_OF_RANGE;
    for (int k = 0; k < count; k++) if (off[k + 1] <= off[k]) return BEAGLE_ERROR_OUT_OF_RANGE;      // (an entry without a segment)
    for (int j = 0; j < off[count]; j++) if (!(std::isfinite(segLen[j]) && segLen[j] >= 0.0)) return BEAGLE_ERROR_OUT_OF_RANGE;
    return BEAGLE_SUCCESS;
}

// What SubstitutionModelDelegate.updateTransitionMatrices does for branches that cross epoch boundaries (an updateTransitionMatrices per
// eigen system into pool buffers, rounds of convolveTransitionMatrices: treedatalikelihood/SubstitutionModelDelegate.java:213-405), with
// the segments named per branch.  A slot is written as beagleUpdateTransitionMatrices writes it: behind everything queued (live()), and
// behind a held-back pre-order list only when that list reads the slot.
static int epochMatrices(Instance* in, const int* off, const int* segEig, const double* segLen, const int* rateIdx, const int* slots,
                         int count, int flags) {
    const int rcc = checkEpochList(in->S, off, segEig, segLen, slots, count, flags); if (rcc) return rcc;
    if (count == 0) return BEAGLE_SUCCESS;
    std::vector<char> named((size_t)in->matrixCount, 0);                // (two workgroups into one slot would race)
    int longest = 0;
    for (int k = 0; k < count; k++) {
        if (badIndex(slots[k], in->matrixCount) || named[(size_t)slots[k]]) return BEAGLE_ERROR_OUT_OF_RANGE;
        named[(size_t)slots[k]] = 1;
        if (rateIdx && badIndex(rateIdx[k], in->eigenCount)) return BEAGLE_ERROR_OUT_OF_RANGE;
        longest = std::max(longest, off[k + 1] - off[k]);
    }
    for (int j = 0; j < off[count]; j++) if (badIndex(segEig[j], in->eigenCount)) return BEAGLE_ERROR_OUT_OF_RANGE;
    if (in->eigenCount < 1) return BEAGLE_ERROR_OUT_OF_RANGE;           // (a NULL rate list names rate set 0)
    for (int k = 0; k < count; k++)
        if (heldReadsMatrix(in, slots[k])) { const int rcp = executeHeldPre(in); if (rcp) return rcp; break; }
    const size_t chunk = epochChunk();
    std::vector<char> pack;
    for (int first = 0; first < count;) {
        // the entries of this launch: as many as the chunk and the ring's budget allow, one at least
        const size_t perEntry = 3 * sizeof(int), perSeg = sizeof(double) + sizeof(int);
        int last = first + 1;
        size_t bytes = sizeof(int) + perEntry + (size_t)(off[last] - off[first]) * perSeg;
        while (last < count && (size_t)(last - first) < chunk) {
            const size_t more = perEntry + (size_t)(off[last + 1] - off[last]) * perSeg;
            if (bytes + more > EPOCH_LAUNCH_BYTES) break;
            bytes += more; last++;
        }
        const size_t m = (size_t)(last - first), s0 = (size_t)off[first], nSeg = (size_t)off[last] - s0;
        // one packed upload per launch: [segment lengths double[nSeg] | offsets int[m + 1] (from 0) | segment eigen int[nSeg] | slot int[m] |
        // rate set int[m]]
        pack.resize(nSeg * sizeof(double) + (m + 1 + nSeg + 2 * m) * sizeof(int));
        double* pLen = (double*)pack.data();
        int* pOff = (int*)(pack.data() + nSeg * sizeof(double));
        int* pEig = pOff + m + 1;
        int* pSlot = pEig + nSeg;
        int* pRate = pSlot + m;
        memcpy(pLen, segLen + s0, nSeg * sizeof(double));
        memcpy(pEig, segEig + s0, nSeg * sizeof(int));
        for (size_t k = 0; k <= m; k++) pOff[k] = off[(size_t)first + k] - (int)s0;
        for (size_t k = 0; k < m; k++) { pSlot[k] = slots[(size_t)first + k]; pRate[k] = rateIdx ? rateIdx[(size_t)first + k] : 0; }
        void* dPack = nullptr;
        const int rc = uploadTransient(in, pack.data(), pack.size(), &dPack); if (rc) return rc;
        const double* dLen = (const double*)dPack;
        const int* dOff = (const int*)((const char*)dPack + nSeg * sizeof(double));
        const int* dEig = dOff + m + 1;
        const int* dSlot = dEig + nSeg;
        const int* dRate = dSlot + m;
        if (!mi355::launchEpochMatrices(live(in), in->matrices, in->eigen, in->rates, dSlot, dRate, dOff, dEig, dLen, (int)m, in->S, in->C,
                                        in->eigenComplex)) return BEAGLE_ERROR_GENERAL;
        HIP_TRY(hipGetLastError());
        first = last;
    }
    in->statEpochCalls++; in->statEpochMatrices += (long)count * in->C; in->statEpochSegments += off[count]; in->statEpochLongest = longest;
    return BEAGLE_SUCCESS;
}

extern "C" {

int beagleMi355UpdateTransitionMatricesWithEpochs(int instance, const int* segmentOffsets, const int* segmentEigenIndices,
                                                  const double* segmentLengths, const int* categoryRateIndices,
                                                  const int* probabilityIndices, int count, int flags) {
    if (mi355::isShardedHandle(instance)) {
        // (queued: every shard's thread applies its copy; what needs no shard is checked here, a bad index surfaces at the next waiting call)
        const int rcc = checkEpochList(mi355::shardedStates(instance), segmentOffsets, segmentEigenIndices, segmentLengths,
                                       probabilityIndices, count, flags); if (rcc) return rcc;
        if (count == 0) return BEAGLE_SUCCESS;
        const int nSeg = segmentOffsets[count];
        std::vector<int> o(segmentOffsets, segmentOffsets + count + 1), e(segmentEigenIndices, segmentEigenIndices + nSeg),
                         p(probabilityIndices, probabilityIndices + count), r;
        std::vector<double> t(segmentLengths, segmentLengths + nSeg);
        if (categoryRateIndices) r.assign(categoryRateIndices, categoryRateIndices + count);
        const bool hasR = categoryRateIndices != nullptr;
        return mi355::shardedPost(instance, [=](int h) {
            return beagleMi355UpdateTransitionMatricesWithEpochs(h, o.data(), e.data(), t.data(), hasR ? r.data() : nullptr, p.data(), count, 0); });
    }
    GET_INSTANCE_KEEP_PENDING(instance);                      // (a held-back pre-order list waits unless one of ITS matrices is rewritten)
    return epochMatrices(in, segmentOffsets, segmentEigenIndices, segmentLengths, categoryRateIndices, probabilityIndices, count, flags);
}

int beagleMi355EpochStats(int instance, long* out4) {
    if (mi355::isShardedHandle(instance)) { return mi355::shardedFirst(instance, [&](int h) { return beagleMi355EpochStats(h, out4); }); }
    GET_INSTANCE_KEEP_PENDING(instance);
    if (!out4) return BEAGLE_ERROR_OUT_OF_RANGE;
    out4[0] = in->statEpochCalls; out4[1] = in->statEpochMatrices; out4[2] = in->statEpochSegments; out4[3] = in->statEpochLongest;
    return BEAGLE_SUCCESS;
}

}  // extern "C"
