// engine_differential.cpp — substitution-parameter differential matrices in one call (include/beagle_mi355.h
// beagleMi355UpdateDifferentialMatrices; kernels_differential.hip): argument checks, the (eigen system, differential) pairs of the
// call, one packed upload, one rotation launch and one launch over every (branch, category).
#include "engine_internal.h"

using namespace mi355::eng;

// What BranchSubstitutionParameterDelegate.cacheDifferentialMassMatrix does with a getExactDifferentialMassMatrix and a
// setDifferentialMatrix per branch (BranchSubstitutionParameterDelegate.java:62-81), into the slots where calculateEdgeDifferentials reads
// them.  A slot is written as beagleSetTransitionMatrix writes it: behind everything queued (live()), and behind a held-back pre-order
// list only when that list reads the slot.
static int differentialMatrices(Instance* in, const int* eigenIdx, const int* rateIdx, const double* inDifferentials, int differentialCount,
                                const int* diffIdx, const int* slots, const double* lens, int count, int mode) {
    if (in->S > 64 || in->basta) return BEAGLE_ERROR_NO_IMPLEMENTATION;
    if (count <= 0) return BEAGLE_SUCCESS;
    if (mode != BEAGLE_MI355_DIFFERENTIAL_EXACT && mode != BEAGLE_MI355_DIFFERENTIAL_FIRST_ORDER) return BEAGLE_ERROR_OUT_OF_RANGE;
    if (!inDifferentials || !slots || !lens || differentialCount < 1) return BEAGLE_ERROR_OUT_OF_RANGE;
    std::vector<char> named((size_t)in->matrixCount, 0);                // (two branches into one slot would race)
    for (int k = 0; k < count; k++) {
        if (badIndex(slots[k], in->matrixCount) || named[(size_t)slots[k]]) return BEAGLE_ERROR_OUT_OF_RANGE;
        named[(size_t)slots[k]] = 1;
        if ((eigenIdx && badIndex(eigenIdx[k], in->eigenCount)) || (rateIdx && badIndex(rateIdx[k], in->eigenCount)) ||
            (diffIdx && badIndex(diffIdx[k], differentialCount))) return BEAGLE_ERROR_OUT_OF_RANGE;
    }
    if (in->eigenCount < 1) return BEAGLE_ERROR_OUT_OF_RANGE;           // (NULL index lists name 0)
    const bool exact = mode == BEAGLE_MI355_DIFFERENTIAL_EXACT;
    // the distinct (eigen system, differential) pairs, in order of first appearance: V = U^-1 dQ U is formed once for each
    std::vector<int> pairs, pairOf((size_t)count);
    if (exact) {
        std::unordered_map<long long, int> seen;
        for (int k = 0; k < count; k++) {
            const int e = eigenIdx ? eigenIdx[k] : 0, d = diffIdx ? diffIdx[k] : 0;
            const auto at = seen.emplace((long long)e * differentialCount + d, (int)(pairs.size() / 2));
            if (at.second) { pairs.push_back(e); pairs.push_back(d); }
            pairOf[(size_t)k] = at.first->second;
        }
    } else for (int k = 0; k < count; k++) pairOf[(size_t)k] = diffIdx ? diffIdx[k] : 0;
    const size_t per = (size_t)in->S * in->S, nPairs = pairs.size() / 2;
    // one packed upload: [dQ double[differentialCount][S][S] | lengths double[count] | slot | eigen | rate set | pair (first order: the
    // differential) int[count] each | {eigen, differential} int[pairs][2]]
    const size_t qBytes = (size_t)differentialCount * per * sizeof(double), lenBytes = (size_t)count * sizeof(double),
                 idxBytes = (size_t)count * sizeof(int), bytes = qBytes + lenBytes + 4 * idxBytes + pairs.size() * sizeof(int);
    if (bytes > RING_BYTES / 2) return BEAGLE_ERROR_OUT_OF_RANGE;
    for (int k = 0; k < count; k++)
        if (heldReadsMatrix(in, slots[k])) { const int rcp = executeHeldPre(in); if (rcp) return rcp; break; }
    std::vector<char> pack(bytes);
    memcpy(pack.data(), inDifferentials, qBytes);
    memcpy(pack.data() + qBytes, lens, lenBytes);
    int* pIdx = (int*)(pack.data() + qBytes + lenBytes);
    memcpy(pIdx, slots, idxBytes);
    if (eigenIdx) memcpy(pIdx + count, eigenIdx, idxBytes); else std::fill(pIdx + count, pIdx + 2 * (size_t)count, 0);
    if (rateIdx) memcpy(pIdx + 2 * (size_t)count, rateIdx, idxBytes); else std::fill(pIdx + 2 * (size_t)count, pIdx + 3 * (size_t)count, 0);
    memcpy(pIdx + 3 * (size_t)count, pairOf.data(), idxBytes);
    if (!pairs.empty()) memcpy(pIdx + 4 * (size_t)count, pairs.data(), pairs.size() * sizeof(int));
    if (exact) {
        const size_t need = nPairs * per * sizeof(double);
        const int rcg = growDevice(in, in->differentialDev, need, (need + 4095) & ~(size_t)4095, Grow::SyncIfHeld); if (rcg) return rcg;
    }
    void* dPack = nullptr;
    const int rc = uploadTransient(in, pack.data(), bytes, &dPack); if (rc) return rc;
    const double* dQ = (const double*)dPack;
    const double* dLen = (const double*)((const char*)dPack + qBytes);
    const int* dIdx = (const int*)((const char*)dPack + qBytes + lenBytes);
    const int *dEig = dIdx + count, *dRate = dIdx + 2 * (size_t)count, *dPair = dIdx + 3 * (size_t)count, *dPairs = dIdx + 4 * (size_t)count;
    if (exact) {
        double* V = in->differentialDev.as<double>();
        mi355::launchDifferentialRotate(live(in), V, in->eigen, dQ, dPairs, (int)nPairs, in->S, in->eigenComplex);
        mi355::launchDifferentialExact(live(in), in->matrices, in->eigen, in->rates, V, dIdx, dLen, dEig, dRate, dPair, count, in->S, in->C,
                                       in->eigenComplex);
    } else {
        mi355::launchDifferentialFirstOrder(live(in), in->matrices, in->rates, dQ, dIdx, dLen, dRate, dPair, count, in->S, in->C);
    }
    HIP_TRY(hipGetLastError());
    return BEAGLE_SUCCESS;
}

extern "C" {

int beagleMi355UpdateDifferentialMatrices(int instance, const int* eigenIndices, const int* categoryRatesIndices,
                                          const double* inDifferentials, int differentialCount, const int* differentialIndices,
                                          const int* matrixIndices, const double* edgeLengths, int count, int mode) {
    if (mi355::isShardedHandle(instance)) {                 // matrices are replicated: every shard forms its own (the same bits)
        return mi355::shardedBroadcast(instance, [&](int h) {
            return beagleMi355UpdateDifferentialMatrices(h, eigenIndices, categoryRatesIndices, inDifferentials, differentialCount,
                                                         differentialIndices, matrixIndices, edgeLengths, count, mode); });
    }
    GET_INSTANCE_KEEP_PENDING(instance);                      // (a held-back pre-order list waits unless one of ITS matrices is rewritten)
    return differentialMatrices(in, eigenIndices, categoryRatesIndices, inDifferentials, differentialCount, differentialIndices,
                                matrixIndices, edgeLengths, count, mode);
}

}  // extern "C"
