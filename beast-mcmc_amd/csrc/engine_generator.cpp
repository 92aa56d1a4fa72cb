// engine_generator.cpp — transition matrices straight from generators, no eigen system (include/beagle_mi355.h
// beagleMi355UpdateTransitionMatricesFromGenerators, beagleMi355GeneratorStats; kernels_generator.hip): argument checks, the split of a
// list into launches, one packed upload and two launches (power tables, matrices) per part.
#include "engine_internal.h"
#include <cfloat>

using namespace mi355::eng;

constexpr size_t GENERATOR_TABLE_BUDGET = (size_t)128 << 20;        // bytes of power tables one launch may hold

// generators / entries of one launch at most (BEAGLE_MI355_GENERATOR_CHUNK=<n>, read at the call: fewer of both — tests of the split)
static size_t generatorChunk(size_t n) {
    n = std::max<size_t>(1, n);
    if (const char* e = getenv("BEAGLE_MI355_GENERATOR_CHUNK")) { const long v = atol(e); if (v > 0) n = std::min(n, (size_t)v); }
    return n;
}

// what needs no instance: the generators and the lengths.  mu[g] = max_i -Q_ii in uniformChain's order (engine_sampling.cpp)
static int checkGenerators(int S, const double* Q, int G, const double* lens, int count, std::vector<double>& mu) {
    if (S > 64) return BEAGLE_ERROR_NO_IMPLEMENTATION;
    if (count < 0 || G < 1 || !Q) return BEAGLE_ERROR_OUT_OF_RANGE;
    if (count > 0 && !lens) return BEAGLE_ERROR_OUT_OF_RANGE;
    mu.resize((size_t)G);
    for (int g = 0; g < G; g++) {
        const double* q = Q + (size_t)g * S * S;
        for (int i = 0; i < S; i++)
            for (int j = 0; j < S; j++) {
                const double x = q[(size_t)i * S + j];
                if (!std::isfinite(x) || (i == j ? x > 0.0 : x < 0.0)) return BEAGLE_ERROR_OUT_OF_RANGE;
            }
        double m = -q[0];
        for (int i = 1; i < S; i++) {
            const double next = -q[(size_t)i * S + i];
            if (next > m) m = next;
        }
        if (!(m > 0.0) || !(m <= DBL_MAX)) return BEAGLE_ERROR_OUT_OF_RANGE;
        mu[(size_t)g] = m;
    }
    for (int k = 0; k < count; k++) if (!(std::isfinite(lens[k]) && lens[k] >= 0.0)) return BEAGLE_ERROR_OUT_OF_RANGE;
    return BEAGLE_SUCCESS;
}

// What SubstitutionModelDelegate.updateSubstitutionModels + updateTransitionMatrices do with a decomposition, a setEigenDecomposition
// and an updateTransitionMatrices (SubstitutionModelDelegate.java:272-288, 213-266), for models without a usable eigen system.  A slot
// is written as beagleUpdateTransitionMatrices writes it: behind everything queued (live()), and behind a held-back pre-order list
// only when that list reads the slot.
static int generatorMatrices(Instance* in, const double* Q, int G, const int* genIdx, const int* rateIdx, const int* slots,
                             const double* lens, int count) {
    std::vector<double> mu;
    const int rcc = checkGenerators(in->S, Q, G, lens, count, mu); if (rcc) return rcc;
    if (count == 0) return BEAGLE_SUCCESS;
    if (!slots) return BEAGLE_ERROR_OUT_OF_RANGE;
    std::vector<char> named((size_t)in->matrixCount, 0);                // (two workgroups into one slot would race)
    for (int k = 0; k < count; k++) {
        if (badIndex(slots[k], in->matrixCount) || named[(size_t)slots[k]]) return BEAGLE_ERROR_OUT_OF_RANGE;
        named[(size_t)slots[k]] = 1;
        if ((genIdx && badIndex(genIdx[k], G)) || (rateIdx && badIndex(rateIdx[k], in->eigenCount))) return BEAGLE_ERROR_OUT_OF_RANGE;
    }
    if (in->eigenCount < 1) return BEAGLE_ERROR_OUT_OF_RANGE;           // (a NULL rate list names rate set 0)
    const size_t S = (size_t)in->S, SS = S * S, tableBytes = (size_t)mi355::GENERATOR_TERMS * SS * sizeof(double);
    const size_t perGen = std::min({GENERATOR_TABLE_BUDGET / tableBytes, (RING_BYTES / 4) / ((SS + 1) * sizeof(double)), (size_t)G});
    const size_t genChunk = generatorChunk(perGen), entChunk = generatorChunk((RING_BYTES / 4) / (sizeof(double) + 3 * sizeof(int)));
    // the entries of every part of genChunk generators, in list order (a counting sort by part)
    const size_t nParts = ((size_t)G + genChunk - 1) / genChunk;
    std::vector<int> partStart(nParts + 1, 0), order((size_t)count);
    for (int k = 0; k < count; k++) partStart[(size_t)(genIdx ? genIdx[k] : 0) / genChunk + 1]++;
    for (size_t p = 0; p < nParts; p++) partStart[p + 1] += partStart[p];
    {
        std::vector<int> at(partStart.begin(), partStart.end() - 1);
        for (int k = 0; k < count; k++) order[(size_t)at[(size_t)(genIdx ? genIdx[k] : 0) / genChunk]++] = k;
    }
    for (int k = 0; k < count; k++)
        if (heldReadsMatrix(in, slots[k])) { const int rcp = executeHeldPre(in); if (rcp) return rcp; break; }
    int rc = growScratch(in, in->generatorDev, std::min((size_t)G, genChunk) * tableBytes); if (rc) return rc;
    bool fresh = false;
    rc = growDevice(in, in->generatorStatsDev, 2 * sizeof(unsigned), 256, Grow::SyncIfHeld, &fresh); if (rc) return rc;
    if (fresh) HIP_TRY(hipMemsetAsync(in->generatorStatsDev.p, 0, 256, live(in)));
    std::vector<char> pack;
    for (size_t p = 0; p < nParts; p++) {
        const size_t g0 = p * genChunk, nGen = std::min(genChunk, (size_t)G - g0);
        bool tablesDone = false;
        for (size_t first = (size_t)partStart[p]; first < (size_t)partStart[p + 1]; first += entChunk) {
            const size_t m = std::min(entChunk, (size_t)partStart[p + 1] - first);
            // one packed upload per launch: [Q double[nGen][S][S] | mu double[nGen] (first launch of the part only) | lengths double[m] |
            // slot | generator of the part | rate set  int[m] each]
            const size_t qBytes = tablesDone ? 0 : nGen * SS * sizeof(double), muBytes = nGen * sizeof(double),
                         lenBytes = m * sizeof(double), idxBytes = m * sizeof(int), bytes = qBytes + muBytes + lenBytes + 3 * idxBytes;
            pack.resize(bytes);
            if (qBytes) memcpy(pack.data(), Q + g0 * SS, qBytes);
            memcpy(pack.data() + qBytes, mu.data() + g0, muBytes);
            double* pLen = (double*)(pack.data() + qBytes + muBytes);
            int* pIdx = (int*)(pack.data() + qBytes + muBytes + lenBytes);
            for (size_t k = 0; k < m; k++) {
                const int e = order[first + k];
                pLen[k] = lens[e];
                pIdx[k] = slots[e];
                pIdx[m + k] = (genIdx ? genIdx[e] : 0) - (int)g0;
                pIdx[2 * m + k] = rateIdx ? rateIdx[e] : 0;
            }
            void* dPack = nullptr;
            rc = uploadTransient(in, pack.data(), bytes, &dPack); if (rc) return rc;
            const double* dMu = (const double*)((const char*)dPack + qBytes);
            const double* dLen = (const double*)((const char*)dPack + qBytes + muBytes);
            const int* dIdx = (const int*)((const char*)dPack + qBytes + muBytes + lenBytes);
            double* tables = in->generatorDev.as<double>();
            if (!tablesDone && !mi355::launchGeneratorPowers(live(in), tables, (const double*)dPack, dMu, (int)nGen, in->S)) return BEAGLE_ERROR_GENERAL;
            tablesDone = true;
            if (!mi355::launchGeneratorMatrices(live(in), in->matrices, in->rates, tables, dMu, dIdx, dLen, dIdx + m, dIdx + 2 * m,
                                                in->generatorStatsDev.as<unsigned>(), (int)m, in->S, in->C)) return BEAGLE_ERROR_GENERAL;
            HIP_TRY(hipGetLastError());
        }
    }
    in->statGeneratorCalls++; in->statGeneratorMatrices += (long)count * in->C;
    return BEAGLE_SUCCESS;
}

extern "C" {

int beagleMi355UpdateTransitionMatricesFromGenerators(int instance, const double* generators, int generatorCount,
                                                      const int* generatorIndices, const int* categoryRateIndices,
                                                      const int* probabilityIndices, const double* edgeLengths, int count) {
    if (mi355::isShardedHandle(instance)) {
        // (queued: every shard's thread applies its copy; what needs no shard is checked here, a bad index surfaces at the next waiting call)
        const int S = mi355::shardedStates(instance);
        std::vector<double> mu;
        const int rcc = checkGenerators(S, generators, generatorCount, edgeLengths, count, mu); if (rcc) return rcc;
        if (count == 0) return BEAGLE_SUCCESS;
        if (!probabilityIndices) return BEAGLE_ERROR_OUT_OF_RANGE;
        std::vector<double> q(generators, generators + (size_t)generatorCount * S * S), t(edgeLengths, edgeLengths + count);
        std::vector<int> p(probabilityIndices, probabilityIndices + count), g, r;
        if (generatorIndices) g.assign(generatorIndices, generatorIndices + count);
        if (categoryRateIndices) r.assign(categoryRateIndices, categoryRateIndices + count);
        const bool hasG = generatorIndices != nullptr, hasR = categoryRateIndices != nullptr;
        return mi355::shardedPost(instance, [=](int h) {
            return beagleMi355UpdateTransitionMatricesFromGenerators(h, q.data(), generatorCount, hasG ? g.data() : nullptr,
                                                                     hasR ? r.data() : nullptr, p.data(), t.data(), count); });
    }
    GET_INSTANCE_KEEP_PENDING(instance);                      // (a held-back pre-order list waits unless one of ITS matrices is rewritten)
    return generatorMatrices(in, generators, generatorCount, generatorIndices, categoryRateIndices, probabilityIndices, edgeLengths, count);
}

int beagleMi355GeneratorStats(int instance, long* out4) {
    if (mi355::isShardedHandle(instance)) { return mi355::shardedFirst(instance, [&](int h) { return beagleMi355GeneratorStats(h, out4); }); }
    GET_INSTANCE_KEEP_PENDING(instance);
    if (!out4) return BEAGLE_ERROR_OUT_OF_RANGE;
    out4[0] = in->statGeneratorCalls; out4[1] = in->statGeneratorMatrices; out4[2] = out4[3] = 0;
    if (in->generatorStatsDev.p) {
        unsigned words[2] = {0, 0};
        const int rc = download(in, words, in->generatorStatsDev.p, sizeof(words)); if (rc) return rc;
        out4[2] = (long)words[0]; out4[3] = (long)words[1];
    }
    return BEAGLE_SUCCESS;
}

}  // extern "C"
