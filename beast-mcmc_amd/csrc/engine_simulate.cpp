// engine_simulate.cpp — sequence simulation (include/beagle_mi355.h beagleMi355SimulateSequences): an alignment drawn from the model
// down the tree, from the branch matrices where they are.  What dr.app.beagle.tools.Partition.traverse computes from an
// updateTransitionMatrices and a getTransitionMatrix per branch and one randomChoicePDF per site and branch in Java
// (Partition.java:292-431, :519-536).
#include "engine_internal.h"

using namespace mi355::eng;

// ---- the front end shared with engine_history.cpp (engine_internal.h)
int mi355::eng::checkSiteCall(const int* nodes, int nodeCount, int siteCount, const unsigned char* inRootStates,
                              const int* inRateCategories, int S, int C, int* maxOut) {
    std::vector<int> used;
    *maxOut = -1;
    for (int r = 0; r < nodeCount; r++) {
        const int out = nodes[3 * r], parent = nodes[3 * r + 2];
        if (out < -1) return BEAGLE_ERROR_OUT_OF_RANGE;
        if (r > 0 && (parent < 0 || parent >= r)) return BEAGLE_ERROR_OUT_OF_RANGE;
        if (out >= 0) { used.push_back(out); *maxOut = std::max(*maxOut, out); }
    }
    std::sort(used.begin(), used.end());
    if (std::adjacent_find(used.begin(), used.end()) != used.end()) return BEAGLE_ERROR_OUT_OF_RANGE;
    if (inRootStates)
        for (int s = 0; s < siteCount; s++)
            if (inRootStates[s] >= S) return BEAGLE_ERROR_OUT_OF_RANGE;
    if (inRateCategories)
        for (int s = 0; s < siteCount; s++)
            if (inRateCategories[s] < 0 || inRateCategories[s] >= C) return BEAGLE_ERROR_OUT_OF_RANGE;
    return 0;
}

size_t mi355::eng::chunkSites(const char* envName, size_t unit, size_t wanted, size_t sites) {
    if (const char* e = getenv(envName)) {
        const long v = atol(e);
        if (v > 0) wanted = (size_t)v;
    }
    return (std::min(wanted, sites) + unit - 1) / unit * unit;
}

int mi355::eng::SiteSplit::init(int handle, int sites) {
    siteCount = sites;
    if (mi355::isShardedHandle(handle)) {
        shards = mi355::shardedShardCount(handle); S = mi355::shardedStates(handle); C = mi355::shardedCategories(handle);
        return shards < 1 ? BEAGLE_ERROR_UNINITIALIZED_INSTANCE : 0;
    }
    GET_INSTANCE(handle);
    S = in->S; C = in->C;
    return 0;
}

std::vector<int> mi355::eng::wantedRows(const int* nodes, int nodeCount) {
    std::vector<int> wanted;
    for (int r = 0; r < nodeCount; r++) if (nodes[3 * r] >= 0) wanted.push_back(nodes[3 * r]);
    std::sort(wanted.begin(), wanted.end());
    return wanted;
}

int mi355::eng::copyWantedRows(Instance* in, const std::vector<int>& wanted, const uint8_t* dStates, size_t chunk, size_t count,
                               unsigned char* outStates, size_t siteCount, size_t first) {
    for (size_t a = 0; a < wanted.size();) {
        size_t b = a + 1;
        while (b < wanted.size() && wanted[b] == wanted[b - 1] + 1) b++;
        HIP_TRY(hipMemcpy2DAsync(outStates + (size_t)wanted[a] * siteCount + first, siteCount, dStates + (size_t)wanted[a] * chunk, chunk,
                                 count, b - a, hipMemcpyDeviceToHost, live(in)));
        a = b;
    }
    return 0;
}

namespace {

constexpr size_t SIM_SCRATCH_BYTES = 256ull << 20;       // the states of one chunk of sites (the Markov-jump gather's rule)

// Sites site0 .. site1 - 1 of a call over siteCount sites (the sharded handle: this instance's part; otherwise all of them): the
// random numbers are keyed on the site of the whole call, and a row's states land at outStates + outRow * siteCount + site.
int simulate(Instance* in, const int* nodes, int nodeCount, std::vector<mi355::SimRow> rows, size_t slots, int siteCount, int site0,
             int site1, int wIdx, int fIdx, unsigned long long seed, const unsigned char* inRootStates, const int* inRateCategories,
             unsigned char* outStates, int* outCategories) {
    if (badIndex(wIdx, in->eigenCount) || badIndex(fIdx, in->eigenCount)) return BEAGLE_ERROR_OUT_OF_RANGE;
    const int S = in->S, C = in->C;
    const size_t n = (size_t)C * S * S;
    for (int r = 1; r < nodeCount; r++) {
        const int m = nodes[3 * r + 1];
        if (badIndex(m, in->matrixCount)) return BEAGLE_ERROR_OUT_OF_RANGE;
        rows[r].matrix = in->matrices + n * m;           // the caller's slot, never a folded tip's shadow
    }
    if (site1 <= site0) return 0;
    // BEAGLE_MI355_SIM_CHUNK_SITES=<n>: the sites of one launch; otherwise as many as keep the states within SIM_SCRATCH_BYTES.  A
    // multiple of SIM_SITES_PER_THREAD, so that every chunk starts on a packed word.
    const size_t W = mi355::SIM_SITES_PER_THREAD, sites = (size_t)(site1 - site0);
    const size_t chunk = chunkSites("BEAGLE_MI355_SIM_CHUNK_SITES", W, std::max<size_t>(W, SIM_SCRATCH_BYTES / slots), sites);
    const mi355::scratch::SimulateLayout L(slots, chunk, mi355::simTableDoubles(nodeCount, S, C), mi355::simTableRows(nodeCount, S, C));
    int rc = growScratch(in, in->simulateDev, L.bytes()); if (rc) return rc;
    char* base = in->simulateDev.p;
    uint8_t* dStates = L.states.at(base);
    int* dCats = L.cats.at(base);
    unsigned* dErr = L.error.at(base);
    double* dTable = L.table.at(base);
    int* dMeta = L.meta.at(base);
    void* dRowsV = nullptr;
    rc = uploadTransient(in, rows.data(), rows.size() * sizeof(mi355::SimRow), &dRowsV); if (rc) return rc;
    const mi355::SimRow* dRows = (const mi355::SimRow*)dRowsV;
    HIP_TRY(hipMemsetAsync(dErr, 0, sizeof(unsigned), live(in)));
    mi355::launchSimTables(live(in), dRows, nodeCount, in->weights + (size_t)wIdx * C, in->freqs + (size_t)fIdx * S, S, C, dTable, dMeta);
    HIP_TRY(hipGetLastError());
    const std::vector<int> wanted = wantedRows(nodes, nodeCount);
    for (size_t c0 = 0; c0 < sites; c0 += chunk) {
        const size_t count = std::min(chunk, sites - c0), first = (size_t)site0 + c0;
        if (inRootStates) { rc = upload(in, dStates + (size_t)rows[0].slot * chunk, inRootStates + first, count); if (rc) return rc; }
        if (inRateCategories) { rc = upload(in, dCats, inRateCategories + first, count * sizeof(int)); if (rc) return rc; }
        mi355::launchSimSites(live(in), dRows, nodeCount, dTable, dMeta, S, C, (int)count, chunk, (unsigned long long)siteCount,
                              (unsigned long long)first, seed, inRootStates != nullptr, inRateCategories != nullptr, dStates, dCats, dErr);
        HIP_TRY(hipGetLastError());
        rc = copyWantedRows(in, wanted, dStates, chunk, count, outStates, (size_t)siteCount, first); if (rc) return rc;
        if (outCategories) HIP_TRY(hipMemcpyAsync(outCategories + first, dCats, count * sizeof(int), hipMemcpyDeviceToHost, live(in)));
        HIP_TRY(hipStreamSynchronize(live(in)));             // (the next chunk overwrites the scratch rows)
    }
    unsigned err = 0;
    rc = download(in, &err, dErr, sizeof(unsigned)); if (rc) return rc;
    return err ? BEAGLE_ERROR_FLOATING_POINT : BEAGLE_SUCCESS;
}

}  // namespace

extern "C" {

int beagleMi355SimulateSequences(int instance, const int* nodes, int nodeCount, int siteCount, int categoryWeightsIndex,
                                 int stateFrequenciesIndex, unsigned long long seed, int flags, const unsigned char* inRootStates,
                                 const int* inRateCategories, unsigned char* outStates, int* outRateCategories) {
    SiteSplit split;
    int rc = split.init(instance, siteCount); if (rc) return rc;
    // what does not depend on the instance's buffers: the node list's shape, the flags, the caller's input states and categories
    if (!nodes || !outStates || nodeCount < 1 || siteCount < 1 || flags != 0) return BEAGLE_ERROR_OUT_OF_RANGE;
    int maxOut = -1;
    rc = checkSiteCall(nodes, nodeCount, siteCount, inRootStates, inRateCategories, split.S, split.C, &maxOut); if (rc) return rc;
    std::vector<mi355::SimRow> rows(nodeCount, mi355::SimRow{});
    size_t slots = 0;
    rc = assignSlots(nodes, nodeCount, maxOut, rows, &slots); if (rc) return rc;
    // every shard holds all matrices and draws its part of the sites into its columns
    return mi355::shardedOrPlain(instance, [&](int h) -> int {
        int site0 = 0, site1 = 0;
        if (!split.next(&site0, &site1)) return BEAGLE_ERROR_GENERAL;
        GET_INSTANCE(h);
        return simulate(in, nodes, nodeCount, rows, slots, siteCount, site0, site1, categoryWeightsIndex, stateFrequenciesIndex, seed,
                        inRootStates, inRateCategories, outStates, outRateCategories);
    });
}

}  // extern "C"
