// engine_simulate.cpp — sequence simulation (include/beagle_mi355.h beagleMi355SimulateSequences): an alignment drawn from the model
// down the tree, from the branch matrices where they are.  What dr.app.beagle.tools.Partition.traverse computes from an
// updateTransitionMatrices and a getTransitionMatrix per branch and one randomChoicePDF per site and branch in Java
// (Partition.java:292-431, :519-536).
#include "engine_internal.h"

#include <climits>

using namespace mi355::eng;

namespace {

constexpr size_t SIM_SCRATCH_BYTES = 256ull << 20;       // the states of one chunk of sites (the Markov-jump gather's rule)

size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }

// What does not depend on the instance's buffers: the node list's shape, the flags, the caller's input states and categories.
// *slots: scratch rows — a node with an outRow keeps its states in scratch row outRow (so that the wanted rows leave as a few
// strided copies), the others behind the largest outRow.
int checkCall(const int* nodes, int nodeCount, int siteCount, int flags, const unsigned char* inRootStates, const int* inRateCategories,
              const unsigned char* outStates, int S, int C, std::vector<mi355::SimRow>* rows, size_t* slots) {
    if (!nodes || !outStates || nodeCount < 1 || siteCount < 1 || flags != 0) return BEAGLE_ERROR_OUT_OF_RANGE;
    std::vector<int> used;
    int maxOut = -1;
    for (int r = 0; r < nodeCount; r++) {
        const int out = nodes[3 * r], parent = nodes[3 * r + 2];
        if (out < -1) return BEAGLE_ERROR_OUT_OF_RANGE;
        if (r > 0 && (parent < 0 || parent >= r)) return BEAGLE_ERROR_OUT_OF_RANGE;
        if (out >= 0) { used.push_back(out); maxOut = std::max(maxOut, out); }
    }
    std::sort(used.begin(), used.end());
    if (std::adjacent_find(used.begin(), used.end()) != used.end()) return BEAGLE_ERROR_OUT_OF_RANGE;
    if (inRootStates)
        for (int s = 0; s < siteCount; s++)
            if (inRootStates[s] >= S) return BEAGLE_ERROR_OUT_OF_RANGE;
    if (inRateCategories)
        for (int s = 0; s < siteCount; s++)
            if (inRateCategories[s] < 0 || inRateCategories[s] >= C) return BEAGLE_ERROR_OUT_OF_RANGE;
    rows->assign(nodeCount, mi355::SimRow{});
    size_t next = (size_t)maxOut + 1;
    for (int r = 0; r < nodeCount; r++) {
        const int out = nodes[3 * r];
        const size_t slot = out >= 0 ? (size_t)out : next++;
        if (slot > (size_t)INT_MAX) return BEAGLE_ERROR_OUT_OF_RANGE;
        mi355::SimRow& row = (*rows)[r];
        row.matrix = nullptr;
        row.slot = (int)slot;
        row.parentSlot = r == 0 ? -1 : (*rows)[nodes[3 * r + 2]].slot;
        row.parentIsPrev = r > 0 && nodes[3 * r + 2] == r - 1;
        row.pad = 0;
    }
    *slots = next;
    return 0;
}

// BEAGLE_MI355_SIM_CHUNK_SITES=<n>: the sites of one launch (tests: chunk independence at a small size); otherwise as many as keep
// the states within SIM_SCRATCH_BYTES.  A multiple of SIM_SITES_PER_THREAD, so that every chunk starts on a packed word.
size_t chunkSites(size_t slots, size_t sites) {
    const size_t K = mi355::SIM_SITES_PER_THREAD;
    size_t chunk = std::max<size_t>(K, SIM_SCRATCH_BYTES / slots);
    if (const char* e = getenv("BEAGLE_MI355_SIM_CHUNK_SITES")) {
        const long v = atol(e);
        if (v > 0) chunk = (size_t)v;
    }
    chunk = std::min(chunk, sites);
    return (chunk + K - 1) / K * K;
}

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
    const size_t sites = (size_t)(site1 - site0), chunk = chunkSites(slots, sites);
    // simulateDev: states [slots][chunk] | categories int [chunk] | error word | tables (doubles) | meta (ints)
    const size_t oCats = up256(slots * chunk), oErr = oCats + chunk * sizeof(int), oTable = up256(oErr + sizeof(unsigned));
    const size_t oMeta = oTable + mi355::simTableDoubles(nodeCount, S, C) * sizeof(double);
    const size_t bytes = oMeta + mi355::simTableRows(nodeCount, S, C) * sizeof(int);
    int rc = growDevice(in, in->simulateDev, bytes, bytes, Grow::SyncIfHeld); if (rc) return rc;
    char* base = in->simulateDev.p;
    uint8_t* dStates = (uint8_t*)base;
    int* dCats = (int*)(base + oCats);
    unsigned* dErr = (unsigned*)(base + oErr);
    double* dTable = (double*)(base + oTable);
    int* dMeta = (int*)(base + oMeta);
    void* dRowsV = nullptr;
    rc = uploadTransient(in, rows.data(), rows.size() * sizeof(mi355::SimRow), &dRowsV); if (rc) return rc;
    const mi355::SimRow* dRows = (const mi355::SimRow*)dRowsV;
    HIP_TRY(hipMemsetAsync(dErr, 0, sizeof(unsigned), live(in)));
    mi355::launchSimTables(live(in), dRows, nodeCount, in->weights + (size_t)wIdx * C, in->freqs + (size_t)fIdx * S, S, C, dTable, dMeta);
    HIP_TRY(hipGetLastError());
    // the rows to copy out, as runs of consecutive outRows (= consecutive scratch rows): one strided copy each
    std::vector<int> wanted;
    for (int r = 0; r < nodeCount; r++) if (nodes[3 * r] >= 0) wanted.push_back(nodes[3 * r]);
    std::sort(wanted.begin(), wanted.end());
    for (size_t c0 = 0; c0 < sites; c0 += chunk) {
        const size_t count = std::min(chunk, sites - c0), first = (size_t)site0 + c0;
        if (inRootStates) { rc = upload(in, dStates + (size_t)rows[0].slot * chunk, inRootStates + first, count); if (rc) return rc; }
        if (inRateCategories) { rc = upload(in, dCats, inRateCategories + first, count * sizeof(int)); if (rc) return rc; }
        mi355::launchSimSites(live(in), dRows, nodeCount, dTable, dMeta, S, C, (int)count, chunk, (unsigned long long)siteCount,
                              (unsigned long long)first, seed, inRootStates != nullptr, inRateCategories != nullptr, dStates, dCats, dErr);
        HIP_TRY(hipGetLastError());
        for (size_t a = 0; a < wanted.size();) {
            size_t b = a + 1;
            while (b < wanted.size() && wanted[b] == wanted[b - 1] + 1) b++;
            HIP_TRY(hipMemcpy2DAsync(outStates + (size_t)wanted[a] * siteCount + first, (size_t)siteCount, dStates + (size_t)wanted[a] * chunk,
                                     chunk, count, b - a, hipMemcpyDeviceToHost, live(in)));
            a = b;
        }
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
    std::vector<mi355::SimRow> rows;
    size_t slots = 0;
    if (mi355::isShardedHandle(instance)) {
        // every shard holds all matrices: shard k of n draws sites [siteCount k / n, siteCount (k + 1) / n) into its columns
        const int shards = mi355::shardedShardCount(instance);
        if (shards < 1) return BEAGLE_ERROR_UNINITIALIZED_INSTANCE;
        int rc = checkCall(nodes, nodeCount, siteCount, flags, inRootStates, inRateCategories, outStates, mi355::shardedStates(instance),
                           mi355::shardedCategories(instance), &rows, &slots);
        if (rc) return rc;
        // (which shard takes which part does not matter — the bytes are keyed on the site — so the parts go out in order of arrival)
        std::atomic<int> arrivals{0};
        return mi355::shardedBroadcast(instance, [&](int h) -> int {
            const int k = arrivals.fetch_add(1);
            if (k >= shards) return BEAGLE_ERROR_GENERAL;
            const int site0 = (int)((long long)siteCount * k / shards), site1 = (int)((long long)siteCount * (k + 1) / shards);
            GET_INSTANCE(h);
            return simulate(in, nodes, nodeCount, rows, slots, siteCount, site0, site1, categoryWeightsIndex, stateFrequenciesIndex, seed,
                            inRootStates, inRateCategories, outStates, outRateCategories);
        });
    }
    GET_INSTANCE(instance);
    int rc = checkCall(nodes, nodeCount, siteCount, flags, inRootStates, inRateCategories, outStates, in->S, in->C, &rows, &slots);
    if (rc) return rc;
    return simulate(in, nodes, nodeCount, std::move(rows), slots, siteCount, 0, siteCount, categoryWeightsIndex, stateFrequenciesIndex, seed,
                    inRootStates, inRateCategories, outStates, outRateCategories);
}

}  // extern "C"
