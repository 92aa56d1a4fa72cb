// engine_nodepattern.cpp — the stochastic Dollo (ALS) node-pattern likelihood in one call (include/beagle_mi355.h
// beagleMi355NodePatternLikelihoods, beagleMi355NodePatternStats; kernels_nodepattern.hip): argument checks, materialising what the
// 4-state walk left unstored, the row descriptors, one launch per chunk of patterns, the ordered sum, the copy-out.
#include "engine_internal.h"

#include <map>

using namespace mi355::eng;
namespace scratch = mi355::scratch;

namespace {

constexpr size_t ROW_SCRATCH_BYTES = 256ull << 20;         // most [slot][chunk] scratch and [row][chunk] stage of one launch

// The list's shape: tips {-1, -1}, an internal row over two different earlier rows, no row a child twice
bool postOrder(const int* nodes, int nodeCount) {
    std::vector<char> used(nodeCount, 0);
    for (int r = 0; r < nodeCount; r++) {
        const int c1 = nodes[4 * r + 2], c2 = nodes[4 * r + 3];
        if (c1 == -1 && c2 == -1) continue;
        if (c1 < 0 || c2 < 0 || c1 >= r || c2 >= r || c1 == c2 || used[c1] || used[c2]) return false;
        used[c1] = used[c2] = 1;
    }
    return true;
}

// One instance's patterns (pOffset .. pOffset + P - 1 of globalP): its columns of the outputs and its own weighted sum
int nodePattern(Instance* in, const int* nodes, const double* logWeights, int nodeCount, int deathState, int wIdx, int fIdx,
                size_t globalP, size_t pOffset, double* outLogPattern, double* outNodeLogTerms, double* sum) {
    if (in->partitionCount > 1 || in->basta || in->S > 255) return BEAGLE_ERROR_NO_IMPLEMENTATION;
    if (badIndex(wIdx, in->eigenCount) || badIndex(fIdx, in->eigenCount) || badIndex(deathState, in->S)) return BEAGLE_ERROR_OUT_OF_RANGE;
    if (!postOrder(nodes, nodeCount) || !in->patternWeights) return BEAGLE_ERROR_OUT_OF_RANGE;
    ReadSet reads(in);
    bool heldWritesOne = false;
    for (int r = 0; r < nodeCount; r++) {
        const int b = nodes[4 * r], sc = nodes[4 * r + 1];
        const bool tip = nodes[4 * r + 2] < 0;
        if (badIndex(b, in->partialsCount)) return BEAGLE_ERROR_OUT_OF_RANGE;
        if (sc != -1 && badIndex(sc, in->scaleCount)) return BEAGLE_ERROR_OUT_OF_RANGE;
        if (!tip && isCompactTip(in, b)) return BEAGLE_ERROR_OUT_OF_RANGE;
        if (int bad = reads.post(b)) return bad;
        heldWritesOne = heldWritesOne || heldWrites(in, b);
    }
    // a held-back pre-order list stays held unless it writes what this call reads (materialising runs programs of its own: it goes first)
    if (in->heldPre.held && (heldWritesOne || reads.keys())) { int rc = executeHeldPre(in); if (rc) return rc; }
    DEMOTE_FOLDED_TIPS(in);
    { int rc = reads.materialize(); if (rc) return rc; }

    // scratch slots: a row's is free again once its parent has read it (the parent may take it over: it reads before it writes)
    std::vector<mi355::NodePatternRow> rows(nodeCount);
    std::vector<int> freeSlots;
    int slots = 0;
    for (int r = 0; r < nodeCount; r++) {
        const int b = nodes[4 * r], sc = nodes[4 * r + 1];
        mi355::NodePatternRow& row = rows[r];
        row = mi355::NodePatternRow{};
        if (isCompactTip(in, b)) row.states = in->tipStates[b];
        else if (in->partials[b]) row.partials = in->partials[b];
        else return BEAGLE_ERROR_OUT_OF_RANGE;
        row.child1 = nodes[4 * r + 2]; row.child2 = nodes[4 * r + 3];
        if (row.child1 >= 0) {
            row.slot1 = rows[row.child1].slot; row.slot2 = rows[row.child2].slot;
            freeSlots.push_back(row.slot2); freeSlots.push_back(row.slot1);
        }
        if (freeSlots.empty()) row.slot = slots++;
        else { row.slot = freeSlots.back(); freeSlots.pop_back(); }
        if (row.child1 >= 0 && sc != -1) {
            int rc = ensureScale(in, sc); if (rc) return rc;
            row.scale = in->scale[sc]; row.scaleRaw = in->scaleIsRaw[sc];
        }
        row.logWeight = logWeights[r];
    }

    const size_t R = (size_t)nodeCount, P = (size_t)in->P, blocks = (size_t)mi355::nodePatternBlocks(in->P);
    const size_t perPattern = (size_t)slots * (sizeof(double) + sizeof(int)) + (outNodeLogTerms ? R * sizeof(double) : 0);
    const size_t fits = std::max<size_t>(256, ROW_SCRATCH_BYTES / perPattern / 256 * 256);
    const size_t chunk = chunkSites("BEAGLE_MI355_NODEPATTERN_CHUNK", 256, fits, P);
    const scratch::NodePatternLayout L((size_t)slots, R, P, chunk, blocks, outNodeLogTerms != nullptr);
    int rc = growScratch(in, in->nodePatternDev, L.bytes()); if (rc) return rc;
    char* base = in->nodePatternDev.p;
    double *dLog = L.logPattern.at(base), *dBlocks = L.blockSums.at(base), *dSum = L.sum.at(base), *dTerms = L.terms.at(base);
    void* dRows = nullptr;
    rc = uploadTransient(in, rows.data(), rows.size() * sizeof(mi355::NodePatternRow), &dRows); if (rc) return rc;
    for (size_t c0 = 0; c0 < P; c0 += chunk) {
        const size_t n = std::min(chunk, P - c0);
        mi355::launchNodePattern(live(in), (const mi355::NodePatternRow*)dRows, nodeCount, in->weights + (size_t)wIdx * in->C,
                                 in->freqs + (size_t)fIdx * in->S, in->patternWeights, in->P, in->S, in->C, in->tiled, deathState,
                                 (int)c0, (int)n, (int)chunk, L.lambda.at(base), L.below.at(base), dTerms, dLog, dBlocks);
        HIP_TRY(hipGetLastError());
        if (outNodeLogTerms) {                                 // the stage's columns to theirs of out[row][globalP]; the next chunk overwrites it
            HIP_TRY(hipMemcpy2DAsync(outNodeLogTerms + pOffset + c0, globalP * sizeof(double), dTerms, chunk * sizeof(double),
                                     n * sizeof(double), R, hipMemcpyDeviceToHost, live(in)));
            if (c0 + chunk < P) HIP_TRY(hipStreamSynchronize(live(in)));
        }
    }
    mi355::launchBlockTotals(live(in), dBlocks, (int)blocks, 1, 1, 0, dSum);
    HIP_TRY(hipGetLastError());
    std::vector<double> back(P + blocks + 1);                  // log pattern values | block sums | the sum: one copy
    rc = download(in, back.data(), dLog, back.size() * sizeof(double)); if (rc) return rc;
    memcpy(outLogPattern + pOffset, back.data(), P * sizeof(double));
    *sum = back[P + blocks];
    long empty = 0;
    for (size_t p = 0; p < P; p++) if (back[p] == -INFINITY) empty++;
    in->statNodePatternCalls++; in->statNodePatternRows += nodeCount; in->statNodePatternEmpty += empty;
    in->statNodePatternMaterialised += (long)reads.keys();
    return BEAGLE_SUCCESS;
}

}  // namespace

extern "C" {

int beagleMi355NodePatternLikelihoods(int instance, const int* nodes, const double* nodeLogWeights, int nodeCount, int deathState,
                                      int categoryWeightsIndex, int stateFrequenciesIndex, int flags, double* outLogPattern,
                                      double* outNodeLogTerms, double* outSum) {
    if (!nodes || !nodeLogWeights || !outLogPattern || nodeCount < 1 || flags != 0) return BEAGLE_ERROR_OUT_OF_RANGE;
    // every shard (a plain handle: the instance) fills its own columns; the sum is the shards' sums, added in shard (= pattern) order
    std::mutex mu;
    std::map<int, mi355::ShardPart> parts;
    const int rc = mi355::shardedOrPlain(instance, [&](int h) -> int {
        GET_INSTANCE_KEEP_PENDING(h);
        int globalP = in->P, pEnd = 0;
        mi355::ShardPart part;
        if (mi355::isShardedHandle(instance)) { mi355::shardedBoundsOfHandle(instance, h, &part.start, &pEnd); globalP = mi355::shardedPatternCount(instance); }
        part.rowTotals.assign(1, 0.0);
        const int r = nodePattern(in, nodes, nodeLogWeights, nodeCount, deathState, categoryWeightsIndex, stateFrequenciesIndex,
                                  (size_t)globalP, (size_t)part.start, outLogPattern, outNodeLogTerms, part.rowTotals.data());
        std::lock_guard<std::mutex> lock(mu);
        parts[h] = std::move(part);
        return r;
    });
    if (rc) return rc;
    double sum = 0.0;
    mi355::sumRowTotals(mi355::orderedParts(parts), 1, &sum);
    if (outSum) *outSum = sum;
    return std::isfinite(sum) ? BEAGLE_SUCCESS : BEAGLE_ERROR_FLOATING_POINT;
}

int beagleMi355NodePatternStats(int instance, long* out4) {
    if (!out4) return BEAGLE_ERROR_OUT_OF_RANGE;
    std::mutex mu;
    long total[4] = {0, 0, 0, 0};
    const int rc = mi355::shardedOrPlain(instance, [&](int h) -> int {
        GET_INSTANCE_KEEP_PENDING(h);
        std::lock_guard<std::mutex> lock(mu);
        total[0] += in->statNodePatternCalls; total[1] += in->statNodePatternRows; total[2] += in->statNodePatternEmpty;
        total[3] += in->statNodePatternMaterialised;
        return (int)BEAGLE_SUCCESS;
    });
    if (rc) return rc;
    for (int k = 0; k < 4; k++) out4[k] = total[k];
    return BEAGLE_SUCCESS;
}

}  // extern "C"
