// engine_nodeposterior.cpp — marginal node state posteriors in one call (include/beagle_mi355.h beagleMi355NodePosteriors,
// beagleMi355NodePosteriorStats; kernels_nodeposterior.hip): argument checks, materialising what the 4-state walk left unstored, the
// row descriptors, one launch per chunk of rows, the ordered totals, the copy-out.
#include "engine_internal.h"

#include <map>

using namespace mi355::eng;
namespace scratch = mi355::scratch;

namespace {

constexpr size_t OUTPUT_SCRATCH_BYTES = 256ull << 20;      // most per-row output scratch of one launch

struct Outputs { double* posteriors; unsigned char* mapStates; double* mapProbabilities; double* categories; };

// One instance's patterns (pOffset .. pOffset + P - 1 of globalP): its columns of the per-pattern outputs, its own state totals
// (totals: [nodeCount][S], nullptr when not wanted), *fpError set when a Z was 0 or not finite
int nodePosteriors(Instance* in, const int* nodes, int nodeCount, int wIdx, size_t globalP, size_t pOffset, const Outputs& out,
                   double* totals, bool* fpError) {
    if (in->partitionCount > 1 || in->basta || in->S > 255) return BEAGLE_ERROR_NO_IMPLEMENTATION;
    if (badIndex(wIdx, in->eigenCount) || (totals && !in->patternWeights)) return BEAGLE_ERROR_OUT_OF_RANGE;
    long unstoredAtEntry = 0;
    int rc = makeResident(in, [&](ReadSet& reads) -> int {
        for (int r = 0; r < nodeCount; r++) {
            const int post = nodes[2 * r], pre = nodes[2 * r + 1];
            if (badIndex(post, in->partialsCount) || badIndex(pre, in->partialsCount)) return BEAGLE_ERROR_OUT_OF_RANGE;
            if (int bad = reads.pre(pre)) return bad;
            if (int bad = reads.post(post)) return bad;
        }
        return 0;
    }, &unstoredAtEntry);
    if (rc) return rc;

    const size_t R = (size_t)nodeCount, P = (size_t)in->P, S = (size_t)in->S, C = (size_t)in->C, blocks = (size_t)mi355::edgeBlocks(in->P);
    const bool full = out.posteriors != nullptr, map = out.mapStates || out.mapProbabilities, wantTotals = totals != nullptr;
    // rows per launch: the descriptors fit a quarter of the staging ring, the outputs' scratch its budget, the grid its second dimension
    const size_t perRow = (full ? P * S * sizeof(double) : 0) + (map ? P * (sizeof(double) + 1) : 0) + (wantTotals ? (blocks + 1) * S * sizeof(double) : 0);
    size_t chunk = std::min<size_t>({R, (RING_BYTES / 4) / sizeof(mi355::NodePosteriorRow), (size_t)mi355::NODE_POSTERIOR_MAX_ROWS});
    if (perRow) chunk = std::min(chunk, std::max<size_t>(1, OUTPUT_SCRATCH_BYTES / perRow));
    chunk = chunkSites("BEAGLE_MI355_NODE_POSTERIOR_CHUNK", 1, chunk, chunk);
    const scratch::NodePosteriorLayout L(chunk, P, S, C, blocks, full, map, wantTotals, out.categories != nullptr);
    rc = growScratch(in, in->nodePosteriorDev, L.bytes()); if (rc) return rc;
    char* base = in->nodePosteriorDev.p;
    double *dPost = L.posteriors.at(base), *dProb = L.mapProb.at(base), *dBlocks = L.blockSums.at(base), *dTotals = L.totals.at(base);
    double* dCats = L.categories.at(base);
    uint8_t* dStates = L.mapStates.at(base);
    unsigned* dError = L.error.at(base);
    HIP_TRY(hipMemsetAsync(dError, 0, sizeof(unsigned), live(in)));
    CallTimer timer(in);
    const double* weights = in->weights + (size_t)wIdx * in->C;
    std::vector<mi355::NodePosteriorRow> rows;
    int launches = 0;
    for (size_t b = 0; b < R && !rc; b += chunk) {
        const size_t m = std::min(chunk, R - b);
        rows.assign(m, mi355::NodePosteriorRow{});
        for (size_t e = 0; e < m; e++) {
            mi355::NodePosteriorRow& row = rows[e];
            row.post = postOperand(in, nodes[2 * (b + e)], &row.statesPost);
            row.pre = preOperand(in, nodes[2 * (b + e) + 1]);
            row.slot = (int)e;
            if (!row.post || !row.pre) { rc = BEAGLE_ERROR_OUT_OF_RANGE; break; }
        }
        if (rc) break;
        void* dRows = nullptr;
        rc = uploadTransient(in, rows.data(), m * sizeof(mi355::NodePosteriorRow), &dRows); if (rc) break;
        rc = timer.start(); if (rc) break;
        if (full || map || wantTotals) {
            if (!mi355::launchNodePosteriors(live(in), (const mi355::NodePosteriorRow*)dRows, (int)m, weights, in->patternWeights, in->P, in->S,
                                             in->C, in->tiled, dPost, out.mapStates ? dStates : nullptr, out.mapProbabilities ? dProb : nullptr,
                                             dBlocks, dError)) { rc = BEAGLE_ERROR_GENERAL; break; }
            launches++;
        }
        if (wantTotals) { mi355::launchBlockTotals(live(in), dBlocks, (int)blocks, 1, (int)(m * S), 0, dTotals); launches++; }
        if (out.categories && b == 0) {
            mi355::launchNodePosteriorCategories(live(in), (const mi355::NodePosteriorRow*)dRows, weights, in->P, in->S, in->C, in->tiled, dCats, dError);
            launches++;
        }
        if (hipGetLastError() != hipSuccess) { rc = BEAGLE_ERROR_GENERAL; break; }
        if (b + m >= R) { rc = timer.stop(launches); if (rc) break; }
        // this launch's rows to theirs of the outputs; the next launch overwrites the scratch, so the last copy is waited for
        // (the states: linear where the instance has every column, as copyStagedRows does — a strided copy goes row by row)
        if (out.mapStates && (globalP == P ? hipMemcpyAsync(out.mapStates + b * P, dStates, m * P, hipMemcpyDeviceToHost, live(in))
                                           : hipMemcpy2DAsync(out.mapStates + b * globalP + pOffset, globalP, dStates, P, P, m, hipMemcpyDeviceToHost, live(in))) != hipSuccess) { rc = BEAGLE_ERROR_GENERAL; break; }
        if (out.categories && b == 0 &&
            hipMemcpyAsync(out.categories + pOffset * C, dCats, P * C * sizeof(double), hipMemcpyDeviceToHost, live(in)) != hipSuccess) { rc = BEAGLE_ERROR_GENERAL; break; }
        if (wantTotals &&
            hipMemcpyAsync(totals + b * S, dTotals, m * S * sizeof(double), hipMemcpyDeviceToHost, live(in)) != hipSuccess) { rc = BEAGLE_ERROR_GENERAL; break; }
        if (out.mapProbabilities) { rc = copyStagedRows(in, dProb, m, b, b + m, 1, R, P, globalP, pOffset, out.mapProbabilities); if (rc) break; }
        if (full) { rc = copyStagedRows(in, dPost, m, b, b + m, 1, R, P * S, globalP * S, pOffset * S, out.posteriors); if (rc) break; }
        if (hipStreamSynchronize(live(in)) != hipSuccess) { rc = BEAGLE_ERROR_GENERAL; break; }
    }
    if (rc) return rc;
    unsigned err = 0;
    rc = download(in, &err, dError, sizeof(err)); if (rc) return rc;
    if (err) *fpError = true;
    in->statNodePosteriorCalls++; in->statNodePosteriorRows += nodeCount; in->statNodePosteriorMaterialised += unstoredAtEntry;
    in->statNodePosteriorLaunches += launches;
    return BEAGLE_SUCCESS;
}

}  // namespace

extern "C" {

int beagleMi355NodePosteriors(int instance, const int* nodes, int nodeCount, int categoryWeightsIndex, int flags,
                              double* outPosteriors, unsigned char* outMapStates, double* outMapProbabilities,
                              double* outStateTotals, double* outCategoryPosteriors) {
    if (!nodes || nodeCount < 1 || flags != 0) return BEAGLE_ERROR_OUT_OF_RANGE;
    if (!outPosteriors && !outMapStates && !outMapProbabilities && !outStateTotals && !outCategoryPosteriors) return BEAGLE_ERROR_OUT_OF_RANGE;
    // every shard (a plain handle: the instance) fills its own columns; the totals are the shards' totals, added in shard (= pattern) order
    const Outputs out = {outPosteriors, outMapStates, outMapProbabilities, outCategoryPosteriors};
    std::mutex mu;
    std::map<int, mi355::ShardPart> parts;
    std::atomic<bool> fpError{false};
    const int rc = mi355::shardedOrPlain(instance, [&](int h) -> int {
        GET_INSTANCE_KEEP_PENDING(h);           // (the list is checked before a held-back pre-order list runs: nodePosteriors)
        int globalP = in->P, pEnd = 0;
        mi355::ShardPart part;
        if (mi355::isShardedHandle(instance)) {
            mi355::shardedBoundsOfHandle(instance, h, &part.start, &pEnd); globalP = mi355::shardedPatternCount(instance);
            if (pEnd - part.start != in->P || pEnd > globalP) return (int)BEAGLE_ERROR_GENERAL;      // (the columns this shard is about to fill)
        }
        part.rowTotals.assign(outStateTotals ? (size_t)nodeCount * in->S : 0, 0.0);
        bool bad = false;
        const int r = nodePosteriors(in, nodes, nodeCount, categoryWeightsIndex, (size_t)globalP, (size_t)part.start, out,
                                     outStateTotals ? part.rowTotals.data() : nullptr, &bad);
        if (bad) fpError = true;
        std::lock_guard<std::mutex> lock(mu);
        parts[h] = std::move(part);
        return r;
    });
    if (rc) return rc;
    if (outStateTotals) mi355::sumRowTotals(mi355::orderedParts(parts), parts.begin()->second.rowTotals.size(), outStateTotals);
    return fpError ? BEAGLE_ERROR_FLOATING_POINT : BEAGLE_SUCCESS;
}

int beagleMi355NodePosteriorStats(int instance, long* out4) {
    if (!out4) return BEAGLE_ERROR_OUT_OF_RANGE;
    auto read = [&](int h) -> int {
        GET_INSTANCE_KEEP_PENDING(h);
        out4[0] = in->statNodePosteriorCalls; out4[1] = in->statNodePosteriorRows; out4[2] = in->statNodePosteriorMaterialised;
        out4[3] = in->statNodePosteriorLaunches;
        return (int)BEAGLE_SUCCESS;
    };
    return mi355::isShardedHandle(instance) ? mi355::shardedFirst(instance, read) : read(instance);
}

}  // extern "C"
