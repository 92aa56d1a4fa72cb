// engine_regraft.cpp — scores of hanging a pruned subtree at candidate points of the tree it was cut from in one call
// (include/beagle_mi355.h beagleMi355RegraftScores, beagleMi355RegraftStats; kernels_regraft.hip): argument checks, materialising what
// the 4-state walk left unstored, the pendant vectors, then per chunk of candidates the log ratios, the weighted pattern sum and the
// copy-out.
#include "engine_internal.h"

#include <map>

using namespace mi355::eng;
namespace scratch = mi355::scratch;

namespace {

constexpr size_t RATIO_SCRATCH_BYTES = 256ull << 20;       // most log-ratio scratch of one launch

int regraftScores(Instance* in, const int* cands, int candidateCount, int subtree, int subtreeScale, int wIdx, double* outScores,
                  double* outRatios, bool* fpError) {
    if (in->partitionCount > 1 || in->basta || in->S > 255) return BEAGLE_ERROR_NO_IMPLEMENTATION;
    if (badIndex(wIdx, in->eigenCount) || badIndex(subtree, in->partialsCount) || !in->patternWeights) return BEAGLE_ERROR_OUT_OF_RANGE;
    if (subtreeScale != BEAGLE_OP_NONE && badIndex(subtreeScale, in->scaleCount)) return BEAGLE_ERROR_OUT_OF_RANGE;
    long unstoredAtEntry = 0;
    int rc = makeResident(in, [&](ReadSet& reads) -> int {
        for (int k = 0; k < candidateCount; k++)
            if (int bad = checkAttachment(in, cands + ATTACH_FIELDS * k, reads)) return bad;
        return reads.post(subtree);
    }, &unstoredAtEntry);
    if (rc) return rc;
    if (mi355::regraftPatternBlock(in->S) == 0) return BEAGLE_ERROR_NO_IMPLEMENTATION;
    const double* dScale = nullptr;
    bool scaleRaw = false;
    if (subtreeScale != BEAGLE_OP_NONE) {
        rc = ensureScale(in, subtreeScale); if (rc) return rc;
        dScale = in->scale[subtreeScale]; scaleRaw = in->scaleIsRaw[subtreeScale] != 0;
    }

    const size_t K = (size_t)candidateCount, P = (size_t)in->P, segments = (size_t)mi355::regraftSegments(in->P);
    const size_t perVector = mi355::regraftPendantDoubles(in->P, in->S, in->C, in->tiled);
    // the distinct pendant matrices, in order of first appearance
    std::map<int, int> pendantOf;
    std::vector<int> slots;
    for (size_t k = 0; k < K; k++) {
        const int m = cands[ATTACH_FIELDS * k + ATTACH_PENDANT_MATRIX];
        if (pendantOf.emplace(m, (int)slots.size()).second) slots.push_back(m);
    }
    // candidates per launch: the descriptors fit a quarter of the staging ring, the log ratios their budget, the grid its second dimension
    size_t chunk = std::min<size_t>({K, (RING_BYTES / 4) / sizeof(mi355::PlacementCandidate), (size_t)mi355::REGRAFT_MAX_CANDIDATES,
                                     std::max<size_t>(1, RATIO_SCRATCH_BYTES / (P * sizeof(double)))});
    chunk = std::min<size_t>(chunkSites("BEAGLE_MI355_REGRAFT_CHUNK", 1, chunk, K), (size_t)mi355::REGRAFT_MAX_CANDIDATES);
    const scratch::RegraftLayout L(chunk, slots.size(), perVector, segments, P);
    rc = growScratch(in, in->regraftDev, L.bytes()); if (rc) return rc;
    char* base = in->regraftDev.p;
    double *dPendants = L.pendants.at(base), *dRatios = L.ratios.at(base), *dPartial = L.partial.at(base), *dScores = L.scores.at(base);
    int* dSlots = L.slots.at(base);
    unsigned* dError = L.error.at(base);
    int subtreeStates = 0;
    const void* dSubtree = postOperand(in, subtree, &subtreeStates);
    if (!dSubtree) return BEAGLE_ERROR_OUT_OF_RANGE;
    rc = upload(in, dSlots, slots.data(), slots.size() * sizeof(int)); if (rc) return rc;
    HIP_TRY(hipMemsetAsync(dError, 0, sizeof(unsigned), live(in)));
    CallTimer timer(in);
    rc = timer.start(); if (rc) return rc;
    const double* weights = in->weights + (size_t)wIdx * in->C;
    int launches = 0;
    mi355::launchRegraftPendants(live(in), in->matrices, dSlots, (int)slots.size(), dSubtree, subtreeStates != 0, in->P, in->S, in->C, in->tiled,
                                 dPendants);
    launches++;

    std::vector<mi355::PlacementCandidate> rows;
    for (size_t b = 0; b < K && !rc; b += chunk) {
        const size_t m = std::min(chunk, K - b);
        rows.assign(m, mi355::PlacementCandidate{});
        for (size_t e = 0; e < m && !rc; e++) {
            const int* c = cands + ATTACH_FIELDS * (b + e);
            rc = fillAttachment(in, c, pendantOf[c[ATTACH_PENDANT_MATRIX]], (int)e, &rows[e]);
        }
        if (rc) break;
        void* dRows = nullptr;
        rc = uploadTransient(in, rows.data(), m * sizeof(mi355::PlacementCandidate), &dRows); if (rc) break;
        if (!mi355::launchRegraftRatios(live(in), (const mi355::PlacementCandidate*)dRows, (int)m, weights, dPendants, dScale, scaleRaw,
                                        in->patternWeights, in->P, in->S, in->C, in->tiled, dRatios, dError)) { rc = BEAGLE_ERROR_GENERAL; break; }
        mi355::launchRegraftScores(live(in), dRatios, in->patternWeights, (int)m, in->P, dPartial, dScores);
        launches += 3;
        if (hipGetLastError() != hipSuccess) { rc = BEAGLE_ERROR_GENERAL; break; }
        if (b + m >= K) { rc = timer.stop(launches); if (rc) break; }
        // this launch's block of the outputs; the next launch overwrites the scratch, so the copies are waited for
        if (outRatios && hipMemcpyAsync(outRatios + b * P, dRatios, m * P * sizeof(double), hipMemcpyDeviceToHost, live(in)) != hipSuccess) {
            rc = BEAGLE_ERROR_GENERAL; break;
        }
        if (hipMemcpyAsync(outScores + b, dScores, m * sizeof(double), hipMemcpyDeviceToHost, live(in)) != hipSuccess) { rc = BEAGLE_ERROR_GENERAL; break; }
        if (hipStreamSynchronize(live(in)) != hipSuccess) { rc = BEAGLE_ERROR_GENERAL; break; }
    }
    if (rc) return rc;
    unsigned err = 0;
    rc = download(in, &err, dError, sizeof(err)); if (rc) return rc;
    if (err) *fpError = true;
    in->statRegraftCalls++; in->statRegraftCandidates += candidateCount; in->statRegraftMaterialised += unstoredAtEntry;
    in->statRegraftLaunches += launches;
    return BEAGLE_SUCCESS;
}

}  // namespace

extern "C" {

int beagleMi355RegraftScores(int instance, const int* candidates, int candidateCount, int subtreeBuffer, int subtreeCumulativeScaleIndex,
                             int categoryWeightsIndex, int flags, double* outScores, double* outPatternLogRatios) {
    if (!candidates || candidateCount < 1 || flags != 0 || !outScores) return BEAGLE_ERROR_OUT_OF_RANGE;
    if (mi355::isShardedHandle(instance)) return BEAGLE_ERROR_NO_IMPLEMENTATION;
    GET_INSTANCE_KEEP_PENDING(instance);        // (the list is checked before a held-back pre-order list runs: regraftScores)
    bool bad = false;
    const int rc = regraftScores(in, candidates, candidateCount, subtreeBuffer, subtreeCumulativeScaleIndex, categoryWeightsIndex, outScores,
                                 outPatternLogRatios, &bad);
    if (rc) return rc;
    return bad ? BEAGLE_ERROR_FLOATING_POINT : BEAGLE_SUCCESS;
}

int beagleMi355RegraftStats(int instance, long* out4) {
    if (!out4) return BEAGLE_ERROR_OUT_OF_RANGE;
    if (mi355::isShardedHandle(instance)) return BEAGLE_ERROR_NO_IMPLEMENTATION;
    GET_INSTANCE_KEEP_PENDING(instance);
    out4[0] = in->statRegraftCalls; out4[1] = in->statRegraftCandidates; out4[2] = in->statRegraftMaterialised;
    out4[3] = in->statRegraftLaunches;
    return BEAGLE_SUCCESS;
}

}  // extern "C"
