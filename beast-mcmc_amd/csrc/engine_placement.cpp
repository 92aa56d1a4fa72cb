// engine_placement.cpp — scores of attaching new sequences at candidate points of the tree in one call (include/beagle_mi355.h
// beagleMi355PlacementScores, beagleMi355PlacementStats; kernels_placement.hip): argument checks, materialising what the 4-state walk
// left unstored, the pendant tables, then per chunk of candidates the log table and per chunk of queries the counts, the product and
// the copy-out.
#include "engine_internal.h"

#include <map>

using namespace mi355::eng;
namespace scratch = mi355::scratch;

namespace {

constexpr size_t TABLE_SCRATCH_BYTES = 256ull << 20;       // most log-table scratch of one launch
constexpr size_t COUNT_SCRATCH_BYTES = 256ull << 20;       // most count-table and query-code scratch of one launch

int placementScores(Instance* in, const int* cands, int candidateCount, int wIdx, const int* sitePatterns, int siteCount,
                    const unsigned char* queryCodes, int queryCount, const double* codeTable, int codeCount, double* outScores,
                    double* outLogTable, bool* fpError) {
    if (in->partitionCount > 1 || in->basta || in->S > 255) return BEAGLE_ERROR_NO_IMPLEMENTATION;
    if (badIndex(wIdx, in->eigenCount)) return BEAGLE_ERROR_OUT_OF_RANGE;
    for (int i = 0; i < siteCount; i++) if (sitePatterns[i] < -1 || sitePatterns[i] >= in->P) return BEAGLE_ERROR_OUT_OF_RANGE;
    for (size_t i = 0, n = (size_t)queryCount * siteCount; i < n; i++)
        if (queryCodes[i] >= codeCount && queryCodes[i] != 255) return BEAGLE_ERROR_OUT_OF_RANGE;
    long unstoredAtEntry = 0;
    int rc = makeResident(in, [&](ReadSet& reads) -> int {
        for (int k = 0; k < candidateCount; k++) {
            if (int bad = checkAttachment(in, cands + ATTACH_FIELDS * k, reads)) return bad;
        }
        return 0;
    }, &unstoredAtEntry);
    if (rc) return rc;

    const size_t K = (size_t)candidateCount, Q = (size_t)queryCount, P = (size_t)in->P, S = (size_t)in->S, C = (size_t)in->C, X = (size_t)codeCount;
    const size_t sites = (size_t)siteCount, segments = (size_t)mi355::placementSegments(in->P, codeCount);
    if (mi355::placementPatternBlock(in->S, codeCount) == 0) return BEAGLE_ERROR_NO_IMPLEMENTATION;
    // the distinct pendant matrices, in order of first appearance
    std::map<int, int> pendantOf;
    std::vector<int> slots;
    for (size_t k = 0; k < K; k++) {
        const int m = cands[ATTACH_FIELDS * k + ATTACH_PENDANT_MATRIX];
        if (pendantOf.emplace(m, (int)slots.size()).second) slots.push_back(m);
    }
    // candidates per launch: the descriptors fit a quarter of the staging ring, the log table its budget, the grid its second
    // dimension; queries per launch: the counts and the codes fit theirs
    size_t kChunk = std::min<size_t>({K, (RING_BYTES / 4) / sizeof(mi355::PlacementCandidate), (size_t)mi355::PLACEMENT_MAX_CANDIDATES,
                                      std::max<size_t>(1, TABLE_SCRATCH_BYTES / (P * X * sizeof(double)))});
    kChunk = std::min<size_t>(chunkSites("BEAGLE_MI355_PLACEMENT_CHUNK", 1, kChunk, K), (size_t)mi355::PLACEMENT_MAX_CANDIDATES);
    size_t qChunk = std::min<size_t>(Q, std::max<size_t>(1, COUNT_SCRATCH_BYTES / (P * X * sizeof(int) + sites)));
    qChunk = std::min<size_t>(chunkSites("BEAGLE_MI355_PLACEMENT_QUERY_CHUNK", 1, qChunk, Q), 65535 * 64);
    const scratch::PlacementLayout L(kChunk, qChunk, slots.size(), sites, segments, P, S, C, X);
    rc = growScratch(in, in->placementDev, L.bytes()); if (rc) return rc;
    char* base = in->placementDev.p;
    double *dPendant = L.pendant.at(base), *dCodeTable = L.codeTable.at(base), *dTable = L.table.at(base), *dPartial = L.partial.at(base);
    double* dScores = L.scores.at(base);
    int *dCounts = L.counts.at(base), *dSitePatterns = L.sitePatterns.at(base), *dSlots = L.slots.at(base);
    uint8_t* dCodes = L.codes.at(base);
    unsigned* dError = L.error.at(base);
    rc = upload(in, dCodeTable, codeTable, X * S * sizeof(double)); if (rc) return rc;
    rc = upload(in, dSitePatterns, sitePatterns, sites * sizeof(int)); if (rc) return rc;
    rc = upload(in, dSlots, slots.data(), slots.size() * sizeof(int)); if (rc) return rc;
    HIP_TRY(hipMemsetAsync(dError, 0, sizeof(unsigned), live(in)));
    CallTimer timer(in);
    rc = timer.start();
    const double* weights = in->weights + (size_t)wIdx * in->C;
    int launches = 0;
    if (!rc) { mi355::launchPendantTables(live(in), in->matrices, dSlots, (int)slots.size(), dCodeTable, in->S, in->C, codeCount, dPendant); launches++; }

    // the counts of queries q0 .. q0 + n - 1, left in dCounts
    auto countQueries = [&](size_t q0, size_t n) -> int {
        int r = upload(in, dCodes, queryCodes + q0 * sites, n * sites); if (r) return r;
        HIP_TRY(hipMemsetAsync(dCounts, 0, n * P * X * sizeof(int), live(in)));
        mi355::launchPlacementCounts(live(in), dSitePatterns, dCodes, (int)n, siteCount, in->P, codeCount, dCounts);
        launches++;
        return 0;
    };
    const bool countOnce = qChunk >= Q;
    if (!rc && countOnce) rc = countQueries(0, Q);

    std::vector<mi355::PlacementCandidate> rows;
    for (size_t b = 0; b < K && !rc; b += kChunk) {
        const size_t m = std::min(kChunk, K - b);
        rows.assign(m, mi355::PlacementCandidate{});
        for (size_t e = 0; e < m; e++) {
            const int* c = cands + ATTACH_FIELDS * (b + e);
            rc = fillAttachment(in, c, pendantOf[c[ATTACH_PENDANT_MATRIX]], (int)e, &rows[e]);
            if (rc) break;
        }
        if (rc) break;
        void* dRows = nullptr;
        rc = uploadTransient(in, rows.data(), m * sizeof(mi355::PlacementCandidate), &dRows); if (rc) break;
        if (!mi355::launchPlacementTable(live(in), (const mi355::PlacementCandidate*)dRows, (int)m, weights, dPendant, in->P, in->S, in->C,
                                         codeCount, in->tiled, dTable, dError)) { rc = BEAGLE_ERROR_GENERAL; break; }
        launches++;
        if (outLogTable && hipMemcpyAsync(outLogTable + b * P * X, dTable, m * P * X * sizeof(double), hipMemcpyDeviceToHost, live(in)) != hipSuccess) {
            rc = BEAGLE_ERROR_GENERAL; break;
        }
        for (size_t q0 = 0; q0 < Q && !rc; q0 += qChunk) {
            const size_t n = std::min(qChunk, Q - q0);
            if (!countOnce) { rc = countQueries(q0, n); if (rc) break; }
            mi355::launchPlacementScores(live(in), dCounts, dTable, (int)n, (int)m, in->P, codeCount, dPartial, dScores);
            launches += 2;
            if (hipGetLastError() != hipSuccess) { rc = BEAGLE_ERROR_GENERAL; break; }
            if (b + m >= K && q0 + n >= Q) { rc = timer.stop(launches); if (rc) break; }
            // this launch's block of the scores; the next launch overwrites the scratch, so the copy is waited for
            if (hipMemcpy2DAsync(outScores + q0 * K + b, K * sizeof(double), dScores, m * sizeof(double), m * sizeof(double), n,
                                 hipMemcpyDeviceToHost, live(in)) != hipSuccess) { rc = BEAGLE_ERROR_GENERAL; break; }
            if (hipStreamSynchronize(live(in)) != hipSuccess) { rc = BEAGLE_ERROR_GENERAL; break; }
        }
    }
    if (rc) return rc;
    unsigned err = 0;
    rc = download(in, &err, dError, sizeof(err)); if (rc) return rc;
    if (err) *fpError = true;
    in->statPlacementCalls++; in->statPlacementCandidates += candidateCount; in->statPlacementMaterialised += unstoredAtEntry;
    in->statPlacementLaunches += launches;
    return BEAGLE_SUCCESS;
}

}  // namespace

extern "C" {

int beagleMi355PlacementScores(int instance, const int* candidates, int candidateCount, int categoryWeightsIndex, const int* sitePatterns,
                               int siteCount, const unsigned char* queryCodes, int queryCount, const double* codeTable, int codeCount,
                               int flags, double* outScores, double* outLogTable) {
    if (!candidates || candidateCount < 1 || !sitePatterns || siteCount < 1 || !queryCodes || queryCount < 1 || !codeTable || codeCount < 1 ||
        codeCount > 255 || flags != 0 || !outScores) return BEAGLE_ERROR_OUT_OF_RANGE;
    if (mi355::isShardedHandle(instance)) return BEAGLE_ERROR_NO_IMPLEMENTATION;
    GET_INSTANCE_KEEP_PENDING(instance);        // (the list is checked before a held-back pre-order list runs: placementScores)
    bool bad = false;
    const int rc = placementScores(in, candidates, candidateCount, categoryWeightsIndex, sitePatterns, siteCount, queryCodes, queryCount,
                                   codeTable, codeCount, outScores, outLogTable, &bad);
    if (rc) return rc;
    return bad ? BEAGLE_ERROR_FLOATING_POINT : BEAGLE_SUCCESS;
}

int beagleMi355PlacementStats(int instance, long* out4) {
    if (!out4) return BEAGLE_ERROR_OUT_OF_RANGE;
    if (mi355::isShardedHandle(instance)) return BEAGLE_ERROR_NO_IMPLEMENTATION;
    GET_INSTANCE_KEEP_PENDING(instance);
    out4[0] = in->statPlacementCalls; out4[1] = in->statPlacementCandidates; out4[2] = in->statPlacementMaterialised;
    out4[3] = in->statPlacementLaunches;
    return BEAGLE_SUCCESS;
}

}  // extern "C"
