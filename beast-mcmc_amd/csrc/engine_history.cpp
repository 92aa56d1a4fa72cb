// engine_history.cpp — complete substitution histories (include/beagle_mi355.h beagleMi355SimulateCompleteHistories): a forward
// simulation down the tree that keeps what happened on every branch.  What dr.app.beagle.tools.CompleteHistorySimulator.simulate
// computes with one StateHistory.simulateUnconditionalOnEndingState per (branch, site) in Java (CompleteHistorySimulator.java:384-496).
// It reads the instance's category rates, category weights and state frequencies and nothing else.
#include "engine_internal.h"

#include <map>

using namespace mi355::eng;

namespace {

constexpr size_t HIST_SCRATCH_BYTES = 256ull << 20;      // what one chunk of sites may take on the device (the simulator's rule)

// the caller's arguments, as every shard gets them
struct HistoryCall {
    const int* nodes; int nodeCount; int siteCount;
    const double* branchLengths; const double* nodeHeights; const double* Q; int qCount;
    int ratesIndex, wIdx, fIdx;
    const double* registers; int rewardMask; int K;
    unsigned long long seed;
    const unsigned char* inRootStates; const int* inRateCategories;
    unsigned char* outStates; int* outCategories; double* outValues; double* outSiteTotals; int* outEventCounts;
    bool rowTotals, history;
};

// what a first pass leaves behind for the event pass and the merge (start: its first site)
struct HistoryPass : mi355::ShardPart {
    mi355::HistoryArgs args;
    size_t chunk = 0, rootSlot = 0; int site1 = 0;
    long long* dOffsets = nullptr;                       // per chunk c: count_c + 1 offsets at dOffsets + c0 + c
    std::vector<long long> chunkEvents;
};

// What does not depend on the instance: the node list's shape, the generators, lengths, registers, the caller's input states and
// categories; the rows, with their scratch slots as engine_simulate.cpp lays them out.
int checkCall(const HistoryCall& c, int S, int C, std::vector<mi355::HistoryRow>* rows, size_t* slots) {
    if (!c.nodes || !c.branchLengths || !c.Q || !c.registers || c.nodeCount < 1 || c.siteCount < 1 || c.qCount < 1)
        return BEAGLE_ERROR_OUT_OF_RANGE;
    if (S < 2 || S > mi355::HISTORY_MAX_STATES) return BEAGLE_ERROR_NO_IMPLEMENTATION;
    for (int r = 1; r < c.nodeCount; r++)
        if (badIndex(c.nodes[3 * r + 1], c.qCount) || !std::isfinite(c.branchLengths[r]) || c.branchLengths[r] < 0.0)
            return BEAGLE_ERROR_OUT_OF_RANGE;
    int maxOut = -1;
    int rc = checkSiteCall(c.nodes, c.nodeCount, c.siteCount, c.inRootStates, c.inRateCategories, S, C, &maxOut); if (rc) return rc;
    for (size_t e = 0; e < (size_t)c.qCount * S * S; e++)
        if (!std::isfinite(c.Q[e])) return BEAGLE_ERROR_OUT_OF_RANGE;
    rows->assign(c.nodeCount, mi355::HistoryRow{});
    for (int r = 0; r < c.nodeCount; r++) {
        mi355::HistoryRow& row = (*rows)[r];
        row.length = r == 0 ? 0.0 : c.branchLengths[r];
        row.hChild = c.nodeHeights ? c.nodeHeights[r] : 0.0;
        row.hParent = c.nodeHeights && r > 0 ? c.nodeHeights[c.nodes[3 * r + 2]] : 0.0;
        row.q = r == 0 ? -1 : c.nodes[3 * r + 1];
    }
    return assignSlots(c.nodes, c.nodeCount, maxOut, *rows, slots);
}

// Sites site0 .. site1 - 1 of a call over siteCount sites (the sharded handle: this instance's part; otherwise all of them): the
// streams are keyed on the site of the whole call, and everything indexed by site lands at the site's place in the caller's arrays.
int firstPass(Instance* in, const HistoryCall& c, std::vector<mi355::HistoryRow> rows, size_t slots, int site0, int site1,
              HistoryPass* pass) {
    if (badIndex(c.ratesIndex, in->eigenCount) || badIndex(c.wIdx, in->eigenCount) || badIndex(c.fIdx, in->eigenCount))
        return BEAGLE_ERROR_OUT_OF_RANGE;
    if (in->basta) return BEAGLE_ERROR_NO_IMPLEMENTATION;
    const int S = in->S, C = in->C, K = c.K, R = c.nodeCount;
    pass->start = site0; pass->site1 = site1; pass->events = 0;
    pass->rowTotals.assign(c.rowTotals ? (size_t)K * R : 0, 0.0);
    if (site1 <= site0) return 0;
    const size_t sites = (size_t)(site1 - site0), Rn = (size_t)R;
    const size_t perSite = slots + sizeof(int) + (size_t)K * sizeof(double) + (c.outValues ? (size_t)K * Rn * sizeof(double) : 0) +
                           (c.rowTotals ? (size_t)K * Rn * sizeof(double) / mi355::HISTORY_WAVE + 1 : 0) +
                           (c.history ? Rn * sizeof(int) + sizeof(long long) : 0);
    // BEAGLE_MI355_HIST_CHUNK_SITES=<n>: the sites of one launch; otherwise as many as keep what a chunk needs within
    // HIST_SCRATCH_BYTES.  A multiple of HISTORY_TOTAL_BLOCK, so that every chunk starts on a block of the row totals' order.
    const size_t B = mi355::HISTORY_TOTAL_BLOCK;
    const size_t chunk = chunkSites("BEAGLE_MI355_HIST_CHUNK_SITES", B, std::max<size_t>(B, HIST_SCRATCH_BYTES / perSite / B * B), sites);
    const size_t nChunks = (sites + chunk - 1) / chunk;
    const mi355::scratch::HistoryLayout L(slots, chunk, sites, c.qCount, S, K, Rn, mi355::historyLines(c.qCount, S),
                                          mi355::historyTableDoubles(c.qCount, S, C), chunk / mi355::HISTORY_WAVE,
                                          sizeof(mi355::HistoryRow), c.outValues != nullptr, c.rowTotals, c.history);
    int rc = growScratch(in, in->historyDev, L.bytes()); if (rc) return rc;
    char* base = in->historyDev.p;
    uint8_t* dStates = L.states.at(base);
    int* dCats = L.cats.at(base);
    unsigned* dErr = L.error.at(base);
    double *dQ = L.Q.at(base), *dReg = L.reg.at(base), *dTable = L.table.at(base), *dTotal = L.total.at(base), *dRate = L.rate.at(base),
           *dSite = L.site.at(base), *dRow = L.row.at(base), *dWave = L.wave.at(base), *dStage = L.stage.at(base);
    int* dLast = L.last.at(base);
    mi355::HistoryRow* dRows = L.rows.as<mi355::HistoryRow>(base);
    int* dCounts = L.counts.at(base);                    // (dWave, dStage, dCounts, dOffsets: NULL where the call does not ask for them)
    long long* dOffsets = L.offsets.at(base);
    rc = upload(in, dQ, c.Q, L.Q.bytes()); if (rc) return rc;
    rc = upload(in, dReg, c.registers, L.reg.bytes()); if (rc) return rc;
    rc = upload(in, dRows, rows.data(), rows.size() * sizeof(mi355::HistoryRow)); if (rc) return rc;
    HIP_TRY(hipMemsetAsync(dErr, 0, sizeof(unsigned), live(in)));
    mi355::launchHistoryTables(live(in), dQ, c.qCount, in->weights + (size_t)c.wIdx * C, in->freqs + (size_t)c.fIdx * S, S, C, dTable,
                               dTotal, dRate, dLast);
    HIP_TRY(hipGetLastError());

    mi355::HistoryArgs& a = pass->args;
    a = mi355::HistoryArgs{};
    a.rows = dRows; a.table = dTable; a.total = dTotal; a.rate = dRate; a.last = dLast; a.catRates = in->rates + (size_t)c.ratesIndex * C;
    a.registers = dReg; a.states = dStates; a.cats = dCats; a.stage = dStage; a.siteTotals = dSite;
    a.wavePartials = dWave; a.eventCounts = dCounts; a.fpError = dErr;
    a.seed = c.seed; a.siteCount = (unsigned long long)c.siteCount; a.stride = chunk; a.nRows = R; a.K = K; a.S = S; a.C = C;
    a.qCount = c.qCount; a.rewardMask = c.rewardMask; a.haveRoot = c.inRootStates != nullptr; a.haveCats = c.inRateCategories != nullptr;
    pass->chunk = chunk; pass->rootSlot = (size_t)rows[0].slot; pass->dOffsets = dOffsets; pass->chunkEvents.assign(nChunks, 0);

    const std::vector<int> wanted = c.outStates ? wantedRows(c.nodes, R) : std::vector<int>();
    const size_t G = (size_t)c.siteCount;
    for (size_t ci = 0; ci < nChunks; ci++) {
        const size_t c0 = ci * chunk, count = std::min(chunk, sites - c0), first = (size_t)site0 + c0;
        if (c.inRootStates) { rc = upload(in, dStates + (size_t)rows[0].slot * chunk, c.inRootStates + first, count); if (rc) return rc; }
        if (c.inRateCategories) { rc = upload(in, dCats, c.inRateCategories + first, count * sizeof(int)); if (rc) return rc; }
        a.nSites = (int)count; a.siteOffset = (unsigned long long)first;
        mi355::launchHistoryWalk(live(in), a, false);
        HIP_TRY(hipGetLastError());
        rc = copyWantedRows(in, wanted, dStates, chunk, count, c.outStates, G, first); if (rc) return rc;
        if (c.outCategories) HIP_TRY(hipMemcpyAsync(c.outCategories + first, dCats, count * sizeof(int), hipMemcpyDeviceToHost, live(in)));
        if (c.outValues)
            HIP_TRY(hipMemcpy2DAsync(c.outValues + first, G * sizeof(double), dStage, chunk * sizeof(double), count * sizeof(double),
                                     (size_t)K * Rn, hipMemcpyDeviceToHost, live(in)));
        if (c.outSiteTotals)
            HIP_TRY(hipMemcpy2DAsync(c.outSiteTotals + first, G * sizeof(double), dSite, chunk * sizeof(double), count * sizeof(double),
                                     (size_t)K, hipMemcpyDeviceToHost, live(in)));
        if (c.rowTotals) {
            mi355::launchHistoryRowTotals(live(in), dWave, (int)((count + mi355::HISTORY_WAVE - 1) / mi355::HISTORY_WAVE), K, R, ci == 0, dRow);
            HIP_TRY(hipGetLastError());
        }
        if (c.history) {
            if (c.outEventCounts)
                HIP_TRY(hipMemcpy2DAsync(c.outEventCounts + first, G * sizeof(int), dCounts, count * sizeof(int), count * sizeof(int), Rn,
                                         hipMemcpyDeviceToHost, live(in)));
            long long* off = dOffsets + c0 + ci;
            mi355::launchEventOffsets(live(in), dCounts, R, (int)count, off);
            HIP_TRY(hipGetLastError());
            rc = download(in, &pass->chunkEvents[ci], off + count, sizeof(long long)); if (rc) return rc;
            pass->events += pass->chunkEvents[ci];
        } else {
            HIP_TRY(hipStreamSynchronize(live(in)));         // (the next chunk overwrites the scratch rows)
        }
    }
    if (c.rowTotals) { rc = download(in, pass->rowTotals.data(), dRow, L.row.bytes()); if (rc) return rc; }
    unsigned err = 0;
    rc = download(in, &err, dErr, sizeof(unsigned)); if (rc) return rc;
    return err ? BEAGLE_ERROR_FLOATING_POINT : BEAGLE_SUCCESS;
}

// The event list of the last firstPass on `in`: the same histories again, chunk by chunk, written at outHeights / outStates (this
// instance's first event)
int eventPass(Instance* in, const HistoryCall& c, HistoryPass* pass, double* outHeights, unsigned char* outStates) {
    if (pass->events == 0) return 0;
    mi355::HistoryArgs a = pass->args;
    int rc = growEvents(in, (size_t)pass->events, &a.eventStates, &a.eventHeights); if (rc) return rc;
    const size_t sites = (size_t)(pass->site1 - pass->start), chunk = pass->chunk;
    long long base = 0;
    for (size_t ci = 0; ci * chunk < sites; ci++) {
        const size_t c0 = ci * chunk, count = std::min(chunk, sites - c0), first = (size_t)pass->start + c0;
        if (pass->chunkEvents[ci] > 0) {
            if (c.inRootStates) { rc = upload(in, a.states + pass->rootSlot * chunk, c.inRootStates + first, count); if (rc) return rc; }
            if (c.inRateCategories) { rc = upload(in, a.cats, c.inRateCategories + first, count * sizeof(int)); if (rc) return rc; }
            a.nSites = (int)count; a.siteOffset = (unsigned long long)first; a.siteOffsets = pass->dOffsets + c0 + ci; a.eventBase = base;
            mi355::launchHistoryWalk(live(in), a, true);
            HIP_TRY(hipGetLastError());
        }
        base += pass->chunkEvents[ci];
    }
    return copyEvents(in, (size_t)pass->events, a.eventStates, a.eventHeights, outStates, outHeights);
}

}  // namespace

extern "C" {

int beagleMi355SimulateCompleteHistories(int instance, const int* nodes, int nodeCount, int siteCount, const double* branchLengths,
                                         const double* nodeHeights, const double* infinitesimalMatrices, int qCount,
                                         int categoryRatesIndex, int categoryWeightsIndex, int stateFrequenciesIndex,
                                         const double* registers, const int* registerFlags, int registerCount, unsigned long long seed,
                                         int flags, const unsigned char* inRootStates, const int* inRateCategories,
                                         unsigned char* outStates, int* outRateCategories, double* outValues, double* outRowTotals,
                                         double* outSiteTotals, int* outEventCounts, long long eventCapacity, double* outEventHeights,
                                         unsigned char* outEventStates, long long* outEventTotal) {
    if (flags != 0 || registerCount < 1 || registerCount > mi355::MAX_JUMP_REGISTERS) return BEAGLE_ERROR_OUT_OF_RANGE;
    int rewardMask = 0;
    if (!checkRegisterFlags(registerFlags, registerCount, BEAGLE_MI355_JUMPS_REWARDS)) return BEAGLE_ERROR_OUT_OF_RANGE;
    for (int k = 0; registerFlags && k < registerCount; k++)
        if (registerFlags[k] & BEAGLE_MI355_JUMPS_REWARDS) rewardMask |= 1 << k;
    const bool wantEvents = outEventHeights || outEventStates;
    const bool history = outEventCounts || wantEvents || outEventTotal;
    if (!outStates && !outRateCategories && !outValues && !outRowTotals && !outSiteTotals && !history) return BEAGLE_ERROR_OUT_OF_RANGE;
    if (outEventHeights && !nodeHeights) return BEAGLE_ERROR_OUT_OF_RANGE;
    if (wantEvents && eventCapacity < 0) return BEAGLE_ERROR_OUT_OF_RANGE;
    if (outEventTotal) *outEventTotal = 0;
    HistoryCall c{nodes, nodeCount, siteCount, branchLengths, nodeHeights, infinitesimalMatrices, qCount, categoryRatesIndex,
                  categoryWeightsIndex, stateFrequenciesIndex, registers, rewardMask, registerCount, seed, inRootStates, inRateCategories,
                  outStates, outRateCategories, outValues, outSiteTotals, outEventCounts, outRowTotals != nullptr, history};
    // phase 1: shard k of n (a plain handle: the instance) simulates its part of the sites (SiteSplit) into its columns; phase 2: its
    // events after the earlier parts' events.  The row totals are the parts' sums, added in site order.
    SiteSplit split;
    int rc = split.init(instance, siteCount); if (rc) return rc;
    std::vector<mi355::HistoryRow> rows;
    size_t slots = 0;
    rc = checkCall(c, split.S, split.C, &rows, &slots); if (rc) return rc;
    std::mutex mu;
    std::map<int, HistoryPass> passes;                       // shard handle -> its pass
    rc = mi355::shardedOrPlain(instance, [&](int h) -> int {
        int site0 = 0, site1 = 0;
        if (!split.next(&site0, &site1)) return BEAGLE_ERROR_GENERAL;
        GET_INSTANCE(h);
        HistoryPass pass;
        const int r = firstPass(in, c, rows, slots, site0, site1, &pass);
        std::lock_guard<std::mutex> lock(mu);
        passes[h] = std::move(pass);
        return r;
    });
    if (rc != BEAGLE_SUCCESS && rc != BEAGLE_ERROR_FLOATING_POINT) return rc;
    const mi355::ShardParts order = mi355::orderedParts(passes);
    if (outRowTotals) mi355::sumRowTotals(order, (size_t)registerCount * nodeCount, outRowTotals);
    return mi355::placeEvents(instance, order, wantEvents, eventCapacity, outEventTotal, rc, [&](int h, long long first) -> int {
        GET_INSTANCE(h);
        return eventPass(in, c, &passes[h], outEventHeights ? outEventHeights + first : nullptr,
                         outEventStates ? outEventStates + 2 * first : nullptr);
    });
}

}  // extern "C"
