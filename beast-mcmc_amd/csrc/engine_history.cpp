// engine_history.cpp — complete substitution histories (include/beagle_mi355.h beagleMi355SimulateCompleteHistories): a forward
// simulation down the tree that keeps what happened on every branch.  What dr.app.beagle.tools.CompleteHistorySimulator.simulate
// computes with one StateHistory.simulateUnconditionalOnEndingState per (branch, site) in Java (CompleteHistorySimulator.java:384-496).
// It reads the instance's category rates, category weights and state frequencies and nothing else.
#include "engine_internal.h"

#include <climits>
#include <map>

using namespace mi355::eng;

namespace {

constexpr size_t HIST_SCRATCH_BYTES = 256ull << 20;      // what one chunk of sites may take on the device (the simulator's rule)

size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }

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

// what a first pass leaves behind for the event pass
struct HistoryPass {
    mi355::HistoryArgs args;
    size_t chunk = 0, rootSlot = 0; int site0 = 0, site1 = 0;
    long long* dOffsets = nullptr;                       // per chunk c: count_c + 1 offsets at dOffsets + c0 + c
    std::vector<long long> chunkEvents;
    long long events = 0;
    std::vector<double> rowTotals;
};

// What does not depend on the instance: the node list's shape, the generators, lengths, registers, the caller's input states and
// categories.  *slots: scratch rows, as engine_simulate.cpp lays them out (a node with an outRow keeps its states in scratch row outRow).
int checkCall(const HistoryCall& c, int S, int C, std::vector<mi355::HistoryRow>* rows, size_t* slots) {
    if (!c.nodes || !c.branchLengths || !c.Q || !c.registers || c.nodeCount < 1 || c.siteCount < 1 || c.qCount < 1)
        return BEAGLE_ERROR_OUT_OF_RANGE;
    if (S < 2 || S > mi355::HISTORY_MAX_STATES) return BEAGLE_ERROR_NO_IMPLEMENTATION;
    std::vector<int> used;
    int maxOut = -1;
    for (int r = 0; r < c.nodeCount; r++) {
        const int out = c.nodes[3 * r], q = c.nodes[3 * r + 1], parent = c.nodes[3 * r + 2];
        if (out < -1) return BEAGLE_ERROR_OUT_OF_RANGE;
        if (r > 0 && (parent < 0 || parent >= r || badIndex(q, c.qCount))) return BEAGLE_ERROR_OUT_OF_RANGE;
        if (r > 0 && (!std::isfinite(c.branchLengths[r]) || c.branchLengths[r] < 0.0)) return BEAGLE_ERROR_OUT_OF_RANGE;
        if (out >= 0) { used.push_back(out); maxOut = std::max(maxOut, out); }
    }
    std::sort(used.begin(), used.end());
    if (std::adjacent_find(used.begin(), used.end()) != used.end()) return BEAGLE_ERROR_OUT_OF_RANGE;
    for (size_t e = 0; e < (size_t)c.qCount * S * S; e++)
        if (!std::isfinite(c.Q[e])) return BEAGLE_ERROR_OUT_OF_RANGE;
    if (c.inRootStates)
        for (int s = 0; s < c.siteCount; s++)
            if (c.inRootStates[s] >= S) return BEAGLE_ERROR_OUT_OF_RANGE;
    if (c.inRateCategories)
        for (int s = 0; s < c.siteCount; s++)
            if (c.inRateCategories[s] < 0 || c.inRateCategories[s] >= C) return BEAGLE_ERROR_OUT_OF_RANGE;
    rows->assign(c.nodeCount, mi355::HistoryRow{});
    size_t next = (size_t)maxOut + 1;
    for (int r = 0; r < c.nodeCount; r++) {
        const int out = c.nodes[3 * r], parent = c.nodes[3 * r + 2];
        const size_t slot = out >= 0 ? (size_t)out : next++;
        if (slot > (size_t)INT_MAX) return BEAGLE_ERROR_OUT_OF_RANGE;
        mi355::HistoryRow& row = (*rows)[r];
        row.length = r == 0 ? 0.0 : c.branchLengths[r];
        row.hChild = c.nodeHeights ? c.nodeHeights[r] : 0.0;
        row.hParent = c.nodeHeights && r > 0 ? c.nodeHeights[parent] : 0.0;
        row.q = r == 0 ? -1 : c.nodes[3 * r + 1];
        row.slot = (int)slot;
        row.parentSlot = r == 0 ? -1 : (*rows)[parent].slot;
        row.parentIsPrev = r > 0 && parent == r - 1;
    }
    *slots = next;
    return 0;
}

// BEAGLE_MI355_HIST_CHUNK_SITES=<n>: the sites of one launch (tests: chunk independence at a small size); otherwise as many as keep
// what a chunk needs within HIST_SCRATCH_BYTES.  A multiple of HISTORY_TOTAL_BLOCK, so that every chunk starts on a block of the row
// totals' order.
size_t chunkSites(size_t bytesPerSite, size_t sites) {
    const size_t B = mi355::HISTORY_TOTAL_BLOCK;
    size_t chunk = std::max<size_t>(B, HIST_SCRATCH_BYTES / bytesPerSite / B * B);
    if (const char* e = getenv("BEAGLE_MI355_HIST_CHUNK_SITES")) {
        const long v = atol(e);
        if (v > 0) chunk = ((size_t)v + B - 1) / B * B;
    }
    return std::min(chunk, (sites + B - 1) / B * B);
}

// Sites site0 .. site1 - 1 of a call over siteCount sites (the sharded handle: this instance's part; otherwise all of them): the
// streams are keyed on the site of the whole call, and everything indexed by site lands at the site's place in the caller's arrays.
int firstPass(Instance* in, const HistoryCall& c, std::vector<mi355::HistoryRow> rows, size_t slots, int site0, int site1,
              HistoryPass* pass) {
    if (badIndex(c.ratesIndex, in->eigenCount) || badIndex(c.wIdx, in->eigenCount) || badIndex(c.fIdx, in->eigenCount))
        return BEAGLE_ERROR_OUT_OF_RANGE;
    if (in->basta) return BEAGLE_ERROR_NO_IMPLEMENTATION;
    const int S = in->S, C = in->C, K = c.K, R = c.nodeCount;
    pass->site0 = site0; pass->site1 = site1; pass->events = 0;
    pass->rowTotals.assign(c.rowTotals ? (size_t)K * R : 0, 0.0);
    if (site1 <= site0) return 0;
    const size_t SS = (size_t)S * S, sites = (size_t)(site1 - site0), Rn = (size_t)R;
    const size_t perSite = slots + sizeof(int) + (size_t)K * sizeof(double) + (c.outValues ? (size_t)K * Rn * sizeof(double) : 0) +
                           (c.rowTotals ? (size_t)K * Rn * sizeof(double) / mi355::HISTORY_WAVE + 1 : 0) +
                           (c.history ? Rn * sizeof(int) + sizeof(long long) : 0);
    const size_t chunk = chunkSites(perSite, sites), nChunks = (sites + chunk - 1) / chunk, waves = chunk / mi355::HISTORY_WAVE;
    const size_t lines = mi355::historyLines(c.qCount, S);
    // historyDev: states [slots][chunk] | categories int [chunk] | error word | Q [qCount][S][S] | registers [K][S][S] | tables | line
    //             totals | line rates | site totals [K][chunk] | row totals [K][R] | wave sums [waves][K][R] | values [K][R][chunk]
    //             (doubles) | line last indices (ints) | rows [R] | event counts int [R][chunk] | site offsets long long [sites + chunks]
    const size_t oCats = up256(slots * chunk), oErr = oCats + chunk * sizeof(int), oQ = up256(oErr + sizeof(unsigned));
    const size_t nQ = (size_t)c.qCount * SS, nReg = (size_t)K * SS, nTable = mi355::historyTableDoubles(c.qCount, S, C),
                 nSite = (size_t)K * chunk, nRow = (size_t)K * Rn, nWave = c.rowTotals ? waves * K * Rn : 0,
                 nStage = c.outValues ? (size_t)K * Rn * chunk : 0;
    const size_t oLast = oQ + (nQ + nReg + nTable + 2 * lines + nSite + nRow + nWave + nStage) * sizeof(double);
    const size_t oRows = up256(oLast + lines * sizeof(int));
    const size_t oCounts = up256(oRows + Rn * sizeof(mi355::HistoryRow));
    const size_t oOffsets = up256(oCounts + (c.history ? Rn * chunk * sizeof(int) : 0));
    const size_t bytes = oOffsets + (c.history ? (sites + nChunks) * sizeof(long long) : 0);
    int rc = growDevice(in, in->historyDev, bytes, bytes, Grow::SyncIfHeld); if (rc) return rc;
    char* base = in->historyDev.p;
    uint8_t* dStates = (uint8_t*)base;
    int* dCats = (int*)(base + oCats);
    unsigned* dErr = (unsigned*)(base + oErr);
    double* dQ = (double*)(base + oQ);
    double* dReg = dQ + nQ;
    double* dTable = dReg + nReg;
    double* dTotal = dTable + nTable;
    double* dRate = dTotal + lines;
    double* dSite = dRate + lines;
    double* dRow = dSite + nSite;
    double* dWave = dRow + nRow;
    double* dStage = dWave + nWave;
    int* dLast = (int*)(base + oLast);
    mi355::HistoryRow* dRows = (mi355::HistoryRow*)(base + oRows);
    int* dCounts = c.history ? (int*)(base + oCounts) : nullptr;
    long long* dOffsets = c.history ? (long long*)(base + oOffsets) : nullptr;
    rc = upload(in, dQ, c.Q, nQ * sizeof(double)); if (rc) return rc;
    rc = upload(in, dReg, c.registers, nReg * sizeof(double)); if (rc) return rc;
    rc = upload(in, dRows, rows.data(), rows.size() * sizeof(mi355::HistoryRow)); if (rc) return rc;
    HIP_TRY(hipMemsetAsync(dErr, 0, sizeof(unsigned), live(in)));
    mi355::launchHistoryTables(live(in), dQ, c.qCount, in->weights + (size_t)c.wIdx * C, in->freqs + (size_t)c.fIdx * S, S, C, dTable,
                               dTotal, dRate, dLast);
    HIP_TRY(hipGetLastError());

    mi355::HistoryArgs& a = pass->args;
    a = mi355::HistoryArgs{};
    a.rows = dRows; a.table = dTable; a.total = dTotal; a.rate = dRate; a.last = dLast; a.catRates = in->rates + (size_t)c.ratesIndex * C;
    a.registers = dReg; a.states = dStates; a.cats = dCats; a.stage = c.outValues ? dStage : nullptr; a.siteTotals = dSite;
    a.wavePartials = c.rowTotals ? dWave : nullptr; a.eventCounts = dCounts; a.fpError = dErr;
    a.seed = c.seed; a.siteCount = (unsigned long long)c.siteCount; a.stride = chunk; a.nRows = R; a.K = K; a.S = S; a.C = C;
    a.qCount = c.qCount; a.rewardMask = c.rewardMask; a.haveRoot = c.inRootStates != nullptr; a.haveCats = c.inRateCategories != nullptr;
    pass->chunk = chunk; pass->rootSlot = (size_t)rows[0].slot; pass->dOffsets = dOffsets; pass->chunkEvents.assign(nChunks, 0);

    // the rows to copy out, as runs of consecutive outRows (= consecutive scratch rows): one strided copy each
    std::vector<int> wanted;
    if (c.outStates)
        for (int r = 0; r < R; r++) if (c.nodes[3 * r] >= 0) wanted.push_back(c.nodes[3 * r]);
    std::sort(wanted.begin(), wanted.end());
    const size_t G = (size_t)c.siteCount;
    for (size_t ci = 0; ci < nChunks; ci++) {
        const size_t c0 = ci * chunk, count = std::min(chunk, sites - c0), first = (size_t)site0 + c0;
        if (c.inRootStates) { rc = upload(in, dStates + (size_t)rows[0].slot * chunk, c.inRootStates + first, count); if (rc) return rc; }
        if (c.inRateCategories) { rc = upload(in, dCats, c.inRateCategories + first, count * sizeof(int)); if (rc) return rc; }
        a.nSites = (int)count; a.siteOffset = (unsigned long long)first;
        mi355::launchHistoryWalk(live(in), a, false);
        HIP_TRY(hipGetLastError());
        for (size_t w = 0; w < wanted.size();) {
            size_t b = w + 1;
            while (b < wanted.size() && wanted[b] == wanted[b - 1] + 1) b++;
            HIP_TRY(hipMemcpy2DAsync(c.outStates + (size_t)wanted[w] * G + first, G, dStates + (size_t)wanted[w] * chunk, chunk, count,
                                     b - w, hipMemcpyDeviceToHost, live(in)));
            w = b;
        }
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
    if (c.rowTotals) { rc = download(in, pass->rowTotals.data(), dRow, nRow * sizeof(double)); if (rc) return rc; }
    unsigned err = 0;
    rc = download(in, &err, dErr, sizeof(unsigned)); if (rc) return rc;
    return err ? BEAGLE_ERROR_FLOATING_POINT : BEAGLE_SUCCESS;
}

// The event list of the last firstPass on `in`: the same histories again, chunk by chunk, written at outHeights / outStates (this
// instance's first event)
int eventPass(Instance* in, const HistoryCall& c, HistoryPass* pass, double* outHeights, unsigned char* outStates) {
    if (pass->events == 0) return 0;
    const size_t n = (size_t)pass->events, stBytes = up256(2 * n);
    int rc = growDevice(in, in->eventDev, stBytes + n * sizeof(double), stBytes + n * sizeof(double), Grow::SyncIfHeld); if (rc) return rc;
    mi355::HistoryArgs a = pass->args;
    a.eventStates = in->eventDev.as<uint8_t>();
    a.eventHeights = (double*)(in->eventDev.p + stBytes);
    const size_t sites = (size_t)(pass->site1 - pass->site0), chunk = pass->chunk;
    long long base = 0;
    for (size_t ci = 0; ci * chunk < sites; ci++) {
        const size_t c0 = ci * chunk, count = std::min(chunk, sites - c0), first = (size_t)pass->site0 + c0;
        if (pass->chunkEvents[ci] > 0) {
            if (c.inRootStates) { rc = upload(in, a.states + pass->rootSlot * chunk, c.inRootStates + first, count); if (rc) return rc; }
            if (c.inRateCategories) { rc = upload(in, a.cats, c.inRateCategories + first, count * sizeof(int)); if (rc) return rc; }
            a.nSites = (int)count; a.siteOffset = (unsigned long long)first; a.siteOffsets = pass->dOffsets + c0 + ci; a.eventBase = base;
            mi355::launchHistoryWalk(live(in), a, true);
            HIP_TRY(hipGetLastError());
        }
        base += pass->chunkEvents[ci];
    }
    if (outHeights) HIP_TRY(hipMemcpyAsync(outHeights, a.eventHeights, n * sizeof(double), hipMemcpyDeviceToHost, live(in)));
    if (outStates) HIP_TRY(hipMemcpyAsync(outStates, a.eventStates, 2 * n, hipMemcpyDeviceToHost, live(in)));
    HIP_TRY(hipStreamSynchronize(live(in)));
    return 0;
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
    if (registerFlags)
        for (int k = 0; k < registerCount; k++) {
            if (registerFlags[k] & ~BEAGLE_MI355_JUMPS_REWARDS) return BEAGLE_ERROR_OUT_OF_RANGE;
            if (registerFlags[k] & BEAGLE_MI355_JUMPS_REWARDS) rewardMask |= 1 << k;
        }
    const bool wantEvents = outEventHeights || outEventStates;
    const bool history = outEventCounts || wantEvents || outEventTotal;
    if (!outStates && !outRateCategories && !outValues && !outRowTotals && !outSiteTotals && !history) return BEAGLE_ERROR_OUT_OF_RANGE;
    if (outEventHeights && !nodeHeights) return BEAGLE_ERROR_OUT_OF_RANGE;
    if (wantEvents && eventCapacity < 0) return BEAGLE_ERROR_OUT_OF_RANGE;
    if (outEventTotal) *outEventTotal = 0;
    HistoryCall c{nodes, nodeCount, siteCount, branchLengths, nodeHeights, infinitesimalMatrices, qCount, categoryRatesIndex,
                  categoryWeightsIndex, stateFrequenciesIndex, registers, rewardMask, registerCount, seed, inRootStates, inRateCategories,
                  outStates, outRateCategories, outValues, outSiteTotals, outEventCounts, outRowTotals != nullptr, history};
    std::vector<mi355::HistoryRow> rows;
    size_t slots = 0;
    const size_t nRow = (size_t)registerCount * (nodeCount > 0 ? nodeCount : 0);
    if (mi355::isShardedHandle(instance)) {
        // phase 1: shard k of n simulates sites [siteCount k / n, siteCount (k + 1) / n) into its columns (which shard takes which part
        // does not matter: the streams are keyed on the site); phase 2: its events after the earlier parts' events
        const int shards = mi355::shardedShardCount(instance);
        if (shards < 1) return BEAGLE_ERROR_UNINITIALIZED_INSTANCE;
        int rc = checkCall(c, mi355::shardedStates(instance), mi355::shardedCategories(instance), &rows, &slots);
        if (rc) return rc;
        std::atomic<int> arrivals{0};
        std::mutex mu;
        std::map<int, HistoryPass> passes;                   // shard handle -> its pass
        rc = mi355::shardedBroadcast(instance, [&](int h) -> int {
            const int k = arrivals.fetch_add(1);
            if (k >= shards) return BEAGLE_ERROR_GENERAL;
            const int site0 = (int)((long long)siteCount * k / shards), site1 = (int)((long long)siteCount * (k + 1) / shards);
            GET_INSTANCE(h);
            HistoryPass pass;
            const int r = firstPass(in, c, rows, slots, site0, site1, &pass);
            std::lock_guard<std::mutex> lock(mu);
            passes[h] = std::move(pass);
            return r;
        });
        if (rc != BEAGLE_SUCCESS && rc != BEAGLE_ERROR_FLOATING_POINT) return rc;
        std::vector<std::pair<int, int>> order;              // (site0, handle) in site order
        for (auto& e : passes) order.emplace_back(e.second.site0, e.first);
        std::sort(order.begin(), order.end());
        if (outRowTotals)
            for (size_t i = 0; i < nRow; i++) {
                double s = passes[order[0].second].rowTotals[i];
                for (size_t q = 1; q < order.size(); q++) s = s + passes[order[q].second].rowTotals[i];
                outRowTotals[i] = s;
            }
        long long total = 0;
        std::map<int, long long> first;
        for (auto& o : order) {
            first[o.second] = total;
            total += passes[o.second].events;
        }
        if (outEventTotal) *outEventTotal = total;
        if (!wantEvents) return rc;
        if (total > eventCapacity) return BEAGLE_ERROR_OUT_OF_RANGE;
        const int rcEvents = mi355::shardedBroadcast(instance, [&](int h) -> int {
            GET_INSTANCE(h);
            const long long f = first[h];
            return eventPass(in, c, &passes[h], outEventHeights ? outEventHeights + f : nullptr,
                             outEventStates ? outEventStates + 2 * f : nullptr);
        });
        return rcEvents ? rcEvents : rc;
    }
    GET_INSTANCE(instance);
    int rc = checkCall(c, in->S, in->C, &rows, &slots);
    if (rc) return rc;
    HistoryPass pass;
    rc = firstPass(in, c, std::move(rows), slots, 0, siteCount, &pass);
    if (rc != BEAGLE_SUCCESS && rc != BEAGLE_ERROR_FLOATING_POINT) return rc;
    if (outRowTotals) std::copy(pass.rowTotals.begin(), pass.rowTotals.end(), outRowTotals);
    if (outEventTotal) *outEventTotal = pass.events;
    if (!wantEvents) return rc;
    if (pass.events > eventCapacity) return BEAGLE_ERROR_OUT_OF_RANGE;
    const int rcEvents = eventPass(in, c, &pass, outEventHeights, outEventStates);
    return rcEvents ? rcEvents : rc;
}

}  // extern "C"
