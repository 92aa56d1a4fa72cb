// engine_sampling.cpp — the device samplers: ancestral-state draws, Markov-jump counts and rewards, uniformized histories; each one
// call over a list of nodes, with its scratch layout.
#include "engine_internal.h"

#include <cfloat>
#include <map>

using namespace mi355::eng;

// Grow-only device scratch of an instance (ancestral draws, Markov jumps): exactly `need` bytes when it grows, counted in deviceBytes.
static int growScratch(Instance* in, DevBuf& b, size_t need) { return growDevice(in, b, need, need, Grow::SyncIfHeld); }

// The draw itself, left on the device (AncestralDraw, engine_internal.h): validation, materialising virtual buffers, ONE launch
// (kernels_ancestral.hip).
int mi355::eng::drawAncestral(Instance* in, const int* nodes, int nodeCount, int wIdx, int fIdx, unsigned long long seed, int flags,
                              int globalP, int pOffset, AncestralDraw* d) {
    if (in->partitionCount > 1) return BEAGLE_ERROR_NO_IMPLEMENTATION;
    if (badIndex(wIdx, in->eigenCount) || badIndex(fIdx, in->eigenCount)) return BEAGLE_ERROR_OUT_OF_RANGE;
    std::vector<int> need;
    for (int r = 0; r < nodeCount; r++) {
        const int b = nodes[3 * r], m = nodes[3 * r + 1], parent = nodes[3 * r + 2];
        if (badIndex(b, in->partialsCount)) return BEAGLE_ERROR_OUT_OF_RANGE;
        if (r == 0 && isCompactTip(in, b)) return BEAGLE_ERROR_OUT_OF_RANGE;
        if (r > 0 && (badIndex(m, in->matrixCount) || parent < 0 || parent >= r)) return BEAGLE_ERROR_OUT_OF_RANGE;
        if (isVirt(in, b)) in->planner.keysOf(b, need);
    }
    if (!need.empty()) { int rc = materializeList(in, need); if (rc) return rc; }
    const size_t n = (size_t)in->C * in->S * in->S;
    std::vector<mi355::AncestralRow> rows(nodeCount);
    for (int r = 0; r < nodeCount; r++) {
        const int b = nodes[3 * r];
        mi355::AncestralRow& row = rows[r];
        row.partials = nullptr; row.states = nullptr; row.pad = 0;
        if (isCompactTip(in, b)) row.states = in->tipStates[b];
        else if (in->partials[b]) row.partials = in->partials[b];
        else return BEAGLE_ERROR_OUT_OF_RANGE;                 // a buffer nothing was ever written to
        row.matrix = r == 0 ? nullptr : in->matrices + n * nodes[3 * r + 1];
        row.parent = r == 0 ? -1 : nodes[3 * r + 2];
    }
    const size_t stateBytes = ((size_t)nodeCount * in->P + 255) & ~(size_t)255;
    const size_t tailBytes = (size_t)in->P * sizeof(int) + sizeof(unsigned);
    int rc = growScratch(in, in->ancestralDev, stateBytes + tailBytes); if (rc) return rc;
    d->states = in->ancestralDev.as<uint8_t>();
    d->cats = (int*)(in->ancestralDev.p + stateBytes);
    d->error = (unsigned*)(d->cats + in->P);
    void* dRows = nullptr;
    rc = uploadTransient(in, rows.data(), rows.size() * sizeof(mi355::AncestralRow), &dRows); if (rc) return rc;
    HIP_TRY(hipMemsetAsync(d->error, 0, sizeof(unsigned), live(in)));
    mi355::launchSampleAncestral(live(in), (const mi355::AncestralRow*)dRows, nodeCount, in->weights + (size_t)wIdx * in->C,
                                 in->freqs + (size_t)fIdx * in->S, in->P, in->S, in->C, in->tiled, globalP, pOffset, seed,
                                 (flags & BEAGLE_MI355_ANCESTRAL_MAP) != 0, d->states, d->cats, d->error);
    HIP_TRY(hipGetLastError());
    return 0;
}

// Copy-out of a draw: the states (queued; NULL: none), then the categories and the error word in one synchronising copy.
int mi355::eng::copyAncestral(Instance* in, const AncestralDraw& d, int nodeCount, int globalP, int pOffset, unsigned char* outStates,
                              int* outCategories, unsigned* error) {
    if (outStates) {
        if (globalP == in->P)
            HIP_TRY(hipMemcpyAsync(outStates, d.states, (size_t)nodeCount * in->P, hipMemcpyDeviceToHost, live(in)));
        else
            HIP_TRY(hipMemcpy2DAsync(outStates + pOffset, (size_t)globalP, d.states, (size_t)in->P, (size_t)in->P, (size_t)nodeCount,
                                     hipMemcpyDeviceToHost, live(in)));
    }
    std::vector<int> tail(in->P + 1);
    int rc = download(in, tail.data(), d.cats, (size_t)in->P * sizeof(int) + sizeof(unsigned)); if (rc) return rc;
    if (outCategories) memcpy(outCategories + pOffset, tail.data(), (size_t)in->P * sizeof(int));
    memcpy(error, &tail[in->P], sizeof(unsigned));
    return 0;
}

// One draw of every listed node's state per pattern (include/beagle_mi355.h beagleMi355SampleAncestralStates; what
// AncestralStateBeagleTreeLikelihood.traverseSample computes from a getPartials per internal node and a getTransitionMatrix per
// branch, AncestralStateBeagleTreeLikelihood.java:414-625).  Virtual buffers are materialised by one walk, as for a read-back; the
// draw itself is ONE launch (kernels_ancestral.hip), then the states and categories come back in two copies.  The instance's
// patterns are patterns pOffset .. pOffset + P - 1 of an alignment of globalP (the sharded handle): the random numbers are keyed
// on the global pattern, and row r's states land at outStates + r * globalP + pOffset.
static int sampleAncestral(Instance* in, const int* nodes, int nodeCount, int wIdx, int fIdx, unsigned long long seed, int flags,
                           int globalP, int pOffset, unsigned char* outStates, int* outCategories) {
    AncestralDraw d;
    int rc = drawAncestral(in, nodes, nodeCount, wIdx, fIdx, seed, flags, globalP, pOffset, &d); if (rc) return rc;
    unsigned err = 0;
    rc = copyAncestral(in, d, nodeCount, globalP, pOffset, outStates, outCategories, &err); if (rc) return rc;
    return err ? BEAGLE_ERROR_FLOATING_POINT : BEAGLE_SUCCESS;
}

extern "C" {

int beagleMi355SampleAncestralStates(int instance, const int* nodes, int nodeCount, int categoryWeightsIndex, int stateFrequenciesIndex,
                                     unsigned long long seed, int flags, unsigned char* outStates, int* outRateCategories) {
    if (!nodes || nodeCount < 1 || !outStates) return BEAGLE_ERROR_OUT_OF_RANGE;
    if (mi355::isShardedHandle(instance)) {
        // every shard draws its own pattern range into its columns of the caller's arrays
        const int globalP = mi355::shardedPatternCount(instance);
        return mi355::shardedBroadcast(instance, [&](int h) {
            int pStart = 0, pEnd = 0;
            mi355::shardedBoundsOfHandle(instance, h, &pStart, &pEnd);
            GET_INSTANCE(h);
            DEMOTE_FOLDED_TIPS(in);
            return sampleAncestral(in, nodes, nodeCount, categoryWeightsIndex, stateFrequenciesIndex, seed, flags, globalP, pStart,
                                   outStates, outRateCategories);
        });
    }
    GET_INSTANCE(instance);
    DEMOTE_FOLDED_TIPS(in);                     // (the samplers read tips' partials as data: engine_tipemission.cpp)
    return sampleAncestral(in, nodes, nodeCount, categoryWeightsIndex, stateFrequenciesIndex, seed, flags, in->P, 0, outStates,
                           outRateCategories);
}

}  // extern "C"

// Expected Markov-jump counts and rewards per branch and pattern (include/beagle_mi355.h beagleMi355SampleMarkovJumps; what
// MarkovJumpsBeagleTreeLikelihood.hookCalculation computes inside traverseSample, MarkovJumpsBeagleTreeLikelihood.java:429-567).
// The draw is drawAncestral's, left on the device; then four launches (kernels_markovjumps.hip): the registers' M_k, the
// conditional tables of every (register, row, category), the per-pattern gather (in row chunks of at most 256 MiB of outJumps when
// it is asked for), the per-row totals.  As for the draw, the instance's patterns are pOffset .. pOffset + P - 1 of globalP;
// outRowTotals gets THIS instance's sums ([K][nodeCount]).
static int sampleJumps(Instance* in, const int* nodes, int nodeCount, const double* branchTimes, const double* branchRates,
                       int eigenIndex, int ratesIndex, int wIdx, int fIdx, const double* registers, const int* registerFlags, int K,
                       unsigned long long seed, int flags, int globalP, int pOffset, unsigned char* outStates, int* outCategories,
                       double* outJumps, double* outPatternTotals, double* outRowTotals) {
    if (in->partitionCount > 1 || in->eigenComplex) return BEAGLE_ERROR_NO_IMPLEMENTATION;
    if (badIndex(eigenIndex, in->eigenCount) || badIndex(ratesIndex, in->eigenCount)) return BEAGLE_ERROR_OUT_OF_RANGE;
    AncestralDraw d;
    int rc = drawAncestral(in, nodes, nodeCount, wIdx, fIdx, seed, flags, globalP, pOffset, &d); if (rc) return rc;
    const int S = in->S, C = in->C, P = in->P;
    const size_t SS = (size_t)S * S, R = (size_t)nodeCount, blocks = (size_t)mi355::jumpSiteBlocks(P);
    const size_t stageRows = outJumps ? std::max<size_t>(1, std::min<size_t>(R, (256ull << 20) / ((size_t)K * P * sizeof(double)))) : 0;
    // jumpDev (doubles): registers [K][S][S] | rateReg, tmp, M [3][K][S][S] | cond [K][R][C][S][S] | blockPartials [blocks][K][R]
    //                    | rowTotals [K][R] | patternTotals [K][P] | outJumps stage [K][stageRows][P] | register flags int [K]
    const size_t nReg = (size_t)K * SS, nCond = (size_t)K * R * C * SS, nPart = blocks * K * R, nRow = (size_t)K * R,
                 nPat = (size_t)K * P, nStage = (size_t)K * stageRows * P;
    const size_t doubles = 4 * nReg + nCond + nPart + nRow + nPat + nStage;
    rc = growScratch(in, in->jumpDev, doubles * sizeof(double) + mi355::MAX_JUMP_REGISTERS * sizeof(int)); if (rc) return rc;
    double* dReg = in->jumpDev.as<double>();
    double* dRateReg = dReg + nReg;
    double* dTmp = dRateReg + nReg;
    double* dM = dTmp + nReg;
    double* dCond = dM + nReg;
    double* dPart = dCond + nCond;
    double* dRow = dPart + nPart;
    double* dPat = dRow + nRow;
    double* dStage = dPat + nPat;
    int* dFlags = (int*)(dStage + nStage);
    std::vector<int> fl(K, 0);
    if (registerFlags) for (int k = 0; k < K; k++) fl[k] = registerFlags[k];
    rc = upload(in, dReg, registers, nReg * sizeof(double)); if (rc) return rc;
    rc = upload(in, dFlags, fl.data(), K * sizeof(int)); if (rc) return rc;
    std::vector<mi355::JumpRow> rows(nodeCount);
    for (int r = 0; r < nodeCount; r++) {
        mi355::JumpRow& row = rows[r];
        row.time = branchTimes[r];
        row.rate = branchRates ? branchRates[r] : 1.0;
        row.matrix = r == 0 ? nullptr : in->matrices + (size_t)C * SS * nodes[3 * r + 1];
        row.parent = r == 0 ? -1 : nodes[3 * r + 2];
        row.pad = 0;
    }
    void* dRowsV = nullptr;
    rc = uploadTransient(in, rows.data(), rows.size() * sizeof(mi355::JumpRow), &dRowsV); if (rc) return rc;
    const mi355::JumpRow* dRows = (const mi355::JumpRow*)dRowsV;
    const double* eig = in->eigen + (2 * SS + S) * (size_t)eigenIndex;
    const double* rates = in->rates + (size_t)ratesIndex * C;
    mi355::launchJumpRegisters(live(in), eig, dReg, dFlags, K, S, dRateReg, dTmp, dM);
    mi355::launchJumpMatrices(live(in), dRows, nodeCount, eig, rates, dM, dFlags, K, S, C, dCond);
    HIP_TRY(hipGetLastError());
    const size_t chunk = outJumps ? stageRows : R;
    for (size_t r0 = 0; r0 < R; r0 += chunk) {
        const size_t r1 = std::min(R, r0 + chunk);
        mi355::launchJumpSites(live(in), dRows, nodeCount, (int)r0, (int)r1, d.states, d.cats, dCond, K, S, C, P,
                               outJumps ? dStage : nullptr, dPat, dPart, d.error);
        HIP_TRY(hipGetLastError());
        if (!outJumps) continue;
        for (int k = 0; k < K; k++)
            HIP_TRY(hipMemcpy2DAsync(outJumps + ((size_t)k * R + r0) * globalP + pOffset, (size_t)globalP * sizeof(double),
                                     dStage + (size_t)k * (r1 - r0) * P, (size_t)P * sizeof(double), (size_t)P * sizeof(double), r1 - r0,
                                     hipMemcpyDeviceToHost, live(in)));
        HIP_TRY(hipStreamSynchronize(live(in)));           // (the next chunk overwrites the stage)
    }
    mi355::launchJumpRowTotals(live(in), dPart, (int)blocks, K, nodeCount, dRow);
    HIP_TRY(hipGetLastError());
    if (outPatternTotals)
        HIP_TRY(hipMemcpy2DAsync(outPatternTotals + pOffset, (size_t)globalP * sizeof(double), dPat, (size_t)P * sizeof(double),
                                 (size_t)P * sizeof(double), (size_t)K, hipMemcpyDeviceToHost, live(in)));
    if (outRowTotals) HIP_TRY(hipMemcpyAsync(outRowTotals, dRow, nRow * sizeof(double), hipMemcpyDeviceToHost, live(in)));
    unsigned err = 0;
    rc = copyAncestral(in, d, nodeCount, globalP, pOffset, outStates, outCategories, &err); if (rc) return rc;
    return err ? BEAGLE_ERROR_FLOATING_POINT : BEAGLE_SUCCESS;
}

extern "C" {

int beagleMi355SampleMarkovJumps(int instance, const int* nodes, int nodeCount, const double* branchTimes, const double* branchRates,
                                 int eigenIndex, int categoryRatesIndex, int categoryWeightsIndex, int stateFrequenciesIndex,
                                 const double* registers, const int* registerFlags, int registerCount, unsigned long long seed, int flags,
                                 unsigned char* outStates, int* outRateCategories, double* outJumps, double* outPatternTotals,
                                 double* outRowTotals) {
    if (!nodes || nodeCount < 1 || !branchTimes || !registers) return BEAGLE_ERROR_OUT_OF_RANGE;
    if (registerCount < 1 || registerCount > mi355::MAX_JUMP_REGISTERS) return BEAGLE_ERROR_OUT_OF_RANGE;
    if (!outJumps && !outPatternTotals && !outRowTotals) return BEAGLE_ERROR_OUT_OF_RANGE;
    if (registerFlags)
        for (int k = 0; k < registerCount; k++)
            if (registerFlags[k] & ~(BEAGLE_MI355_JUMPS_REWARDS | BEAGLE_MI355_JUMPS_SCALE_BY_TIME)) return BEAGLE_ERROR_OUT_OF_RANGE;
    const size_t nRow = (size_t)registerCount * nodeCount;
    if (mi355::isShardedHandle(instance)) {
        // every shard fills its own columns; the row totals are the shards' sums, added in shard (= pattern) order
        const int globalP = mi355::shardedPatternCount(instance);
        std::mutex mu;
        std::vector<std::pair<int, std::vector<double>>> partial;
        const int rc = mi355::shardedBroadcast(instance, [&](int h) {
            int pStart = 0, pEnd = 0;
            mi355::shardedBoundsOfHandle(instance, h, &pStart, &pEnd);
            GET_INSTANCE(h);
            DEMOTE_FOLDED_TIPS(in);
            std::vector<double> rows(outRowTotals ? nRow : 0);
            const int r = sampleJumps(in, nodes, nodeCount, branchTimes, branchRates, eigenIndex, categoryRatesIndex, categoryWeightsIndex,
                                      stateFrequenciesIndex, registers, registerFlags, registerCount, seed, flags, globalP, pStart,
                                      outStates, outRateCategories, outJumps, outPatternTotals, outRowTotals ? rows.data() : nullptr);
            std::lock_guard<std::mutex> lock(mu);
            partial.emplace_back(pStart, std::move(rows));
            return r;
        });
        if (outRowTotals && (rc == BEAGLE_SUCCESS || rc == BEAGLE_ERROR_FLOATING_POINT)) {
            std::sort(partial.begin(), partial.end(), [](const std::pair<int, std::vector<double>>& a,
                                                         const std::pair<int, std::vector<double>>& b) { return a.first < b.first; });
            for (size_t i = 0; i < nRow; i++) {
                double s = partial[0].second[i];
                for (size_t q = 1; q < partial.size(); q++) s = s + partial[q].second[i];
                outRowTotals[i] = s;
            }
        }
        return rc;
    }
    GET_INSTANCE(instance);
    DEMOTE_FOLDED_TIPS(in);
    return sampleJumps(in, nodes, nodeCount, branchTimes, branchRates, eigenIndex, categoryRatesIndex, categoryWeightsIndex,
                       stateFrequenciesIndex, registers, registerFlags, registerCount, seed, flags, in->P, 0, outStates, outRateCategories,
                       outJumps, outPatternTotals, outRowTotals);
}

}  // extern "C"

// Sampled Markov-jump histories by uniformization (include/beagle_mi355.h beagleMi355SampleMarkovJumpsUniformized; what
// MarkovJumpsBeagleTreeLikelihood.computeSampledMarkovJumpsForBranch computes inside traverseSample with useUniformization = true,
// MarkovJumpsBeagleTreeLikelihood.java:473-509).  The draw is drawAncestral's, left on the device; then kernels_uniformized.hip:
// the R^n table, the histories per chunk of rows (at most 256 MiB of staged values), the pattern totals per chunk, the row totals
// (launchJumpRowTotals), and with histories the event offsets.  Writing the events is a second step (uniformEvents) so that the
// sharded handle can place every shard's list after the earlier shards' totals are known.
struct UniformPass {
    mi355::UniformSiteArgs args;
    long long events = 0, fallbacks = 0;
    bool wantEvents = false;
};

// mu = max_i -Q_ii in SubordinatedProcess.getMaxRate's order; R = Q / mu + I (constructDtmcMatrix).  false: mu not finite and > 0
static bool uniformChain(const double* Q, int S, double* mu, std::vector<double>& R) {
    for (int e = 0; e < S * S; e++)
        if (!std::isfinite(Q[e])) return false;
    double m = -Q[0];
    for (int i = 1; i < S; i++) {
        const double next = -Q[(size_t)i * S + i];
        if (next > m) m = next;
    }
    if (!(m > 0.0) || !(m <= DBL_MAX)) return false;
    R.assign((size_t)S * S, 0.0);
    for (int i = 0; i < S; i++)
        for (int j = 0; j < S; j++) {
            R[(size_t)i * S + j] = Q[(size_t)i * S + j] / m;
            if (i == j) R[(size_t)i * S + j] += 1.0;
        }
    *mu = m;
    return true;
}

// The length of the R^n table (header): min(1000, ceil(lambda + 20 sqrt(lambda)) + 40), lambda = mu * the largest tau of the call
static int uniformTableLength(double mu, const double* branchTimes, const double* branchRates, int nodeCount, const double* catRates, int C) {
    double tmax = 0.0;
    for (int r = 1; r < nodeCount; r++)
        for (int c = 0; c < C; c++)
            if (catRates[c] > 0.0) {
                const double tau = (branchTimes[r] * (branchRates ? branchRates[r] : 1.0)) * catRates[c];
                if (!(tau <= tmax)) tmax = tau;
            }
    const double lambda = mu * tmax;
    if (!(lambda < 1000.0)) return mi355::UNIFORM_MAX_TRIES;
    return std::min(mi355::UNIFORM_MAX_TRIES, (int)std::ceil(lambda + 20.0 * std::sqrt(lambda)) + 40);
}

static int uniformRun(Instance* in, const int* nodes, int nodeCount, const double* branchTimes, const double* branchRates,
                      const double* nodeHeights, const double* Q, int ratesIndex, int wIdx, int fIdx, const double* registers,
                      const int* registerFlags, int K, int simulants, unsigned long long seed, int flags, int globalP, int pOffset,
                      unsigned char* outStates, int* outCategories, double* outJumps, double* outPatternTotals, double* outRowTotals,
                      int* outEventCounts, bool history, UniformPass* pass) {
    if (badIndex(ratesIndex, in->eigenCount)) return BEAGLE_ERROR_OUT_OF_RANGE;
    const int S = in->S, C = in->C, P = in->P;
    double mu = 0.0;
    std::vector<double> R;
    if (!uniformChain(Q, S, &mu, R)) return BEAGLE_ERROR_OUT_OF_RANGE;
    AncestralDraw d;
    int rc = drawAncestral(in, nodes, nodeCount, wIdx, fIdx, seed, flags, globalP, pOffset, &d); if (rc) return rc;
    const double* dRates = in->rates + (size_t)ratesIndex * C;
    std::vector<double> catRates(C);
    rc = download(in, catRates.data(), dRates, C * sizeof(double)); if (rc) return rc;
    const int N = uniformTableLength(mu, branchTimes, branchRates, nodeCount, catRates.data(), C);
    const size_t SS = (size_t)S * S, Rn = (size_t)nodeCount, blocks = (size_t)mi355::jumpSiteBlocks(P);
    const size_t stageRows = std::max<size_t>(1, std::min<size_t>({Rn, (256ull << 20) / ((size_t)K * P * sizeof(double)), 65535}));
    // uniformDev: table [N][S][S] | registers [K][S][S] | blockPartials [blocks][K][R] | rowTotals [K][R] | patternTotals [K][P]
    //             | stage [K][stageRows][P] (doubles) | rows [R] | register flags int [K] | pattern offsets + total, fallbacks
    //             long long [P + 2] | event counts int [R][P] (histories)
    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t nTable = (size_t)N * SS, nReg = (size_t)K * SS, nPart = blocks * K * Rn, nRow = (size_t)K * Rn, nPat = (size_t)K * P,
                 nStage = (size_t)K * stageRows * P;
    const size_t oRows = up((nTable + nReg + nPart + nRow + nPat + nStage) * sizeof(double));
    const size_t oFlags = oRows + up(Rn * sizeof(mi355::UniformRow));
    const size_t oLong = oFlags + up(mi355::MAX_JUMP_REGISTERS * sizeof(int));
    const size_t oCounts = oLong + up(((size_t)P + 2) * sizeof(long long));
    const size_t bytes = oCounts + (history ? Rn * P * sizeof(int) : 0);
    rc = growScratch(in, in->uniformDev, bytes); if (rc) return rc;
    char* base = in->uniformDev.p;
    double* dTable = (double*)base;
    double* dReg = dTable + nTable;
    double* dPart = dReg + nReg;
    double* dRow = dPart + nPart;
    double* dPat = dRow + nRow;
    double* dStage = dPat + nPat;
    mi355::UniformRow* dRowsU = (mi355::UniformRow*)(base + oRows);
    int* dFlags = (int*)(base + oFlags);
    long long* dLong = (long long*)(base + oLong);
    int* dCounts = history ? (int*)(base + oCounts) : nullptr;

    std::vector<double> head(2 * SS, 0.0);
    for (int i = 0; i < S; i++) head[(size_t)i * S + i] = 1.0;
    std::copy(R.begin(), R.end(), head.begin() + SS);
    rc = upload(in, dTable, head.data(), head.size() * sizeof(double)); if (rc) return rc;
    rc = upload(in, dReg, registers, nReg * sizeof(double)); if (rc) return rc;
    std::vector<int> fl(K, 0);
    if (registerFlags) for (int k = 0; k < K; k++) fl[k] = registerFlags[k];
    rc = upload(in, dFlags, fl.data(), K * sizeof(int)); if (rc) return rc;
    std::vector<mi355::UniformRow> rows(nodeCount);
    for (int r = 0; r < nodeCount; r++) {
        mi355::UniformRow& row = rows[r];
        row.time = branchTimes[r];
        row.rate = branchRates ? branchRates[r] : 1.0;
        row.parent = r == 0 ? -1 : nodes[3 * r + 2];
        row.hChild = nodeHeights ? nodeHeights[r] : 0.0;
        row.hParent = nodeHeights && r > 0 ? nodeHeights[row.parent] : 0.0;
        row.matrix = r == 0 ? nullptr : in->matrices + (size_t)C * SS * nodes[3 * r + 1];
        row.pad = 0;
    }
    rc = upload(in, dRowsU, rows.data(), rows.size() * sizeof(mi355::UniformRow)); if (rc) return rc;
    HIP_TRY(hipMemsetAsync(dLong + P + 1, 0, sizeof(long long), live(in)));
    mi355::launchUniformPowers(live(in), dTable, S, N);
    HIP_TRY(hipGetLastError());

    mi355::UniformSiteArgs& a = pass->args;
    a = mi355::UniformSiteArgs{};
    a.rows = dRowsU; a.states = d.states; a.cats = d.cats; a.rates = dRates; a.table = dTable; a.registers = dReg; a.regFlags = dFlags;
    a.stage = dStage; a.blockPartials = dPart; a.eventCounts = dCounts; a.patternOffsets = dLong; a.fpError = d.error;
    a.fallbacks = (unsigned long long*)(dLong + P + 1); a.seed = seed; a.mu = mu; a.nRows = nodeCount; a.K = K; a.S = S; a.P = P;
    a.N = N; a.simulants = simulants; a.stageRows = (int)stageRows; a.globalP = globalP; a.pOffset = pOffset;
    for (size_t r0 = 0; r0 < Rn; r0 += stageRows) {
        const size_t r1 = std::min(Rn, r0 + stageRows);
        mi355::launchUniformSites(live(in), a, (int)r0, (int)r1, false);
        mi355::launchUniformPatternTotals(live(in), dStage, (int)stageRows, (int)r0, (int)r1, K, P, dPat);
        HIP_TRY(hipGetLastError());
        if (!outJumps) continue;
        for (int k = 0; k < K; k++)
            HIP_TRY(hipMemcpy2DAsync(outJumps + ((size_t)k * Rn + r0) * globalP + pOffset, (size_t)globalP * sizeof(double),
                                     dStage + (size_t)k * stageRows * P, (size_t)P * sizeof(double), (size_t)P * sizeof(double), r1 - r0,
                                     hipMemcpyDeviceToHost, live(in)));
        HIP_TRY(hipStreamSynchronize(live(in)));           // (the next chunk overwrites the stage)
    }
    mi355::launchJumpRowTotals(live(in), dPart, (int)blocks, K, nodeCount, dRow);
    HIP_TRY(hipGetLastError());
    if (outPatternTotals)
        HIP_TRY(hipMemcpy2DAsync(outPatternTotals + pOffset, (size_t)globalP * sizeof(double), dPat, (size_t)P * sizeof(double),
                                 (size_t)P * sizeof(double), (size_t)K, hipMemcpyDeviceToHost, live(in)));
    if (outRowTotals) HIP_TRY(hipMemcpyAsync(outRowTotals, dRow, nRow * sizeof(double), hipMemcpyDeviceToHost, live(in)));
    if (history) {
        if (outEventCounts)
            HIP_TRY(hipMemcpy2DAsync(outEventCounts + pOffset, (size_t)globalP * sizeof(int), dCounts, (size_t)P * sizeof(int),
                                     (size_t)P * sizeof(int), Rn, hipMemcpyDeviceToHost, live(in)));
        mi355::launchEventOffsets(live(in), dCounts, nodeCount, P, dLong);
        HIP_TRY(hipGetLastError());
    }
    long long tail[2] = {0, 0};                            // events, fallbacks
    rc = download(in, tail, dLong + P, sizeof(tail)); if (rc) return rc;
    pass->events = history ? tail[0] : 0;
    pass->fallbacks = tail[1];
    unsigned err = 0;
    rc = copyAncestral(in, d, nodeCount, globalP, pOffset, outStates, outCategories, &err); if (rc) return rc;
    return err ? BEAGLE_ERROR_FLOATING_POINT : BEAGLE_SUCCESS;
}

// The event list of the last uniformRun on `in`: the same histories again, written at outHeights / outStates (this instance's first event)
static int uniformEvents(Instance* in, UniformPass* pass, double* outHeights, unsigned char* outStates) {
    if (pass->events == 0) return 0;
    const size_t n = (size_t)pass->events;
    const size_t stBytes = (2 * n + 255) & ~(size_t)255;
    int rc = growScratch(in, in->eventDev, stBytes + n * sizeof(double)); if (rc) return rc;
    mi355::UniformSiteArgs a = pass->args;
    a.eventStates = in->eventDev.as<uint8_t>();
    a.eventHeights = (double*)(in->eventDev.p + stBytes);
    for (int r0 = 0; r0 < a.nRows; r0 += 65535)
        mi355::launchUniformSites(live(in), a, r0, std::min(a.nRows, r0 + 65535), true);
    HIP_TRY(hipGetLastError());
    if (outHeights) HIP_TRY(hipMemcpyAsync(outHeights, a.eventHeights, n * sizeof(double), hipMemcpyDeviceToHost, live(in)));
    if (outStates) HIP_TRY(hipMemcpyAsync(outStates, a.eventStates, 2 * n, hipMemcpyDeviceToHost, live(in)));
    HIP_TRY(hipStreamSynchronize(live(in)));
    return 0;
}

extern "C" {

int beagleMi355SampleMarkovJumpsUniformized(int instance, const int* nodes, int nodeCount, const double* branchTimes,
                                            const double* branchRates, const double* nodeHeights, const double* infinitesimalMatrix,
                                            int categoryRatesIndex, int categoryWeightsIndex, int stateFrequenciesIndex,
                                            const double* registers, const int* registerFlags, int registerCount, int simulantCount,
                                            unsigned long long seed, int flags, unsigned char* outStates, int* outRateCategories,
                                            double* outJumps, double* outPatternTotals, double* outRowTotals, int* outEventCounts,
                                            long long eventCapacity, double* outEventHeights, unsigned char* outEventStates,
                                            long long* outEventTotal, long long* outFallbacks) {
    if (!nodes || nodeCount < 1 || !branchTimes || !registers || !infinitesimalMatrix) return BEAGLE_ERROR_OUT_OF_RANGE;
    if (registerCount < 1 || registerCount > mi355::MAX_JUMP_REGISTERS) return BEAGLE_ERROR_OUT_OF_RANGE;
    if (simulantCount < 1 || simulantCount > mi355::UNIFORM_MAX_SIMULANTS) return BEAGLE_ERROR_OUT_OF_RANGE;
    if (registerFlags)
        for (int k = 0; k < registerCount; k++)
            if (registerFlags[k] & ~(BEAGLE_MI355_JUMPS_REWARDS | BEAGLE_MI355_JUMPS_SCALE_BY_TIME)) return BEAGLE_ERROR_OUT_OF_RANGE;
    const bool wantEvents = outEventHeights || outEventStates;
    const bool history = outEventCounts || wantEvents || outEventTotal;
    if (!outJumps && !outPatternTotals && !outRowTotals && !history) return BEAGLE_ERROR_OUT_OF_RANGE;
    if (history && (simulantCount > 1 || !nodeHeights)) return BEAGLE_ERROR_OUT_OF_RANGE;
    if (wantEvents && eventCapacity < 0) return BEAGLE_ERROR_OUT_OF_RANGE;
    if (outEventTotal) *outEventTotal = 0;
    if (outFallbacks) *outFallbacks = 0;
    const size_t nRow = (size_t)registerCount * nodeCount;
    if (mi355::isShardedHandle(instance)) {
        // phase 1: every shard draws, simulates and fills its own columns; phase 2: its events after the earlier shards' events
        const int globalP = mi355::shardedPatternCount(instance);
        std::mutex mu;
        std::map<int, std::pair<int, std::vector<double>>> partial;      // shard handle -> (pStart, row totals)
        std::map<int, UniformPass> passes;
        int rc = mi355::shardedBroadcast(instance, [&](int h) {
            int pStart = 0, pEnd = 0;
            mi355::shardedBoundsOfHandle(instance, h, &pStart, &pEnd);
            GET_INSTANCE(h);
            DEMOTE_FOLDED_TIPS(in);
            std::vector<double> rows(outRowTotals ? nRow : 0);
            UniformPass pass;
            const int r = uniformRun(in, nodes, nodeCount, branchTimes, branchRates, nodeHeights, infinitesimalMatrix, categoryRatesIndex,
                                     categoryWeightsIndex, stateFrequenciesIndex, registers, registerFlags, registerCount, simulantCount,
                                     seed, flags, globalP, pStart, outStates, outRateCategories, outJumps, outPatternTotals,
                                     outRowTotals ? rows.data() : nullptr, outEventCounts, history, &pass);
            std::lock_guard<std::mutex> lock(mu);
            partial[h] = std::make_pair(pStart, std::move(rows));
            passes[h] = pass;
            return r;
        });
        if (rc != BEAGLE_SUCCESS && rc != BEAGLE_ERROR_FLOATING_POINT) return rc;
        std::vector<std::pair<int, int>> order;                          // (pStart, handle) in shard order
        for (auto& e : partial) order.emplace_back(e.second.first, e.first);
        std::sort(order.begin(), order.end());
        if (outRowTotals)
            for (size_t i = 0; i < nRow; i++) {
                double s = partial[order[0].second].second[i];
                for (size_t q = 1; q < order.size(); q++) s = s + partial[order[q].second].second[i];
                outRowTotals[i] = s;
            }
        long long total = 0, fallbacks = 0;
        std::map<int, long long> first;
        for (auto& o : order) {
            first[o.second] = total;
            total += passes[o.second].events;
            fallbacks += passes[o.second].fallbacks;
        }
        if (outEventTotal) *outEventTotal = total;
        if (outFallbacks) *outFallbacks = fallbacks;
        if (!wantEvents) return rc;
        if (total > eventCapacity) return BEAGLE_ERROR_OUT_OF_RANGE;
        const int rcEvents = mi355::shardedBroadcast(instance, [&](int h) {
            GET_INSTANCE(h);
            const long long f = first[h];
            return uniformEvents(in, &passes[h], outEventHeights ? outEventHeights + f : nullptr,
                                 outEventStates ? outEventStates + 2 * f : nullptr);
        });
        return rcEvents ? rcEvents : rc;
    }
    GET_INSTANCE(instance);
    DEMOTE_FOLDED_TIPS(in);
    UniformPass pass;
    int rc = uniformRun(in, nodes, nodeCount, branchTimes, branchRates, nodeHeights, infinitesimalMatrix, categoryRatesIndex,
                        categoryWeightsIndex, stateFrequenciesIndex, registers, registerFlags, registerCount, simulantCount, seed, flags,
                        in->P, 0, outStates, outRateCategories, outJumps, outPatternTotals, outRowTotals, outEventCounts, history, &pass);
    if (rc != BEAGLE_SUCCESS && rc != BEAGLE_ERROR_FLOATING_POINT) return rc;
    if (outEventTotal) *outEventTotal = pass.events;
    if (outFallbacks) *outFallbacks = pass.fallbacks;
    if (!wantEvents) return rc;
    if (pass.events > eventCapacity) return BEAGLE_ERROR_OUT_OF_RANGE;
    const int rcEvents = uniformEvents(in, &pass, outEventHeights, outEventStates);
    return rcEvents ? rcEvents : rc;
}

}  // extern "C"
