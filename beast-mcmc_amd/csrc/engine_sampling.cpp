// engine_sampling.cpp — the device samplers: ancestral-state draws, Markov-jump counts and rewards, uniformized histories; each one
// call over a list of nodes.  Also what the other samplers' files share with them: the staged copy-out, the event list's buffer.
#include "engine_internal.h"

#include <cfloat>
#include <map>

using namespace mi355::eng;
namespace scratch = mi355::scratch;

int mi355::eng::copyStagedRows(Instance* in, const double* stage, size_t stride, size_t r0, size_t r1, int K, size_t R, size_t P,
                               size_t globalP, size_t pOffset, double* out) {
    for (int k = 0; k < K; k++) {
        double* dst = out + ((size_t)k * R + r0) * globalP + pOffset;
        const double* src = stage + (size_t)k * stride * P;
        if (globalP == P)
            HIP_TRY(hipMemcpyAsync(dst, src, (r1 - r0) * P * sizeof(double), hipMemcpyDeviceToHost, live(in)));
        else
            HIP_TRY(hipMemcpy2DAsync(dst, globalP * sizeof(double), src, P * sizeof(double), P * sizeof(double), r1 - r0,
                                     hipMemcpyDeviceToHost, live(in)));
    }
    HIP_TRY(hipStreamSynchronize(live(in)));
    return 0;
}

int mi355::eng::copyJumpTotals(Instance* in, const double* dPat, const double* dRow, int K, size_t R, size_t P, size_t globalP,
                               size_t pOffset, double* outPatternTotals, double* outRowTotals) {
    if (outPatternTotals)
        HIP_TRY(hipMemcpy2DAsync(outPatternTotals + pOffset, globalP * sizeof(double), dPat, P * sizeof(double), P * sizeof(double),
                                 (size_t)K, hipMemcpyDeviceToHost, live(in)));
    if (outRowTotals) HIP_TRY(hipMemcpyAsync(outRowTotals, dRow, (size_t)K * R * sizeof(double), hipMemcpyDeviceToHost, live(in)));
    return 0;
}

int mi355::eng::growEvents(Instance* in, size_t n, uint8_t** states, double** heights) {
    const scratch::EventLayout L(n);
    int rc = growScratch(in, in->eventDev, L.bytes()); if (rc) return rc;
    *states = L.states.at(in->eventDev.p);
    *heights = L.heights.at(in->eventDev.p);
    return 0;
}

int mi355::eng::copyEvents(Instance* in, size_t n, const uint8_t* states, const double* heights, unsigned char* outStates,
                           double* outHeights) {
    if (outHeights) HIP_TRY(hipMemcpyAsync(outHeights, heights, n * sizeof(double), hipMemcpyDeviceToHost, live(in)));
    if (outStates) HIP_TRY(hipMemcpyAsync(outStates, states, 2 * n, hipMemcpyDeviceToHost, live(in)));
    HIP_TRY(hipStreamSynchronize(live(in)));
    return 0;
}

// the registers [K][S][S] and their flags (NULL: none set) to the device
static int uploadRegisters(Instance* in, double* dReg, const double* registers, size_t nReg, int* dFlags, const int* registerFlags, int K) {
    std::vector<int> fl(K, 0);
    if (registerFlags) for (int k = 0; k < K; k++) fl[k] = registerFlags[k];
    int rc = upload(in, dReg, registers, nReg * sizeof(double)); if (rc) return rc;
    return upload(in, dFlags, fl.data(), K * sizeof(int));
}

// The draw itself, left on the device (AncestralDraw, engine_internal.h): validation, materialising virtual buffers, ONE launch
// (kernels_ancestral.hip).
int mi355::eng::drawAncestral(Instance* in, const int* nodes, int nodeCount, int wIdx, int fIdx, unsigned long long seed, int flags,
                              int globalP, int pOffset, AncestralDraw* d) {
    if (in->partitionCount > 1) return BEAGLE_ERROR_NO_IMPLEMENTATION;
    if (badIndex(wIdx, in->eigenCount) || badIndex(fIdx, in->eigenCount)) return BEAGLE_ERROR_OUT_OF_RANGE;
    ReadSet reads(in);
    for (int r = 0; r < nodeCount; r++) {
        const int b = nodes[3 * r], m = nodes[3 * r + 1], parent = nodes[3 * r + 2];
        if (badIndex(b, in->partialsCount)) return BEAGLE_ERROR_OUT_OF_RANGE;
        if (r == 0 && isCompactTip(in, b)) return BEAGLE_ERROR_OUT_OF_RANGE;
        if (r > 0 && (badIndex(m, in->matrixCount) || parent < 0 || parent >= r)) return BEAGLE_ERROR_OUT_OF_RANGE;
        if (int bad = reads.post(b)) return bad;
    }
    int rc = reads.materialize(); if (rc) return rc;
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
    const scratch::AncestralLayout L(nodeCount, in->P);
    rc = growScratch(in, in->ancestralDev, L.bytes()); if (rc) return rc;
    d->states = L.states.at(in->ancestralDev.p);
    d->cats = L.cats.at(in->ancestralDev.p);
    d->error = L.error.at(in->ancestralDev.p);                 // (right behind the categories: copyAncestral takes both in one copy)
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

// The instance behind shard handle h of `handle` (a plain handle: itself) made ready for a sampler (the samplers read tips' partials
// as data: engine_tipemission.cpp), and which patterns of how many it holds
static int samplerInstance(int handle, int h, Instance** out, int* globalP, int* pStart) {
    GET_INSTANCE(h);
    DEMOTE_FOLDED_TIPS(in);
    int pEnd = 0;
    *out = in; *globalP = in->P; *pStart = 0;
    if (mi355::isShardedHandle(handle)) { mi355::shardedBoundsOfHandle(handle, h, pStart, &pEnd); *globalP = mi355::shardedPatternCount(handle); }
    return 0;
}

// One draw of every listed node's state per pattern (include/beagle_mi355.h beagleMi355SampleAncestralStates; what
// AncestralStateBeagleTreeLikelihood.traverseSample computes from a getPartials per internal node and a getTransitionMatrix per
// branch, AncestralStateBeagleTreeLikelihood.java:414-625).  Virtual buffers are materialised by one walk, as for a read-back; the
// draw itself is ONE launch (kernels_ancestral.hip), then the states and categories come back in two copies.  The instance's
// patterns are patterns pOffset .. pOffset + P - 1 of an alignment of globalP (the sharded handle): the random numbers are keyed
// on the global pattern, and row r's states land at outStates + r * globalP + pOffset.
extern "C" {

int beagleMi355SampleAncestralStates(int instance, const int* nodes, int nodeCount, int categoryWeightsIndex, int stateFrequenciesIndex,
                                     unsigned long long seed, int flags, unsigned char* outStates, int* outRateCategories) {
    if (!nodes || nodeCount < 1 || !outStates) return BEAGLE_ERROR_OUT_OF_RANGE;
    return mi355::shardedOrPlain(instance, [&](int h) {      // every shard draws its own pattern range into its columns of the caller's arrays
        Instance* in = nullptr;
        int globalP = 0, pStart = 0;
        int rc = samplerInstance(instance, h, &in, &globalP, &pStart); if (rc) return rc;
        AncestralDraw d;
        rc = drawAncestral(in, nodes, nodeCount, categoryWeightsIndex, stateFrequenciesIndex, seed, flags, globalP, pStart, &d); if (rc) return rc;
        unsigned err = 0;
        rc = copyAncestral(in, d, nodeCount, globalP, pStart, outStates, outRateCategories, &err); if (rc) return rc;
        return err ? (int)BEAGLE_ERROR_FLOATING_POINT : (int)BEAGLE_SUCCESS;
    });
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
    const size_t stageRows = outJumps ? stageRowCount(R, K, P) : 0;
    const scratch::JumpLayout L(S, C, P, K, R, blocks, stageRows);
    rc = growScratch(in, in->jumpDev, L.bytes()); if (rc) return rc;
    char* base = in->jumpDev.p;
    double *dReg = L.reg.at(base), *dM = L.M.at(base), *dCond = L.cond.at(base), *dPart = L.part.at(base), *dRow = L.row.at(base),
           *dPat = L.pat.at(base), *dStage = L.stage.at(base);           // (dStage: NULL without outJumps)
    int* dFlags = L.flags.at(base);
    rc = uploadRegisters(in, dReg, registers, L.reg.count, dFlags, registerFlags, K); if (rc) return rc;
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
    mi355::launchJumpRegisters(live(in), eig, dReg, dFlags, K, S, L.rateReg.at(base), L.tmp.at(base), dM);
    mi355::launchJumpMatrices(live(in), dRows, nodeCount, eig, rates, dM, dFlags, K, S, C, dCond);
    HIP_TRY(hipGetLastError());
    const size_t chunk = outJumps ? stageRows : R;
    for (size_t r0 = 0; r0 < R; r0 += chunk) {
        const size_t r1 = std::min(R, r0 + chunk);
        mi355::launchJumpSites(live(in), dRows, nodeCount, (int)r0, (int)r1, d.states, d.cats, dCond, K, S, C, P, dStage, dPat, dPart,
                               d.error);
        HIP_TRY(hipGetLastError());
        if (outJumps) { rc = copyStagedRows(in, dStage, r1 - r0, r0, r1, K, R, P, globalP, pOffset, outJumps); if (rc) return rc; }
    }
    mi355::launchBlockTotals(live(in), dPart, (int)blocks, K, nodeCount, 1, dRow);
    HIP_TRY(hipGetLastError());
    rc = copyJumpTotals(in, dPat, dRow, K, R, P, globalP, pOffset, outPatternTotals, outRowTotals); if (rc) return rc;
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
    if (!checkRegisterFlags(registerFlags, registerCount, BEAGLE_MI355_JUMPS_REWARDS | BEAGLE_MI355_JUMPS_SCALE_BY_TIME))
        return BEAGLE_ERROR_OUT_OF_RANGE;
    const size_t nRow = (size_t)registerCount * nodeCount;
    // every shard (a plain handle: the instance) fills its own columns; the row totals are the shards' sums, added in shard (= pattern) order
    std::mutex mu;
    std::map<int, mi355::ShardPart> parts;
    const int rc = mi355::shardedOrPlain(instance, [&](int h) {
        Instance* in = nullptr;
        int globalP = 0;
        mi355::ShardPart part;
        int r = samplerInstance(instance, h, &in, &globalP, &part.start); if (r) return r;
        part.rowTotals.resize(outRowTotals ? nRow : 0);
        r = sampleJumps(in, nodes, nodeCount, branchTimes, branchRates, eigenIndex, categoryRatesIndex, categoryWeightsIndex,
                        stateFrequenciesIndex, registers, registerFlags, registerCount, seed, flags, globalP, part.start, outStates,
                        outRateCategories, outJumps, outPatternTotals, outRowTotals ? part.rowTotals.data() : nullptr);
        std::lock_guard<std::mutex> lock(mu);
        parts[h] = std::move(part);
        return r;
    });
    if (outRowTotals && (rc == BEAGLE_SUCCESS || rc == BEAGLE_ERROR_FLOATING_POINT))
        mi355::sumRowTotals(mi355::orderedParts(parts), nRow, outRowTotals);
    return rc;
}

}  // extern "C"

// Sampled Markov-jump histories by uniformization (include/beagle_mi355.h beagleMi355SampleMarkovJumpsUniformized; what
// MarkovJumpsBeagleTreeLikelihood.computeSampledMarkovJumpsForBranch computes inside traverseSample with useUniformization = true,
// MarkovJumpsBeagleTreeLikelihood.java:473-509).  The draw is drawAncestral's, left on the device; then kernels_uniformized.hip:
// the R^n table, the histories per chunk of rows (at most 256 MiB of staged values), the pattern totals per chunk, the row totals
// (launchBlockTotals), and with histories the event offsets.  Writing the events is a second step (uniformEvents) so that the
// sharded handle can place every shard's list after the earlier shards' totals are known.
struct UniformPass : mi355::ShardPart {                    // (start: the instance's first pattern)
    mi355::UniformSiteArgs args;
    long long fallbacks = 0;
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
                      unsigned char* outStates, int* outCategories, double* outJumps, double* outPatternTotals, bool rowTotals,
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
    const size_t stageRows = stageRowCount(Rn, K, P, 65535);           // (65535: a grid's y extent)
    const scratch::UniformLayout L(S, P, K, Rn, blocks, stageRows, N, sizeof(mi355::UniformRow), history);
    rc = growScratch(in, in->uniformDev, L.bytes()); if (rc) return rc;
    char* base = in->uniformDev.p;
    double *dTable = L.table.at(base), *dReg = L.reg.at(base), *dPart = L.part.at(base), *dRow = L.row.at(base), *dPat = L.pat.at(base),
           *dStage = L.stage.at(base);
    mi355::UniformRow* dRowsU = L.rows.as<mi355::UniformRow>(base);
    int* dFlags = L.flags.at(base);
    long long* dLong = L.longs.at(base);
    int* dCounts = L.counts.at(base);                       // (NULL without histories)

    std::vector<double> head(2 * SS, 0.0);
    for (int i = 0; i < S; i++) head[(size_t)i * S + i] = 1.0;
    std::copy(R.begin(), R.end(), head.begin() + SS);
    rc = upload(in, dTable, head.data(), head.size() * sizeof(double)); if (rc) return rc;
    rc = uploadRegisters(in, dReg, registers, L.reg.count, dFlags, registerFlags, K); if (rc) return rc;
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
        if (outJumps) { rc = copyStagedRows(in, dStage, stageRows, r0, r1, K, Rn, P, globalP, pOffset, outJumps); if (rc) return rc; }
    }
    mi355::launchBlockTotals(live(in), dPart, (int)blocks, K, nodeCount, 1, dRow);
    HIP_TRY(hipGetLastError());
    pass->start = pOffset;
    pass->rowTotals.resize(rowTotals ? (size_t)K * Rn : 0);
    rc = copyJumpTotals(in, dPat, dRow, K, Rn, P, globalP, pOffset, outPatternTotals, rowTotals ? pass->rowTotals.data() : nullptr);
    if (rc) return rc;
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
static int uniformEvents(Instance* in, const UniformPass& pass, double* outHeights, unsigned char* outStates) {
    if (pass.events == 0) return 0;
    mi355::UniformSiteArgs a = pass.args;
    int rc = growEvents(in, (size_t)pass.events, &a.eventStates, &a.eventHeights); if (rc) return rc;
    for (int r0 = 0; r0 < a.nRows; r0 += 65535)
        mi355::launchUniformSites(live(in), a, r0, std::min(a.nRows, r0 + 65535), true);
    HIP_TRY(hipGetLastError());
    return copyEvents(in, (size_t)pass.events, a.eventStates, a.eventHeights, outStates, outHeights);
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
    if (!checkRegisterFlags(registerFlags, registerCount, BEAGLE_MI355_JUMPS_REWARDS | BEAGLE_MI355_JUMPS_SCALE_BY_TIME))
        return BEAGLE_ERROR_OUT_OF_RANGE;
    const bool wantEvents = outEventHeights || outEventStates;
    const bool history = outEventCounts || wantEvents || outEventTotal;
    if (!outJumps && !outPatternTotals && !outRowTotals && !history) return BEAGLE_ERROR_OUT_OF_RANGE;
    if (history && (simulantCount > 1 || !nodeHeights)) return BEAGLE_ERROR_OUT_OF_RANGE;
    if (wantEvents && eventCapacity < 0) return BEAGLE_ERROR_OUT_OF_RANGE;
    if (outEventTotal) *outEventTotal = 0;
    if (outFallbacks) *outFallbacks = 0;
    // phase 1: every shard (a plain handle: the instance) draws, simulates and fills its own columns; phase 2: its events after the
    // earlier shards' events.  The row totals are the shards' sums, added in shard (= pattern) order.
    std::mutex mu;
    std::map<int, UniformPass> passes;                              // shard handle -> its pass
    const int rc = mi355::shardedOrPlain(instance, [&](int h) {
        Instance* in = nullptr;
        int globalP = 0, pStart = 0;
        int r = samplerInstance(instance, h, &in, &globalP, &pStart); if (r) return r;
        UniformPass pass;
        r = uniformRun(in, nodes, nodeCount, branchTimes, branchRates, nodeHeights, infinitesimalMatrix, categoryRatesIndex,
                       categoryWeightsIndex, stateFrequenciesIndex, registers, registerFlags, registerCount, simulantCount, seed, flags,
                       globalP, pStart, outStates, outRateCategories, outJumps, outPatternTotals, outRowTotals != nullptr,
                       outEventCounts, history, &pass);
        std::lock_guard<std::mutex> lock(mu);
        passes[h] = std::move(pass);
        return r;
    });
    if (rc != BEAGLE_SUCCESS && rc != BEAGLE_ERROR_FLOATING_POINT) return rc;
    const mi355::ShardParts order = mi355::orderedParts(passes);
    if (outRowTotals) mi355::sumRowTotals(order, (size_t)registerCount * nodeCount, outRowTotals);
    long long fallbacks = 0;
    for (const auto& o : order) fallbacks += passes[o.first].fallbacks;
    if (outFallbacks) *outFallbacks = fallbacks;
    return mi355::placeEvents(instance, order, wantEvents, eventCapacity, outEventTotal, rc, [&](int h, long long first) {
        GET_INSTANCE(h);
        return uniformEvents(in, passes[h], outEventHeights ? outEventHeights + first : nullptr,
                             outEventStates ? outEventStates + 2 * first : nullptr);
    });
}

}  // extern "C"
