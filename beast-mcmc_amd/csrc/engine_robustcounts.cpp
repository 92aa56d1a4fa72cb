// engine_robustcounts.cpp — codon robust counting: the conditional counts of the 64-state product chain over three instances'
// ancestral draws in one call, and the unconditioned count simulation; argument checks, the scratch layout, the launches.
#include "engine_internal.h"

using namespace mi355::eng;

namespace {

constexpr int SS64 = mi355::ROBUST_STATES * mi355::ROBUST_STATES;

// the events that order the other instances' draws in front of the gather: destroyed on every exit path
struct DrawEvents {
    hipEvent_t ev[2] = {nullptr, nullptr};
    ~DrawEvents() { for (hipEvent_t e : ev) if (e) hipEventDestroy(e); }
};

// one of the three position instances: an ordinary single-device 4-state instance with one pattern partition
int positionInstance(int handle, Instance** out) {
    if (mi355::isShardedHandle(handle)) return BEAGLE_ERROR_NO_IMPLEMENTATION;
    GET_INSTANCE(handle);
    if (in->S != 4 || in->partitionCount > 1) return BEAGLE_ERROR_NO_IMPLEMENTATION;
    DEMOTE_FOLDED_TIPS(in);
    *out = in;
    return 0;
}

}  // namespace

// Conditional robust counts (include/beagle_mi355.h beagleMi355RobustCounts; what CodonPartitionedRobustCounting.computeAllExpectedCounts
// computes from three getStatesForNode read-backs and a MarkovJumpsCore table per branch and labelling,
// CodonPartitionedRobustCounting.java:216-307).  The three draws are drawAncestral's, left on the device, instance 0's on its own
// stream behind nothing, the other two on their streams with an event each in front of the gather; then kernels_robustcounts.hip on
// instance 0's stream: the registers' M_k, the tables of every (register, row), the per-site gather (in row chunks of at most
// 256 MiB of outCounts when it is asked for), the per-row totals.
static int robustCounts(Instance* const* ins, const int* nodes, int nodeCount, const int* wIdx, const int* fIdx,
                        const unsigned long long* seeds, int flags, const double* branchLengths, const double* U, const double* Ui,
                        const double* lam, const double* Q, const double* registers, int K, const unsigned char* includeRows,
                        unsigned char* outStates, double* outCounts, double* outSiteTotals, double* outBranchTotals,
                        double* outTables) {
    Instance* in = ins[0];
    const int P = in->P;
    const size_t R = (size_t)nodeCount, blocks = (size_t)mi355::jumpSiteBlocks(P);
    AncestralDraw d[3];
    DrawEvents events;
    for (int q = 0; q < 3; q++) {
        HIP_TRY(hipSetDevice(ins[q]->device));
        int rc = drawAncestral(ins[q], nodes + (size_t)q * R * 3, nodeCount, wIdx[q], fIdx[q], seeds[q], flags, P, 0, &d[q]);
        if (rc) return rc;
        if (q > 0) {
            HIP_TRY(hipEventCreateWithFlags(&events.ev[q - 1], hipEventDisableTiming));
            HIP_TRY(hipEventRecord(events.ev[q - 1], live(ins[q])));
        }
    }
    const size_t stageRows = outCounts ? std::max<size_t>(1, std::min<size_t>(R, (256ull << 20) / ((size_t)K * P * sizeof(double)))) : 0;
    // robustDev (doubles): U, U^-1, lambda [2 * 4096 + 64] | Q [4096] | registers [K][4096] | rateReg, tmp, M [3][K][4096]
    //                      | cond [K][R][4096] | blockPartials [blocks][K][R] | branchTotals [K][R] | siteTotals [K][P]
    //                      | outCounts stage [K][stageRows][P] | rows [R] | error word
    const size_t nEig = 2 * (size_t)SS64 + mi355::ROBUST_STATES, nReg = (size_t)K * SS64, nCond = (size_t)K * R * SS64,
                 nPart = blocks * K * R, nRow = (size_t)K * R, nSite = (size_t)K * P, nStage = (size_t)K * stageRows * P;
    const size_t doubles = nEig + SS64 + 4 * nReg + nCond + nPart + nRow + nSite + nStage;
    int rc = growDevice(in, in->robustDev, doubles * sizeof(double) + R * sizeof(mi355::RobustRow) + sizeof(unsigned),
                        doubles * sizeof(double) + R * sizeof(mi355::RobustRow) + sizeof(unsigned), Grow::SyncIfHeld);
    if (rc) return rc;
    double* dEig = in->robustDev.as<double>();
    double* dQ = dEig + nEig;
    double* dReg = dQ + SS64;
    double* dRateReg = dReg + nReg;
    double* dTmp = dRateReg + nReg;
    double* dM = dTmp + nReg;
    double* dCond = dM + nReg;
    double* dPart = dCond + nCond;
    double* dRow = dPart + nPart;
    double* dSite = dRow + nRow;
    double* dStage = dSite + nSite;
    mi355::RobustRow* dRows = (mi355::RobustRow*)(dStage + nStage);
    unsigned* dErr = (unsigned*)(dRows + R);
    rc = upload(in, dEig, U, SS64 * sizeof(double)); if (rc) return rc;
    rc = upload(in, dEig + SS64, Ui, SS64 * sizeof(double)); if (rc) return rc;
    rc = upload(in, dEig + 2 * SS64, lam, mi355::ROBUST_STATES * sizeof(double)); if (rc) return rc;
    rc = upload(in, dQ, Q, SS64 * sizeof(double)); if (rc) return rc;
    rc = upload(in, dReg, registers, nReg * sizeof(double)); if (rc) return rc;
    std::vector<mi355::RobustRow> rows(nodeCount);
    for (int r = 0; r < nodeCount; r++) {
        rows[r].tau = r == 0 ? 0.0 : branchLengths[r];
        rows[r].parent = r == 0 ? -1 : nodes[3 * r + 2];
        rows[r].include = r > 0 && (!includeRows || includeRows[r] != 0);
    }
    rc = upload(in, dRows, rows.data(), rows.size() * sizeof(mi355::RobustRow)); if (rc) return rc;
    HIP_TRY(hipMemsetAsync(dErr, 0, sizeof(unsigned), live(in)));
    for (int k = 0; k < K; k++) HIP_TRY(hipMemsetAsync(dCond + (size_t)k * R * SS64, 0, SS64 * sizeof(double), live(in)));      // row 0
    mi355::launchRobustRegisters(live(in), dEig, dQ, dReg, K, dRateReg, dTmp, dM);
    mi355::launchRobustTables(live(in), dRows, nodeCount, dEig, dM, K, dCond);
    HIP_TRY(hipGetLastError());
    for (int q = 0; q < 2; q++) HIP_TRY(hipStreamWaitEvent(live(in), events.ev[q], 0));
    const size_t chunk = outCounts ? stageRows : R;
    for (size_t r0 = 0; r0 < R; r0 += chunk) {
        const size_t r1 = std::min(R, r0 + chunk);
        mi355::launchRobustSites(live(in), dRows, nodeCount, (int)r0, (int)r1, d[0].states, d[1].states, d[2].states, dCond, K, P,
                                 outCounts ? dStage : nullptr, dSite, dPart, dErr);
        HIP_TRY(hipGetLastError());
        if (!outCounts) continue;
        for (int k = 0; k < K; k++)
            HIP_TRY(hipMemcpyAsync(outCounts + ((size_t)k * R + r0) * P, dStage + (size_t)k * (r1 - r0) * P, (r1 - r0) * P * sizeof(double),
                                   hipMemcpyDeviceToHost, live(in)));
        HIP_TRY(hipStreamSynchronize(live(in)));           // (the next chunk overwrites the stage)
    }
    if (outBranchTotals) {
        mi355::launchRobustTotals(live(in), dPart, (int)blocks, K, nodeCount, 1, dRow);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(outBranchTotals, dRow, nRow * sizeof(double), hipMemcpyDeviceToHost, live(in)));
    }
    if (outSiteTotals) HIP_TRY(hipMemcpyAsync(outSiteTotals, dSite, nSite * sizeof(double), hipMemcpyDeviceToHost, live(in)));
    if (outTables) HIP_TRY(hipMemcpyAsync(outTables, dCond, nCond * sizeof(double), hipMemcpyDeviceToHost, live(in)));
    unsigned err = 0, drawErr = 0;
    rc = download(in, &err, dErr, sizeof(unsigned)); if (rc) return rc;
    for (int q = 0; q < 3; q++) {
        unsigned e = 0;
        rc = copyAncestral(ins[q], d[q], nodeCount, P, 0, outStates ? outStates + (size_t)q * R * P : nullptr, nullptr, &e);
        if (rc) return rc;
        drawErr |= e;
    }
    return (err | drawErr) ? BEAGLE_ERROR_FLOATING_POINT : BEAGLE_SUCCESS;
}

// Unconditioned counts (include/beagle_mi355.h beagleMi355SimulateUnconditionedCounts): one launch per chunk of length rows (at most
// 256 MiB of staged values when outCounts is asked for), then the totals over the workgroups.
static int unconditionedCounts(Instance* in, int S, const double* Q, const double* freqs, const double* lengths, int L, int sites,
                               const double* registers, int K, unsigned long long seed, double* outCounts, double* outTotals) {
    const size_t SS = (size_t)S * S, blocks = (size_t)mi355::unconditionedBlocks(sites);
    const size_t stageRows = outCounts ? std::max<size_t>(1, std::min<size_t>(L, (256ull << 20) / ((size_t)K * sites * sizeof(double)))) : 0;
    // robustDev (doubles): Q [S][S] | frequencies [S] | lengths [L] | registers [K][S][S] | blockPartials [blocks][K][L]
    //                      | totals [K][L] | outCounts stage [K][stageRows][sites] | error word
    const size_t nReg = (size_t)K * SS, nPart = blocks * K * L, nTot = (size_t)K * L, nStage = (size_t)K * stageRows * sites;
    const size_t doubles = SS + S + L + nReg + nPart + nTot + nStage;
    int rc = growDevice(in, in->robustDev, doubles * sizeof(double) + sizeof(unsigned), doubles * sizeof(double) + sizeof(unsigned),
                        Grow::SyncIfHeld);
    if (rc) return rc;
    double* dQ = in->robustDev.as<double>();
    double* dFreq = dQ + SS;
    double* dLen = dFreq + S;
    double* dReg = dLen + L;
    double* dPart = dReg + nReg;
    double* dTot = dPart + nPart;
    double* dStage = dTot + nTot;
    unsigned* dErr = (unsigned*)(dStage + nStage);
    rc = upload(in, dQ, Q, SS * sizeof(double)); if (rc) return rc;
    rc = upload(in, dFreq, freqs, S * sizeof(double)); if (rc) return rc;
    rc = upload(in, dLen, lengths, (size_t)L * sizeof(double)); if (rc) return rc;
    rc = upload(in, dReg, registers, nReg * sizeof(double)); if (rc) return rc;
    HIP_TRY(hipMemsetAsync(dErr, 0, sizeof(unsigned), live(in)));
    const size_t chunk = outCounts ? stageRows : (size_t)L;
    for (size_t l0 = 0; l0 < (size_t)L; l0 += chunk) {
        const size_t l1 = std::min<size_t>(L, l0 + chunk);
        mi355::launchUnconditioned(live(in), dQ, dFreq, dLen, L, (int)l0, (int)l1, sites, dReg, K, S, seed, outCounts ? dStage : nullptr,
                                   dPart, dErr);
        HIP_TRY(hipGetLastError());
        if (!outCounts) continue;
        for (int k = 0; k < K; k++)
            HIP_TRY(hipMemcpyAsync(outCounts + ((size_t)k * L + l0) * sites, dStage + (size_t)k * (l1 - l0) * sites,
                                   (l1 - l0) * sites * sizeof(double), hipMemcpyDeviceToHost, live(in)));
        HIP_TRY(hipStreamSynchronize(live(in)));           // (the next chunk overwrites the stage)
    }
    if (outTotals) {
        mi355::launchRobustTotals(live(in), dPart, (int)blocks, K, L, 0, dTot);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(outTotals, dTot, nTot * sizeof(double), hipMemcpyDeviceToHost, live(in)));
    }
    unsigned err = 0;
    rc = download(in, &err, dErr, sizeof(unsigned)); if (rc) return rc;
    return err ? BEAGLE_ERROR_FLOATING_POINT : BEAGLE_SUCCESS;
}

extern "C" {

int beagleMi355RobustCounts(const int* instances, const int* nodes, int nodeCount, const int* categoryWeightsIndices,
                            const int* stateFrequenciesIndices, const unsigned long long* seeds, int flags, const double* branchLengths,
                            const double* eigenVectors, const double* inverseEigenVectors, const double* eigenValues,
                            const double* infinitesimalMatrix, const double* registers, int registerCount,
                            const unsigned char* includeRows, unsigned char* outStates, double* outCounts, double* outSiteTotals,
                            double* outBranchTotals, double* outTables) {
    if (!instances || !nodes || nodeCount < 1 || !categoryWeightsIndices || !stateFrequenciesIndices || !seeds || !branchLengths ||
        !eigenVectors || !inverseEigenVectors || !eigenValues || !infinitesimalMatrix || !registers)
        return BEAGLE_ERROR_OUT_OF_RANGE;
    if (registerCount < 1 || registerCount > mi355::MAX_JUMP_REGISTERS) return BEAGLE_ERROR_OUT_OF_RANGE;
    if (flags & ~BEAGLE_MI355_ANCESTRAL_MAP) return BEAGLE_ERROR_OUT_OF_RANGE;
    if (!outCounts && !outSiteTotals && !outBranchTotals && !outTables) return BEAGLE_ERROR_OUT_OF_RANGE;
    if (instances[0] == instances[1] || instances[0] == instances[2] || instances[1] == instances[2]) return BEAGLE_ERROR_OUT_OF_RANGE;
    for (int r = 0; r < nodeCount; r++) {
        const int parent = nodes[3 * r + 2];
        if (nodes[3 * ((size_t)nodeCount + r) + 2] != parent || nodes[3 * (2 * (size_t)nodeCount + r) + 2] != parent)
            return BEAGLE_ERROR_OUT_OF_RANGE;
    }
    Instance* ins[3] = {nullptr, nullptr, nullptr};
    for (int q = 0; q < 3; q++) {
        const int rc = positionInstance(instances[q], &ins[q]);
        if (rc) return rc;
    }
    if (ins[1]->P != ins[0]->P || ins[2]->P != ins[0]->P) return BEAGLE_ERROR_NO_IMPLEMENTATION;
    if (ins[1]->device != ins[0]->device || ins[2]->device != ins[0]->device) return BEAGLE_ERROR_NO_IMPLEMENTATION;
    return robustCounts(ins, nodes, nodeCount, categoryWeightsIndices, stateFrequenciesIndices, seeds, flags, branchLengths, eigenVectors,
                        inverseEigenVectors, eigenValues, infinitesimalMatrix, registers, registerCount, includeRows, outStates,
                        outCounts, outSiteTotals, outBranchTotals, outTables);
}

int beagleMi355SimulateUnconditionedCounts(int instance, int stateCount, const double* infinitesimalMatrix,
                                           const double* startFrequencies, const double* lengths, int lengthCount, int siteCount,
                                           const double* registers, int registerCount, unsigned long long seed, double* outCounts,
                                           double* outTotals) {
    if (!infinitesimalMatrix || !startFrequencies || !lengths || !registers) return BEAGLE_ERROR_OUT_OF_RANGE;
    if (stateCount < 2 || stateCount > mi355::ROBUST_STATES) return BEAGLE_ERROR_OUT_OF_RANGE;
    if (registerCount < 1 || registerCount > mi355::MAX_JUMP_REGISTERS) return BEAGLE_ERROR_OUT_OF_RANGE;
    if (lengthCount < 1 || siteCount < 1 || (!outCounts && !outTotals)) return BEAGLE_ERROR_OUT_OF_RANGE;
    for (int e = 0; e < stateCount * stateCount; e++)
        if (!std::isfinite(infinitesimalMatrix[e])) return BEAGLE_ERROR_OUT_OF_RANGE;
    for (int l = 0; l < lengthCount; l++)
        if (!std::isfinite(lengths[l]) || lengths[l] < 0.0) return BEAGLE_ERROR_OUT_OF_RANGE;
    if (mi355::isShardedHandle(instance)) return BEAGLE_ERROR_NO_IMPLEMENTATION;
    GET_INSTANCE(instance);
    return unconditionedCounts(in, stateCount, infinitesimalMatrix, startFrequencies, lengths, lengthCount, siteCount, registers,
                               registerCount, seed, outCounts, outTotals);
}

}  // extern "C"
