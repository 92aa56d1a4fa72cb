// engine_robustcounts.cpp — codon robust counting: the conditional counts of the 64-state product chain over three instances'
// ancestral draws in one call, and the unconditioned count simulation; argument checks and the launches.
#include "engine_internal.h"

using namespace mi355::eng;
namespace scratch = mi355::scratch;

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
    const size_t stageRows = outCounts ? stageRowCount(R, K, P) : 0;
    const scratch::RobustLayout L(mi355::ROBUST_STATES, P, K, R, blocks, stageRows, sizeof(mi355::RobustRow));
    int rc = growScratch(in, in->robustDev, L.bytes()); if (rc) return rc;
    char* base = in->robustDev.p;
    double *dEig = L.eig.at(base), *dQ = L.Q.at(base), *dReg = L.reg.at(base), *dM = L.M.at(base), *dCond = L.cond.at(base),
           *dPart = L.part.at(base), *dRow = L.row.at(base), *dSite = L.site.at(base), *dStage = L.stage.at(base);      // (dStage: NULL without outCounts)
    mi355::RobustRow* dRows = L.rows.as<mi355::RobustRow>(base);
    unsigned* dErr = L.error.at(base);
    rc = upload(in, dEig, U, SS64 * sizeof(double)); if (rc) return rc;
    rc = upload(in, dEig + SS64, Ui, SS64 * sizeof(double)); if (rc) return rc;
    rc = upload(in, dEig + 2 * SS64, lam, mi355::ROBUST_STATES * sizeof(double)); if (rc) return rc;
    rc = upload(in, dQ, Q, SS64 * sizeof(double)); if (rc) return rc;
    rc = upload(in, dReg, registers, L.reg.bytes()); if (rc) return rc;
    std::vector<mi355::RobustRow> rows(nodeCount);
    for (int r = 0; r < nodeCount; r++) {
        rows[r].tau = r == 0 ? 0.0 : branchLengths[r];
        rows[r].parent = r == 0 ? -1 : nodes[3 * r + 2];
        rows[r].include = r > 0 && (!includeRows || includeRows[r] != 0);
    }
    rc = upload(in, dRows, rows.data(), rows.size() * sizeof(mi355::RobustRow)); if (rc) return rc;
    HIP_TRY(hipMemsetAsync(dErr, 0, sizeof(unsigned), live(in)));
    for (int k = 0; k < K; k++) HIP_TRY(hipMemsetAsync(dCond + (size_t)k * R * SS64, 0, SS64 * sizeof(double), live(in)));      // row 0
    mi355::launchRobustRegisters(live(in), dEig, dQ, dReg, K, L.rateReg.at(base), L.tmp.at(base), dM);
    mi355::launchRobustTables(live(in), dRows, nodeCount, dEig, dM, K, dCond);
    HIP_TRY(hipGetLastError());
    for (int q = 0; q < 2; q++) HIP_TRY(hipStreamWaitEvent(live(in), events.ev[q], 0));
    const size_t chunk = outCounts ? stageRows : R;
    for (size_t r0 = 0; r0 < R; r0 += chunk) {
        const size_t r1 = std::min(R, r0 + chunk);
        mi355::launchRobustSites(live(in), dRows, nodeCount, (int)r0, (int)r1, d[0].states, d[1].states, d[2].states, dCond, K, P,
                                 dStage, dSite, dPart, dErr);
        HIP_TRY(hipGetLastError());
        if (outCounts) { rc = copyStagedRows(in, dStage, r1 - r0, r0, r1, K, R, P, P, 0, outCounts); if (rc) return rc; }
    }
    if (outBranchTotals) {
        mi355::launchBlockTotals(live(in), dPart, (int)blocks, K, nodeCount, 1, dRow);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(outBranchTotals, dRow, L.row.bytes(), hipMemcpyDeviceToHost, live(in)));
    }
    if (outSiteTotals) HIP_TRY(hipMemcpyAsync(outSiteTotals, dSite, L.site.bytes(), hipMemcpyDeviceToHost, live(in)));
    if (outTables) HIP_TRY(hipMemcpyAsync(outTables, dCond, L.cond.bytes(), hipMemcpyDeviceToHost, live(in)));
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
    const size_t blocks = (size_t)mi355::unconditionedBlocks(sites);
    const size_t stageRows = outCounts ? stageRowCount(L, K, sites) : 0;
    const scratch::UnconditionedLayout Y(S, L, sites, K, blocks, stageRows);
    int rc = growScratch(in, in->robustDev, Y.bytes()); if (rc) return rc;
    char* base = in->robustDev.p;
    double *dQ = Y.Q.at(base), *dFreq = Y.freq.at(base), *dLen = Y.len.at(base), *dReg = Y.reg.at(base), *dPart = Y.part.at(base),
           *dTot = Y.tot.at(base), *dStage = Y.stage.at(base);              // (dStage: NULL without outCounts)
    unsigned* dErr = Y.error.at(base);
    rc = upload(in, dQ, Q, Y.Q.bytes()); if (rc) return rc;
    rc = upload(in, dFreq, freqs, Y.freq.bytes()); if (rc) return rc;
    rc = upload(in, dLen, lengths, Y.len.bytes()); if (rc) return rc;
    rc = upload(in, dReg, registers, Y.reg.bytes()); if (rc) return rc;
    HIP_TRY(hipMemsetAsync(dErr, 0, sizeof(unsigned), live(in)));
    const size_t chunk = outCounts ? stageRows : (size_t)L;
    for (size_t l0 = 0; l0 < (size_t)L; l0 += chunk) {
        const size_t l1 = std::min<size_t>(L, l0 + chunk);
        mi355::launchUnconditioned(live(in), dQ, dFreq, dLen, L, (int)l0, (int)l1, sites, dReg, K, S, seed, dStage, dPart, dErr);
        HIP_TRY(hipGetLastError());
        if (outCounts) { rc = copyStagedRows(in, dStage, l1 - l0, l0, l1, K, L, sites, sites, 0, outCounts); if (rc) return rc; }
    }
    if (outTotals) {
        mi355::launchBlockTotals(live(in), dPart, (int)blocks, K, L, 0, dTot);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(outTotals, dTot, Y.tot.bytes(), hipMemcpyDeviceToHost, live(in)));
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
