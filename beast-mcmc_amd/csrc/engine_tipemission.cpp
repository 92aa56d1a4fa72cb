// engine_tipemission.cpp — tip error models (SequenceErrorModel, HypermutantErrorModel, ambiguity codes): the partials of such a tip are a
// lookup, E[code][state] with a handful of codes, not per-pattern data.  A tip branch then contributes
//     sum_j P[i][j] E[code_p][j] = (P E^T)[i][code_p]
// so with K <= S codes the tip IS a compact tip whose branch matrix is P E^T ("folded"): runOperations' pre-pass (foldTipOperations)
// points every operation on such a tip at a shadow matrix slot and one launch of k_foldTipEmission writes the shadows in front of the
// list — on every call, a replay of a cached plan included, because the matrix or the table may have changed since.  Everything behind
// the pre-pass sees an ordinary compact tip.  With K > S, when a list shares a matrix index between a folded tip and another child, and for
// every caller that reads a tip's partials as data (pre-order, gradients, samplers, getPartials) the lookup is written out as a partials
// buffer by k_expandTipEmission ("expanded": what beagleSetTipPartials leaves behind, without its upload).  See engine_internal.h.
#include "engine_internal.h"

using namespace mi355::eng;

namespace mi355 {
namespace eng {

// the first emission of an instance: the matrix block grows by the shadow slots (behind every slot it had, so no index moves)
static int enableEmissions(Instance* in) {
    const size_t per = (size_t)in->C * in->S * in->S, oldSlots = matrixSlotLayout(in);
    in->emis = new TipEmissions();
    in->emis->tips.resize((size_t)in->tipCount);
    in->emis->useOf.assign((size_t)std::max(1, in->matrixCount), -1);
    in->emis->useStamp.assign((size_t)std::max(1, in->matrixCount), 0);
    const size_t slots = matrixSlotLayout(in);
    double* grown = nullptr;
    int rc = devAlloc(in, (void**)&grown, slots * per * sizeof(double));
    if (rc) { delete in->emis; in->emis = nullptr; matrixSlotLayout(in); return rc; }
    HIP_TRY(hipMemsetAsync(grown + oldSlots * per, 0, (slots - oldSlots) * per * sizeof(double), live(in)));
    HIP_TRY(hipMemcpyAsync(grown, in->matrices, oldSlots * per * sizeof(double), hipMemcpyDeviceToDevice, live(in)));
    in->matrices = grown;                                  // (the old block stays owned by the instance until it is destroyed)
    in->resolveEpoch++;                                    // kept device programs hold addresses inside the old block
    return 0;
}

void freeTipEmissions(Instance* in) { delete in->emis; in->emis = nullptr; }

void dropTipEmission(Instance* in, int tip) {
    if (!in->emis || badIndex(tip, in->tipCount)) return;
    TipEmission& t = in->emis->tips[(size_t)tip];
    if (t.K == 0) return;
    if (t.folded) in->emis->foldedCount--; else in->emis->expandedCount--;
    t.K = 0; t.folded = false;
    t.codes.clear(); t.codes.shrink_to_fit(); t.table.clear();
}

static int uploadTable(Instance* in, TipEmission& t) {
    const size_t n = (size_t)t.K * in->S;
    int rc = growDevice(in, t.dTable, n * sizeof(double), n * sizeof(double), Grow::KeepOld); if (rc) return rc;
    return upload(in, t.dTable.p, t.table.data(), n * sizeof(double));      // K S doubles through the pinned ring
}

// the tip's partials buffer from its codes and table: what beagleSetTipPartials leaves behind
static int expandTip(Instance* in, int tip) {
    TipEmission& t = in->emis->tips[(size_t)tip];
    in->scaleOfPartial[tip] = -1;
    int rc = materializeTipUsers(in, tip); if (rc) return rc;          // definitions made of what the tip was until now
    clearVirtual(in, tip);
    rc = ensurePartials(in, tip); if (rc) return rc;
    if (!t.dCodes) { rc = devAlloc(in, (void**)&t.dCodes, ((size_t)in->P + 255) & ~(size_t)255); if (rc) return rc; }
    if (!t.codesOnDevice) { rc = upload(in, t.dCodes, t.codes.data(), (size_t)in->P); if (rc) return rc; t.codesOnDevice = true; }
    mi355::launchExpandTipEmission(live(in), in->partials[tip], t.dCodes, t.dTable.as<double>(), t.K, in->P, in->S, in->C, in->tiled);
    HIP_TRY(hipGetLastError());
    in->tipStates[tip] = nullptr;                          // the buffer holds partials now (the state slab stays owned by the instance)
    setCompact(in, tip, false);
    setLeaf(in, tip);
    return 0;
}

int demoteFoldedTip(Instance* in, int tip) {
    if (!foldedTip(in, tip)) return 0;
    TipEmission& t = in->emis->tips[(size_t)tip];
    t.folded = false;
    in->emis->foldedCount--; in->emis->expandedCount++; in->emis->demotions++;
    return expandTip(in, tip);
}

int demoteFoldedTips(Instance* in) {
    if (!in->emis || in->emis->foldedCount == 0) return 0;
    for (int tip = 0; tip < in->tipCount; tip++) { const int rc = demoteFoldedTip(in, tip); if (rc) return rc; }
    return 0;
}

// One pass over the list: a child that is a folded tip gets the shadow of its matrix index, and (source matrix, tip, shadow) becomes a
// job of the fold launch.  A matrix index that the list uses for two different folded tips, or for a folded tip and any other child,
// cannot have one shadow: the tips involved are demoted and the pass starts over (not what BEAST sends).
int foldTipOperations(Instance* in, const int** opsInOut, int count, int tuple) {
    TipEmissions& E = *in->emis;
    if (count <= 0 || !*opsInOut) return 0;
    const int* ops = *opsInOut;
    for (int k = 0; k < count; k++) {                      // a tip index written by the list holds the list's result from now on
        const int dest = ops[(size_t)k * tuple];
        if (dest >= 0 && dest < in->tipCount && E.tips[(size_t)dest].K) dropTipEmission(in, dest);
    }
    if (E.foldedCount == 0) return 0;
    const int OTHER = -2;
    for (;;) {
        const long stamp = ++E.stamp;
        bool conflict = false, any = false;
        E.jobs.clear();
        for (int k = 0; k < count; k++) {
            const int* op = ops + (size_t)k * tuple;
            for (int w = 0; w < 2; w++) {
                const int c = op[3 + 2 * w], m = op[4 + 2 * w];
                if (badIndex(m, in->matrixCount)) continue;                  // (reported by the path that runs the list)
                const int user = foldedTip(in, c) ? c : OTHER;
                any = any || user != OTHER;
                if (E.useStamp[(size_t)m] != stamp) {
                    E.useStamp[(size_t)m] = stamp; E.useOf[(size_t)m] = user;
                    if (user != OTHER) {
                        const TipEmission& t = E.tips[(size_t)c];
                        E.jobs.push_back(mi355::TipFoldJob{m, E.shadowBase + m, t.K, 0, t.dTable.as<double>()});
                    }
                } else if (E.useOf[(size_t)m] != user) { E.useOf[(size_t)m] = -3; conflict = true; }
            }
        }
        if (!any) return 0;
        if (!conflict) break;
        for (int k = 0; k < count; k++) {
            const int* op = ops + (size_t)k * tuple;
            for (int w = 0; w < 2; w++) {
                const int c = op[3 + 2 * w], m = op[4 + 2 * w];
                if (badIndex(m, in->matrixCount) || E.useOf[(size_t)m] != -3 || !foldedTip(in, c)) continue;
                const int rc = demoteFoldedTip(in, c); if (rc) return rc;
            }
        }
    }
    E.ops.assign(ops, ops + (size_t)count * tuple);
    for (int k = 0; k < count; k++) {
        int* op = E.ops.data() + (size_t)k * tuple;
        if (foldedTip(in, op[3]) && !badIndex(op[4], in->matrixCount)) op[4] += E.shadowBase;
        if (foldedTip(in, op[5]) && !badIndex(op[6], in->matrixCount)) op[6] += E.shadowBase;
    }
    void* dJobs = nullptr;
    int rc = uploadTransient(in, E.jobs.data(), E.jobs.size() * sizeof(mi355::TipFoldJob), &dJobs); if (rc) return rc;
    mi355::launchFoldTipEmission(live(in), in->matrices, (const mi355::TipFoldJob*)dJobs, (int)E.jobs.size(), in->S, in->C);
    HIP_TRY(hipGetLastError());
    E.foldLaunches++;
    *opsInOut = E.ops.data();
    return 0;
}

}  // namespace eng
}  // namespace mi355

extern "C" {

int beagleMi355SetTipEmission(int instance, int tipIndex, const int* codes, int codeCount, const double* emission) {
    if (mi355::isShardedHandle(instance)) {
        if (codeCount < 1 || codeCount > 255 || !emission) return BEAGLE_ERROR_OUT_OF_RANGE;
        // codes split by pattern like tip states, the table to every shard
        if (codes) return mi355::shardedSetPerPatternInts(instance, codes, [&](int h, const int* v) { return beagleMi355SetTipEmission(h, tipIndex, v, codeCount, emission); });
        return mi355::shardedBroadcast(instance, [&](int h) { return beagleMi355SetTipEmission(h, tipIndex, nullptr, codeCount, emission); });
    }
    GET_INSTANCE(instance);
    if (in->basta) return BEAGLE_ERROR_NO_IMPLEMENTATION;
    if (codeCount < 1 || codeCount > 255 || !emission || badIndex(tipIndex, in->tipCount) || badIndex(tipIndex, in->partialsCount) ||
        tipIndex >= in->compactCount) return BEAGLE_ERROR_OUT_OF_RANGE;
    if (!codes && (!in->emis || in->emis->tips[(size_t)tipIndex].K == 0)) return BEAGLE_ERROR_OUT_OF_RANGE;      // no codes to keep
    if (!in->emis) { const int rce = enableEmissions(in); if (rce) return rce; }
    TipEmissions& E = *in->emis;
    TipEmission& t = E.tips[(size_t)tipIndex];
    const int S = in->S;
    if (!codes) {
        // the per-proposal call: a new table for the codes the tip has (so one of the size they were given with).  A folded tip needs
        // nothing else (the next list refolds); an expanded one is written out again.
        if (codeCount != t.K) return BEAGLE_ERROR_OUT_OF_RANGE;
        t.table.assign(emission, emission + (size_t)codeCount * S);
        int rc = uploadTable(in, t); if (rc) return rc;
        return t.folded ? 0 : expandTip(in, tipIndex);
    }
    // the record as it will be: codes outside the table are 255 ("missing": all ones, a factor of one)
    std::vector<uint8_t> c8((size_t)in->P);
    for (int p = 0; p < in->P; p++) c8[(size_t)p] = codes[p] >= 0 && codes[p] < codeCount ? (uint8_t)codes[p] : (uint8_t)255;
    const bool fold = codeCount <= S;
    if (fold) {
        // route 1: what beagleSetTipStates does, on the codes (it drops whatever emission the tip had)
        std::vector<int> states((size_t)in->P);
        for (int p = 0; p < in->P; p++) states[(size_t)p] = c8[(size_t)p] == 255 ? S : (int)c8[(size_t)p];
        const int rcs = beagleSetTipStates(instance, tipIndex, states.data()); if (rcs) return rcs;
    } else dropTipEmission(in, tipIndex);
    t.K = codeCount; t.table.assign(emission, emission + (size_t)codeCount * S);
    t.codes.swap(c8); t.codesOnDevice = false; t.folded = fold;
    if (fold) E.foldedCount++; else E.expandedCount++;
    int rc = uploadTable(in, t); if (rc) return rc;
    return fold ? 0 : expandTip(in, tipIndex);
}

int beagleMi355TipEmissionStats(int instance, long* out4) {
    if (mi355::isShardedHandle(instance)) { return mi355::shardedFirst(instance, [&](int h) { return beagleMi355TipEmissionStats(h, out4); }); }
    GET_INSTANCE_KEEP_PENDING(instance);
    if (!out4) return BEAGLE_ERROR_OUT_OF_RANGE;
    out4[0] = out4[1] = out4[2] = out4[3] = 0;
    if (in->emis) { out4[0] = in->emis->foldedCount; out4[1] = in->emis->expandedCount; out4[2] = in->emis->foldLaunches; out4[3] = in->emis->demotions; }
    return BEAGLE_SUCCESS;
}

}  // extern "C"
