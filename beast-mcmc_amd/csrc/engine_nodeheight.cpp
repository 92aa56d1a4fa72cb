// engine_nodeheight.cpp — node-height gradients and diagonal Hessians in one call (include/beagle_mi355.h
// beagleMi355NodeHeightDerivatives; kernels_nodeheight.hip): argument checks, operand bookkeeping, one launch per chunk of nodes.
#include "engine_internal.h"

using namespace mi355::eng;

// What DiscreteTraitNodeHeightDelegate.getNodeDerivatives computes from a getPartials per post-order and per pre-order buffer and a
// getTransitionMatrix per branch (DiscreteTraitNodeHeightDelegate.java:63-200), from the partials where they are.  The caller's held-
// back pre-order list has run by now (GET_INSTANCE); unstored post-order operands are materialised by one walk, as for a read-back.
static int nodeHeightDerivatives(Instance* in, const int* nodes, const double* rates, int nodeCount, int wIdx, double* outFirst, double* outSecond) {
    if (in->partitionCount > 1 || in->S > 64 || in->basta) return BEAGLE_ERROR_NO_IMPLEMENTATION;
    if (badIndex(wIdx, in->eigenCount)) return BEAGLE_ERROR_OUT_OF_RANGE;
    ReadSet reads(in);
    for (int r = 0; r < nodeCount; r++) {
        const int* nd = nodes + (size_t)8 * r;
        const int pre = nd[0], dI = nd[7];
        if (badIndex(pre, in->partialsCount) || (dI != -1 && badIndex(dI, in->matrixCount))) return BEAGLE_ERROR_OUT_OF_RANGE;
        if (int bad = reads.pre(pre)) return bad;
        for (int w = 0; w < 2; w++) {
            const int post = nd[1 + 3 * w], mat = nd[2 + 3 * w], dmat = nd[3 + 3 * w];
            if (badIndex(post, in->partialsCount) || badIndex(mat, in->matrixCount) || badIndex(dmat, in->matrixCount)) return BEAGLE_ERROR_OUT_OF_RANGE;
            if (int bad = reads.post(post)) return bad;
        }
    }
    int rc = reads.materialize(); if (rc) return rc;
    const bool second = outSecond != nullptr, general = !(in->S == 4 && !in->tiled);
    const int nb = mi355::edgeBlocks(in->P);
    // nodes per chunk: the descriptors fit a quarter of the staging ring, the block sums 256 MiB, the general kernel's products 128 MiB
    size_t chunk = std::min<size_t>((size_t)nodeCount, (RING_BYTES / 4) / sizeof(mi355::NodeHeightJob));
    chunk = std::min(chunk, std::max<size_t>(1, ((size_t)256 << 20) / ((size_t)(nb + 1) * 2 * sizeof(double))));
    const size_t productDoubles = general ? mi355::nodeHeightProductDoubles(1, in->S, in->C) : 0;
    if (general) chunk = std::min(chunk, std::max<size_t>(1, ((size_t)128 << 20) / (productDoubles * sizeof(double))));
    rc = ensureEdgeScratch(in, chunk * (size_t)(nb + 1) * 2 * sizeof(double)); if (rc) return rc;
    double *dBlock = in->edgeScratch.as<double>(), *dSums = dBlock + chunk * nb * 2;
    ScopedDevice products(in);                                      // (the general kernel's; freed, behind a drained stream, wherever the call ends)
    if (general) { rc = products.alloc(chunk * productDoubles * sizeof(double)); if (rc) return rc; }
    double* const dProducts = products.as<double>();
    CallTimer timer(in);
    std::vector<mi355::NodeHeightJob> jobs;
    std::vector<double> sums;
    bool finite = true;
    int launches = 0;
    for (size_t b = 0; b < (size_t)nodeCount && !rc; b += chunk) {
        const size_t m = std::min(chunk, (size_t)nodeCount - b);
        jobs.assign(m, mi355::NodeHeightJob());
        for (size_t e = 0; e < m; e++) {
            const int* nd = nodes + 8 * (b + e);
            const double* rt = rates + 3 * (b + e);
            mi355::NodeHeightJob& jb = jobs[e];
            memset(&jb, 0, sizeof(jb));
            jb.pre = preOperand(in, nd[0]);
            jb.postJ = postOperand(in, nd[1], &jb.statesJ); jb.postK = postOperand(in, nd[4], &jb.statesK);
            if (!jb.pre || !jb.postJ || !jb.postK) { rc = BEAGLE_ERROR_OUT_OF_RANGE; break; }
            jb.matJ = nd[2]; jb.dJ = nd[3]; jb.matK = nd[5]; jb.dK = nd[6]; jb.dI = nd[7];
            jb.slot = (int)e;
            jb.rJ = rt[0]; jb.rK = rt[1]; jb.rI = nd[7] < 0 ? 0.0 : rt[2];
        }
        if (rc) break;
        void* dJobs = nullptr;
        rc = uploadTransient(in, jobs.data(), m * sizeof(mi355::NodeHeightJob), &dJobs); if (rc) break;
        rc = timer.start(); if (rc) break;
        const double* weights = in->weights + (size_t)wIdx * in->C;
        if (!general)
            mi355::launchNodeHeight4(live(in), (const mi355::NodeHeightJob*)dJobs, (int)m, in->matrices, weights, in->patternWeights, dBlock, in->P, in->C, second);
        else if (!mi355::launchNodeHeight(live(in), (const mi355::NodeHeightJob*)dJobs, (int)m, in->matrices, dProducts, weights, in->patternWeights, dBlock,
                                          in->P, in->S, in->C, in->tiled, second)) { rc = BEAGLE_ERROR_GENERAL; break; }
        mi355::launchEdgeFinal(live(in), dBlock, (int)m, in->P, dSums);
        launches += general ? (second ? 4 : 3) : 2;
        if (b + m >= (size_t)nodeCount) { rc = timer.stop(launches); if (rc) break; }
        sums.resize(m * 2);
        rc = download(in, sums.data(), dSums, sums.size() * sizeof(double)); if (rc) break;
        for (size_t e = 0; e < m; e++) {
            if (outFirst) { outFirst[b + e] = sums[2 * e]; finite = finite && std::isfinite(sums[2 * e]); }
            if (outSecond) { outSecond[b + e] = sums[2 * e + 1]; finite = finite && std::isfinite(sums[2 * e + 1]); }
        }
    }
    products.reset();
    if (rc) return rc;
    if (hipGetLastError() != hipSuccess) return BEAGLE_ERROR_GENERAL;
    return finite ? BEAGLE_SUCCESS : BEAGLE_ERROR_FLOATING_POINT;
}

extern "C" {

int beagleMi355NodeHeightDerivatives(int instance, const int* nodes, const double* rates, int nodeCount, int categoryWeightsIndex,
                                     double* outFirst, double* outSecond) {
    if (!nodes || !rates || nodeCount < 1 || (!outFirst && !outSecond)) return BEAGLE_ERROR_OUT_OF_RANGE;
    if (mi355::isShardedHandle(instance)) {
        // every shard sums over its own pattern range; a shard whose sums are not finite still hands them over
        std::vector<double> tot((size_t)2 * nodeCount, 0.0);
        const int rc = mi355::shardedSumDoubles(instance, 2 * nodeCount, [&](int h, double* out) {
            const int r = beagleMi355NodeHeightDerivatives(h, nodes, rates, nodeCount, categoryWeightsIndex, outFirst ? out : nullptr,
                                                           outSecond ? out + nodeCount : nullptr);
            return r == BEAGLE_ERROR_FLOATING_POINT ? BEAGLE_SUCCESS : r; }, tot.data());
        if (rc) return rc;
        bool finite = true;
        for (int e = 0; e < nodeCount; e++) {
            if (outFirst) { outFirst[e] = tot[e]; finite = finite && std::isfinite(tot[e]); }
            if (outSecond) { outSecond[e] = tot[(size_t)nodeCount + e]; finite = finite && std::isfinite(tot[(size_t)nodeCount + e]); }
        }
        return finite ? BEAGLE_SUCCESS : BEAGLE_ERROR_FLOATING_POINT;
    }
    GET_INSTANCE(instance);
    DEMOTE_FOLDED_TIPS(in);                     // (tips' partials are read as data: engine_tipemission.cpp)
    return nodeHeightDerivatives(in, nodes, rates, nodeCount, categoryWeightsIndex, outFirst, outSecond);
}

}  // extern "C"
