// engine_abi.cpp — the part of the C ABI of include/beagle_mi355.h through which a caller sets or enqueues something: pattern weights
// and partitions, tips, partials, the model arrays, transition matrices, updatePartials, the scale-factor calls, the pre-order entry
// points; and the two Beagle*Api tables.  Argument checks and buffer bookkeeping over the engine's internals (engine_internal.h, whose
// head says where the rest of the ABI lives).
#include "engine_internal.h"

using mi355::OpDesc;
using mi355::shardedStates;
using mi355::shardedCategories;
using namespace mi355::eng;

namespace {

// part < 0: the whole pattern range (every partition's)
int accumulate(Instance* in, const int* idx, int count, int cum, double sign, int part) {
    if (badIndex(cum, in->scaleCount) || (part >= 0 && badIndex(part, in->partitionCount))) return BEAGLE_ERROR_OUT_OF_RANGE;
    const int pStart = part < 0 ? 0 : in->partStart[part], pEnd = part < 0 ? in->P : in->partEnd[part];
    int rc = materializeScaleUsers(in, cum); if (rc) return rc;
    rc = ensureScale(in, cum); if (rc) return rc;
    if (in->scaleIsRaw[cum]) return BEAGLE_ERROR_OUT_OF_RANGE;
    // exactly the scale buffers the last write-mode walk wrote, none of them touched since: a few dozen slice products instead of a factor
    // per node (Instance::lastSums)
    if (in->walk && in->sliceSums && in->partitionCount == 1 && in->lastSums.valid && in->lastSums.epoch == in->scaleWriteEpoch &&
        count > 0 && count == in->lastSums.nWritten) {
        const long stamp = ++in->seenCounter;
        bool same = true;
        for (int k = 0; k < count && same; k++) {
            if (badIndex(idx[k], in->scaleCount)) return BEAGLE_ERROR_OUT_OF_RANGE;
            same = in->scaleGen[(size_t)idx[k]] == in->lastSums.gen && in->scaleSeen[(size_t)idx[k]] != stamp;
            in->scaleSeen[(size_t)idx[k]] = stamp;
        }
        if (same) {
            void* dRows = nullptr;
            rc = uploadTransient(in, in->lastSums.rows.data(), in->lastSums.rows.size() * sizeof(int), &dRows); if (rc) return rc;
            mi355::launchAccumulateSlices(live(in), in->scale[cum], in->sliceMant.as<double>(), in->sliceExp.as<int>(), (const int*)dRows, (int)in->lastSums.rows.size(), in->pairLen,
                                          in->dPairPos, sign, pStart, pEnd);
            in->statSliceAccum++;
            HIP_TRY(hipGetLastError());
            return 0;
        }
    }
    std::vector<const double*> srcs(count);
    std::vector<int> raw(count);
    for (int k = 0; k < count; k++) {
        if (badIndex(idx[k], in->scaleCount)) return BEAGLE_ERROR_OUT_OF_RANGE;
        rc = ensureScale(in, idx[k]); if (rc) return rc;
        srcs[k] = in->scale[idx[k]]; raw[k] = in->scaleIsRaw[idx[k]];
    }
    const int chunk = 4096;
    for (int b = 0; b < count; b += chunk) {
        const int n = std::min(chunk, count - b);
        void *dSrc = nullptr, *dRaw = nullptr;
        rc = uploadTransient(in, &srcs[b], (size_t)n * sizeof(double*), &dSrc); if (rc) return rc;
        rc = uploadTransient(in, &raw[b], (size_t)n * sizeof(int), &dRaw); if (rc) return rc;
        mi355::launchAccumulateScale(live(in), in->scale[cum], (const double* const*)dSrc, (const int*)dRaw, n, sign, pStart, pEnd);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

// result[k] = first[k] (x) second[k] for `count` checked triples of matrix indices, `launch` being the (x) — launchConvolveMatrices or
// launchAddMatrices.  A result may feed a later triple of the same call (epoch chains): the longest runs of independent triples get a
// launch each, in order.
int runTriples(Instance* in, const int* first, const int* second, const int* result, int count, decltype(&mi355::launchConvolveMatrices) launch) {
    int b = 0;
    while (b < count) {
        int e = b + 1;
        for (; e < count; e++) {
            bool dep = false;
            for (int k = b; k < e && !dep; k++)
                dep = result[k] == first[e] || result[k] == second[e] || result[k] == result[e] ||
                      first[k] == result[e] || second[k] == result[e];
            if (dep) break;
        }
        const int n = e - b;
        void *dF, *dS, *dR;
        int rc = uploadTransient(in, first + b, n * sizeof(int), &dF); if (rc) return rc;
        rc = uploadTransient(in, second + b, n * sizeof(int), &dS); if (rc) return rc;
        rc = uploadTransient(in, result + b, n * sizeof(int), &dR); if (rc) return rc;
        launch(live(in), in->matrices, (const int*)dF, (const int*)dS, (const int*)dR, n, in->S, in->C);
        b = e;
    }
    HIP_TRY(hipGetLastError());
    return BEAGLE_SUCCESS;
}

// API layout double[C][P][S]  <->  T32 layout double[C][tile][S][32] (kernels_mfma.hip); padded patterns are zero
void toTiled(const Instance* in, const double* api, double* tiled, int categories) {
    const size_t S = in->S, P = in->P, nt = in->ntile;
    std::fill(tiled, tiled + (size_t)categories * nt * S * 32, 0.0);
    for (int c = 0; c < categories; c++)
        for (size_t p = 0; p < P; p++) {
            const double* src = api + ((size_t)c * P + p) * S;
            double* dst = tiled + ((size_t)c * nt + p / 32) * S * 32 + p % 32;
            for (size_t j = 0; j < S; j++) dst[j * 32] = src[j];
        }
}

}  // namespace

extern "C" {

const char* beagleGetVersion(void) { return "4.0.0-mi355"; }

const char* beagleGetCitation(void) {
    return "MI355X-native tree-likelihood engine behind the beagle.Beagle surface (gfx950 HIP kernels).\n"
           "API after: Ayres et al. (2019) BEAGLE 3, Systematic Biology 68:1052-1061.";
}

BeagleResourceList* beagleGetResourceList(void) { return &resources()->rl; }

int beagleFinalizeInstance(int instance) {
    if (mi355::isShardedHandle(instance)) { return mi355::shardedFinalize(instance); }
    Instance* in = nullptr;
    {
        std::lock_guard<std::mutex> lock(g_mutex);
        if (instance < 0 || instance >= (int)g_instances.size() || !g_instances[instance]) return BEAGLE_ERROR_UNINITIALIZED_INSTANCE;
        in = g_instances[instance];
        g_instances[instance] = nullptr;
    }
    destroy(in);
    return BEAGLE_SUCCESS;
}

int beagleSetCPUThreadCount(int instance, int threadCount) {
    if (mi355::isShardedHandle(instance)) { return BEAGLE_SUCCESS; }
    (void)threadCount;
    return lookup(instance) ? BEAGLE_SUCCESS : BEAGLE_ERROR_UNINITIALIZED_INSTANCE;   // no-op on a GPU instance
}

int beagleSetPatternWeights(int instance, const double* w) {
    if (mi355::isShardedHandle(instance)) {
        return mi355::shardedSetPerPatternDoubles(instance, w, 1, 1, [&](int h, const double* v) { return beagleSetPatternWeights(h, v); });
    }
    GET_INSTANCE(instance);
    return upload(in, in->patternWeights, w, (size_t)in->P * sizeof(double));
}

int beagleSetPatternPartitions(int instance, int partitionCount, const int* partitions) {
    if (mi355::isShardedHandle(instance)) {
        return mi355::shardedSetPerPatternInts(instance, partitions,
                                               [&](int h, const int* v) { return beagleSetPatternPartitions(h, partitionCount, v); });
    }
    GET_INSTANCE(instance);
    if (partitionCount < 1) return BEAGLE_ERROR_OUT_OF_RANGE;
    for (int x = 0; x < in->partialsCount; x++) { int rcv = materializeVirtual(in, x); if (rcv) return rcv; }   // whole-range definitions
    // partitions are contiguous pattern ranges in concatenation order
    // (MultiPartitionDataLikelihoodDelegate.java:520-535); anything else is rejected
    std::vector<int> s(partitionCount, -1), e(partitionCount, -1);
    for (int p = 0; p < in->P; p++) {
        const int k = partitions[p];
        if (badIndex(k, partitionCount)) return BEAGLE_ERROR_OUT_OF_RANGE;
        if (s[k] < 0) s[k] = p;
        else if (e[k] != p) return BEAGLE_ERROR_NO_IMPLEMENTATION;   // not contiguous
        e[k] = p + 1;
    }
    for (int k = 0; k < partitionCount; k++) if (s[k] < 0) { s[k] = 0; e[k] = 0; }
    in->partitionCount = partitionCount; in->partStart = s; in->partEnd = e; in->resolveEpoch++;
    // (the T32 walk needs no layout change: a tile that straddles two partitions is walked once per partition, each walk storing
    // only its own patterns — kernels_mfma.hip k_walkT32 masks by the segment's range)
    // (every instance whose planner is in use: its tables are keyed by (buffer, partition) — the level kernels' cherry instances
    // too, although they define nothing while there are several partitions)
    if (in->walk || in->walkT || in->virt) in->planner.setPartitionCount(partitionCount);
    if (in->virt) {
        // definitions are kept per (buffer, partition): more snapshot slots behind the caller's matrices
        // (T32 instances keep an identity matrix and the transposed-matrix scratch of the two-pass pre-order path BEHIND the
        // snapshot slots — matrixSlotLayout, as at creation: they move with the block and the identity is sent again)
        const size_t per = (size_t)in->C * in->S * in->S, slots = matrixSlotLayout(in);
        double* grown = nullptr;
        int rcm = devAlloc(in, (void**)&grown, slots * per * sizeof(double)); if (rcm) return rcm;
        HIP_TRY(hipMemsetAsync(grown, 0, slots * per * sizeof(double), live(in)));
        HIP_TRY(hipMemcpyAsync(grown, in->matrices, (size_t)std::max(1, in->matrixCount) * per * sizeof(double), hipMemcpyDeviceToDevice, live(in)));
        in->matrices = grown;                              // (the old block stays owned by the instance until it is destroyed)
        if (in->tiled) { int rci = uploadIdentityMatrix(in); if (rci) return rci; }
    }
    if (in->walk) {
        // the pair-interleaved arrays follow the partitions (Instance::pairPos): what exists already — tips are uploaded before
        // this call, MultiPartitionDataLikelihoodDelegate.java:544-553 — moves to the new layout on the device
        forgetFolds(in);
        setPairLayout(in);
        in->sliceRows = 0; in->lastSums.valid = false;                    // (the per-slice factor products are [row][pairLen]: re-made at the new length on first use)
        if (!in->dPairPos) { int rc = devAlloc(in, (void**)&in->dPairPos, (size_t)in->P * sizeof(unsigned)); if (rc) return rc; }
        HIP_TRY(hipStreamSynchronize(live(in)));
        HIP_TRY(hipMemcpy(in->dPairPos, in->pairPos.data(), (size_t)in->P * sizeof(unsigned), hipMemcpyHostToDevice));
        in->stateSlabLeft = 0; in->scaleSlabLeft = 0;                      // new slabs: the element sizes changed
        std::vector<mi355::RelayoutJob> jobs;                              // every tip in one pair of launches
        for (int t = 0; t < in->partialsCount; t++) {
            uint8_t* old = in->tipStates[t];
            if (!old) continue;
            in->tipStates[t] = nullptr;
            int rc = ensureStates(in, t); if (rc) return rc;
            jobs.push_back({old, in->tipStates[t], in->tipStates[t] + in->statePairOff});
        }
        for (size_t b = 0; b < jobs.size(); b += 16384) {                  // (the job list goes through the staging ring)
            const size_t e = std::min(jobs.size(), b + 16384);
            void* dJobs = nullptr;
            int rc = uploadTransient(in, jobs.data() + b, (e - b) * sizeof(mi355::RelayoutJob), &dJobs); if (rc) return rc;
            mi355::launchRelayoutStatesBatch(live(in), (const mi355::RelayoutJob*)dJobs, (int)(e - b), in->dPairPos, in->P, (int)in->pairLen, in->S);
        }
        for (int k = 0; k < (int)in->scale.size(); k++) {
            double* old = in->scale[k];
            if (!old) continue;
            const char raw = in->scaleIsRaw[k];
            in->scale[k] = nullptr;
            int rc = ensureScale(in, k); if (rc) return rc;                // (zero-filled)
            in->scaleIsRaw[k] = raw;
            HIP_TRY(hipMemcpyAsync(in->scale[k], old, (size_t)in->P * sizeof(double), hipMemcpyDeviceToDevice, live(in)));
            if (raw) mi355::launchRecipFromFactors(live(in), in->scale[k], in->scale[k] + in->scaleStride, in->dPairPos, in->P);
        }
        in->dummyTips = nullptr; in->onesScale = nullptr;                  // re-made at their new sizes on first use
        HIP_TRY(hipGetLastError());
    }
    const size_t n = (size_t)in->partialsCount * partitionCount;
    in->wStamp.assign(n, 0); in->wLevel.assign(n, 0); in->rStamp.assign(n, 0); in->rLevel.assign(n, 0); in->wOp.assign(n, 0);
    in->stamp = 0;
    return BEAGLE_SUCCESS;
}

int beagleSetTipStates(int instance, int tipIndex, const int* inStates) {
    if (mi355::isShardedHandle(instance)) {
        return mi355::shardedSetPerPatternInts(instance, inStates, [&](int h, const int* v) { return beagleSetTipStates(h, tipIndex, v); });
    }
    GET_INSTANCE(instance);
    if (badIndex(tipIndex, in->tipCount) || badIndex(tipIndex, in->partialsCount) || tipIndex >= in->compactCount)
        return BEAGLE_ERROR_OUT_OF_RANGE;
    if (in->emis) dropTipEmission(in, tipIndex);                      // (beagleMi355SetTipEmission: the tip is the caller's again)
    int rc = materializeTipUsers(in, tipIndex); if (rc) return rc;   // virtual cherries defined by the OLD states
    rc = ensureStates(in, tipIndex); if (rc) return rc;
    setCompact(in, tipIndex, true);
    if (!in->walk) {
        std::vector<uint8_t> s(in->P);
        for (int p = 0; p < in->P; p++) s[p] = (inStates[p] >= 0 && inStates[p] < in->S) ? (uint8_t)inStates[p] : (uint8_t)in->S;
        return upload(in, in->tipStates[tipIndex], s.data(), (size_t)in->P);
    }
    // walk instances: plain states (pre-order kernels, getTipStates), then the pair-interleaved copy the walk reads; the
    // padding of the last block of 128 is "missing"
    std::vector<uint8_t> s(in->statePairOff + in->pairLen, (uint8_t)in->S);
    for (int p = 0; p < in->P; p++) {
        const uint8_t v = (inStates[p] >= 0 && inStates[p] < in->S) ? (uint8_t)inStates[p] : (uint8_t)in->S;
        s[p] = v; s[in->statePairOff + in->pairPos[p]] = v;
    }
    if (in->repeatsOn) {                               // the class indices are built from the states (engine_walk.cpp prepareRepeats)
        repeatsForget(in);
        in->hostTips[(size_t)tipIndex].assign(s.begin(), s.begin() + in->P);
        in->repeatIndex.setTip(tipIndex, in->hostTips[(size_t)tipIndex].data());
    }
    return upload(in, in->tipStates[tipIndex], s.data(), s.size());
}

int beagleGetTipStates(int instance, int tipIndex, int* outStates) {
    if (mi355::isShardedHandle(instance)) {
        return mi355::shardedGetPerPatternInts(instance, outStates, [&](int h, int* v) { return beagleGetTipStates(h, tipIndex, v); });
    }
    GET_INSTANCE(instance);
    if (badIndex(tipIndex, in->partialsCount)) return BEAGLE_ERROR_OUT_OF_RANGE;
    if (in->emis && tipIndex < in->tipCount && in->emis->tips[(size_t)tipIndex].K) {      // a tip with an emission table: its codes (one outside the table: K)
        const TipEmission& t = in->emis->tips[(size_t)tipIndex];
        for (int p = 0; p < in->P; p++) outStates[p] = t.codes[(size_t)p] == 255 ? t.K : (int)t.codes[(size_t)p];
        return BEAGLE_SUCCESS;
    }
    if (!in->tipStates[tipIndex]) return BEAGLE_ERROR_OUT_OF_RANGE;
    std::vector<uint8_t> s(in->P);
    int rc = download(in, s.data(), in->tipStates[tipIndex], (size_t)in->P); if (rc) return rc;
    for (int p = 0; p < in->P; p++) outStates[p] = s[p];
    return BEAGLE_SUCCESS;
}

int beagleSetTipPartials(int instance, int tipIndex, const double* inPartials) {
    if (mi355::isShardedHandle(instance)) {
        return mi355::shardedSetPerPatternDoubles(instance, inPartials, shardedStates(instance), 1,
                                                  [&](int h, const double* v) { return beagleSetTipPartials(h, tipIndex, v); });
    }
    GET_INSTANCE(instance);
    if (badIndex(tipIndex, in->partialsCount)) return BEAGLE_ERROR_OUT_OF_RANGE;
    if (in->emis) dropTipEmission(in, tipIndex);
    in->scaleOfPartial[tipIndex] = -1;                     // (caller's data: no scale factor of ours in it)
    int rc = materializeTipUsers(in, tipIndex); if (rc) return rc;
    clearVirtual(in, tipIndex);
    rc = ensurePartials(in, tipIndex); if (rc) return rc;
    const size_t n = (size_t)in->P * in->S * sizeof(double);
    if (in->tiled) {
        const size_t plane = (size_t)in->ntile * 32 * in->S;
        std::vector<double> t(plane * in->C);
        toTiled(in, inPartials, t.data(), 1);
        for (int c = 1; c < in->C; c++) memcpy(&t[plane * c], &t[0], plane * sizeof(double));
        rc = upload(in, in->partials[tipIndex], t.data(), t.size() * sizeof(double));
    } else if (in->C == 1) { rc = upload(in, in->partials[tipIndex], inPartials, n); }
    else {
        // upload one category plane to the LAST plane, replicate it into all planes on the device
        double* last = in->partials[tipIndex] + (size_t)(in->C - 1) * in->P * in->S;
        rc = upload(in, last, inPartials, n);
        if (!rc) mi355::launchReplicateCategories(live(in), last, in->partials[tipIndex], in->P, in->S, in->C - 1);
    }
    in->tipStates[tipIndex] = nullptr;   // the buffer now holds partials (slab memory stays owned by the instance)
    setCompact(in, tipIndex, false);
    setLeaf(in, tipIndex);               // ... that no operation computes: definitions may read them (planner.h leafPartials)
    return rc;
}

int beagleSetPartials(int instance, int bufferIndex, const double* inPartials) {
    if (mi355::isShardedHandle(instance)) {
        return mi355::shardedSetPerPatternDoubles(instance, inPartials, shardedStates(instance), shardedCategories(instance),
                                                  [&](int h, const double* v) { return beagleSetPartials(h, bufferIndex, v); });
    }
    GET_INSTANCE_KEEP_PENDING(instance);
    if (in->basta) return bastaSetPartials(in, bufferIndex, inPartials);      // (a BASTA instance's vectors: engine_basta.cpp)
    if (badIndex(bufferIndex, in->partialsCount)) return BEAGLE_ERROR_OUT_OF_RANGE;
    // (a held-back pre-order list has its own copy of its root's pre-order partial — the buffer the gradient delegates rewrite
    // before every list — and waits unless this is one of the other buffers it reads or writes)
    if (heldTouches(in, bufferIndex)) { int rcp = executeHeldPre(in); if (rcp) return rcp; }
    if (in->emis) dropTipEmission(in, bufferIndex);
    in->scaleOfPartial[bufferIndex] = -1;                  // (caller's data: no scale factor of ours in it)
    int rc = materializeTipUsers(in, bufferIndex); if (rc) return rc;
    clearVirtual(in, bufferIndex);
    rc = ensurePartials(in, bufferIndex); if (rc) return rc;
    in->tipStates[bufferIndex] = nullptr; setCompact(in, bufferIndex, false);
    setLeaf(in, bufferIndex);
    if (in->tiled) {
        std::vector<double> t((size_t)in->C * in->ntile * 32 * in->S);
        toTiled(in, inPartials, t.data(), in->C);
        return upload(in, in->partials[bufferIndex], t.data(), t.size() * sizeof(double));
    }
    return upload(in, in->partials[bufferIndex], inPartials, (size_t)in->C * in->P * in->S * sizeof(double));
}

// Small model arrays are re-sent by BEAST before every evaluation whether they changed or not (frequencies and category
// weights right before calculateRootLogLikelihoods, BeagleTreeLikelihood.java:1029-1030, i.e. behind the last pruning
// kernel in stream order): an identical value is not uploaded again.
static int uploadIfChanged(Instance* in, std::vector<double>& shadow, std::vector<char>& ok, int count, int idx, size_t n,
                           double* dst, const double* src) {
    if (shadow.empty()) { shadow.assign((size_t)count * n, 0.0); ok.assign(count, 0); }
    double* sh = &shadow[(size_t)idx * n];
    if (ok[idx] && memcmp(sh, src, n * sizeof(double)) == 0) return 0;
    memcpy(sh, src, n * sizeof(double));
    ok[idx] = 1;
    return upload(in, dst, src, n * sizeof(double));
}

int beagleSetEigenDecomposition(int instance, int eigenIndex, const double* U, const double* Uinv, const double* lambda) {
    if (mi355::isShardedHandle(instance)) {          // (queued: every shard's thread applies its copy; sharded.h shardedPost)
        const size_t S = (size_t)shardedStates(instance);
        std::vector<double> u(U, U + S * S), ui(Uinv, Uinv + S * S), lam(lambda, lambda + (mi355::shardedEigenComplex(instance) ? 2 : 1) * S);
        return mi355::shardedPost(instance, [=](int h) { return beagleSetEigenDecomposition(h, eigenIndex, u.data(), ui.data(), lam.data()); });
    }
    GET_INSTANCE(instance);
    if (badIndex(eigenIndex, in->eigenCount)) return BEAGLE_ERROR_OUT_OF_RANGE;
    const size_t S = in->S, nLambda = in->eigenComplex ? 2 * S : S, stride = 2 * S * S + nLambda;
    if (in->eigenComplex) {
        // imaginary parts come as adjacent conjugate pairs (b, -b) — ComplexSubstitutionModel.java:121-173 walks them that way, and
        // the kernel (transition_body.h iexpEntry) reads the row after a pair's first row: a lone or unmatched entry is refused here
        for (size_t k = 0; k < S; k++) {
            const double im = lambda[S + k];
            if (im == 0.0) continue;
            if (k + 1 >= S || lambda[S + k + 1] != -im) return BEAGLE_ERROR_OUT_OF_RANGE;
            k++;
        }
    }
    std::vector<double> pack(stride);
    memcpy(&pack[0], U, S * S * sizeof(double));
    memcpy(&pack[S * S], Uinv, S * S * sizeof(double));
    memcpy(&pack[2 * S * S], lambda, nLambda * sizeof(double));
    return uploadIfChanged(in, in->shEigen, in->okEigen, in->eigenCount, eigenIndex, stride, in->eigen + stride * eigenIndex, pack.data());
}

int beagleSetStateFrequencies(int instance, int idx, const double* f) {
    if (mi355::isShardedHandle(instance)) {
        std::vector<double> v(f, f + shardedStates(instance));
        return mi355::shardedPost(instance, [=](int h) { return beagleSetStateFrequencies(h, idx, v.data()); });
    }
    GET_INSTANCE(instance);
    if (badIndex(idx, in->eigenCount)) return BEAGLE_ERROR_OUT_OF_RANGE;
    KeepWalkHeld keep(in);                               // (the root's input, not the walk's: a held launch stays held)
    return uploadIfChanged(in, in->shFreqs, in->okFreqs, in->eigenCount, idx, in->S, in->freqs + (size_t)idx * in->S, f);
}

int beagleSetCategoryWeights(int instance, int idx, const double* w) {
    if (mi355::isShardedHandle(instance)) {
        std::vector<double> v(w, w + shardedCategories(instance));
        return mi355::shardedPost(instance, [=](int h) { return beagleSetCategoryWeights(h, idx, v.data()); });
    }
    GET_INSTANCE(instance);
    if (badIndex(idx, in->eigenCount)) return BEAGLE_ERROR_OUT_OF_RANGE;
    KeepWalkHeld keep(in);
    return uploadIfChanged(in, in->shWeights, in->okWeights, in->eigenCount, idx, in->C, in->weights + (size_t)idx * in->C, w);
}

int beagleSetCategoryRatesWithIndex(int instance, int idx, const double* r) {
    if (mi355::isShardedHandle(instance)) {
        std::vector<double> v(r, r + shardedCategories(instance));
        return mi355::shardedPost(instance, [=](int h) { return beagleSetCategoryRatesWithIndex(h, idx, v.data()); });
    }
    GET_INSTANCE(instance);
    if (badIndex(idx, in->eigenCount)) return BEAGLE_ERROR_OUT_OF_RANGE;
    return uploadIfChanged(in, in->shRates, in->okRates, in->eigenCount, idx, in->C, in->rates + (size_t)idx * in->C, r);
}

int beagleSetCategoryRates(int instance, const double* r) { return beagleSetCategoryRatesWithIndex(instance, 0, r); }

int beagleSetTransitionMatrix(int instance, int matrixIndex, const double* inMatrix, double paddedValue) {
    if (mi355::isShardedHandle(instance)) {
        return mi355::shardedBroadcast(instance, [&](int h) { return beagleSetTransitionMatrix(h, matrixIndex, inMatrix, paddedValue); });
    }
    (void)paddedValue;
    GET_INSTANCE_KEEP_PENDING(instance);
    if (badIndex(matrixIndex, in->matrixCount)) return BEAGLE_ERROR_OUT_OF_RANGE;
    // (setDifferentialMatrix arrives between updatePrePartials and calculateEdgeDifferentials: the held-back list stays held
    // unless this very matrix is one of its branch matrices)
    if (heldReadsMatrix(in, matrixIndex)) { int rcp = executeHeldPre(in); if (rcp) return rcp; }
    const size_t n = (size_t)in->C * in->S * in->S;
    return upload(in, in->matrices + n * matrixIndex, inMatrix, n * sizeof(double));
}

int beagleGetTransitionMatrix(int instance, int matrixIndex, double* outMatrix) {
    if (mi355::isShardedHandle(instance)) { return mi355::shardedFirst(instance, [&](int h) { return beagleGetTransitionMatrix(h, matrixIndex, outMatrix); }); }
    GET_INSTANCE(instance);
    if (badIndex(matrixIndex, in->matrixCount)) return BEAGLE_ERROR_OUT_OF_RANGE;
    const size_t n = (size_t)in->C * in->S * in->S;
    // a small matrix (4 states: 64 doubles with four categories) comes back through the polled result page, as a root sum does: callers that
    // read one per branch (ancestral states, Markov jumps: AncestralStateBeagleTreeLikelihood.java:414-542) paid a device-to-host copy and a
    // stream synchronisation each — 27 us a matrix
    if (outMatrix && n <= 480) return mi355::publishAndWait(instance, in->matrices + n * matrixIndex, (int)n, outMatrix);
    return download(in, outMatrix, in->matrices + n * matrixIndex, n * sizeof(double));
}

int beagleConvolveTransitionMatrices(int instance, const int* first, const int* second, const int* result, int count) {
    if (mi355::isShardedHandle(instance)) {
        return mi355::shardedBroadcast(instance, [&](int h) { return beagleConvolveTransitionMatrices(h, first, second, result, count); });
    }
    GET_INSTANCE(instance);
    if (count <= 0) return BEAGLE_SUCCESS;
    for (int k = 0; k < count; k++) {
        if (badIndex(first[k], in->matrixCount) || badIndex(second[k], in->matrixCount) || badIndex(result[k], in->matrixCount) ||
            result[k] == first[k] || result[k] == second[k]) return BEAGLE_ERROR_OUT_OF_RANGE;
    }
    return runTriples(in, first, second, result, count, mi355::launchConvolveMatrices);
}

// Which scale factor operation `op` (a tuple of `tuple` ints) divides its destination by (the pre-order walk needs it:
// Instance::scaleOfPartial), and that a scale buffer it writes has a new version.
static void noteScaleOfOp(Instance* in, const int* op, int tuple) {
    if (badIndex(op[0], in->partialsCount)) return;                    // (reported by runOperations)
    const int sIdx = op[1] != BEAGLE_OP_NONE ? op[1] : op[2];
    if (op[1] != BEAGLE_OP_NONE && !badIndex(op[1], in->scaleCount)) in->scaleVersion[op[1]]++;
    // (9-int tuples: with several partitions a buffer's pattern ranges may carry different factors: unknown to the walk, which is
    // single-partition anyway)
    const bool unknown = tuple == BEAGLE_PARTITION_OP_COUNT && in->partitionCount > 1;
    in->scaleOfPartial[op[0]] = unknown ? -2 : (sIdx != BEAGLE_OP_NONE && !badIndex(sIdx, in->scaleCount)) ? sIdx : -1;
    in->scaleVersionAtWrite[op[0]] = in->scaleOfPartial[op[0]] >= 0 ? in->scaleVersion[sIdx] : 0u;
}

static int transitionMatrices(Instance* in, const int* eigenIdx, int eigenScalar, const int* rateIdx,
                              const int* probIdx, const double* lens, int count) {
    if (count <= 0) return BEAGLE_SUCCESS;
    // range checks as minimum / maximum scans (they vectorise; a partitioned evaluation names 12 900 branches, and a loop with an early
    // return per branch cost more than the kernel it fed)
    auto outOfRange = [count](const int* v, int limit) {
        int lo = v[0], hi = v[0];
        for (int k = 1; k < count; k++) { lo = v[k] < lo ? v[k] : lo; hi = v[k] > hi ? v[k] : hi; }
        return lo < 0 || hi >= limit;
    };
    if (outOfRange(probIdx, in->matrixCount) || (eigenIdx ? outOfRange(eigenIdx, in->eigenCount) : badIndex(eigenScalar, in->eigenCount)) ||
        (rateIdx && outOfRange(rateIdx, in->eigenCount))) return BEAGLE_ERROR_OUT_OF_RANGE;
    // 4 states, one eigen system and one rate set (beagleUpdateTransitionMatrices — what every evaluation of a chain issues): the
    // branch lengths and matrix indices stay in the staging ring, which the device maps, and the kernel reads them — and an
    // eigen system / rate set whose upload is still queued — from there; the queued copies ride in the same launch
    // (kernels.hip k_transition4Fused).  One launch instead of a copy kernel and a transition kernel: 5 us of a 12 500-pattern
    // evaluation's 170 (profiles/r04_experiments.txt).
    // The queued copies would run side by side with the transition blocks and with each other, in no order: a queued copy INTO the
    // matrix block (beagleSetTransitionMatrix of a slot this call may rewrite: the later call has to win) or two queued copies whose
    // ranges overlap without being the same array are flushed first, in order, and the plain kernel takes this call.
    bool fusable = in->S == 4 && in->kernelUploads && in->fuseLaunches && !eigenIdx && !rateIdx && (size_t)count * 12 <= RING_BYTES / 4 &&
                   (int)in->pendingCopies.size() <= mi355::HOST_COPY_MAX;
    if (fusable) {
        const char* m0 = (const char*)in->matrices;
        const char* m1 = m0 + (size_t)std::max(1, in->matrixCount) * in->C * in->S * in->S * sizeof(double);
        const std::vector<Instance::PendingCopy>& pc = in->pendingCopies;
        for (size_t a = 0; a < pc.size() && fusable; a++) {
            const char* d0 = (const char*)pc[a].dst; const char* d1 = d0 + pc[a].bytes;
            if (d0 < m1 && m0 < d1) fusable = false;
            for (size_t b = a + 1; b < pc.size() && fusable; b++) {
                const char* e0 = (const char*)pc[b].dst; const char* e1 = e0 + pc[b].bytes;
                if (d0 < e1 && e0 < d1 && !(e0 <= d0 && d1 <= e1)) fusable = false;      // (an earlier copy fully covered by a later one is simply dropped below)
            }
        }
    }
    if (fusable) {
        const size_t lenBytes = (size_t)count * sizeof(double), idxBytes = (size_t)count * sizeof(int);
        const long off = stage(in, lens, lenBytes, lenBytes + idxBytes);
        if (off < 0) return BEAGLE_ERROR_GENERAL;
        memcpy(in->hRing + off + lenBytes, probIdx, idxBytes);
        const size_t eigStride = in->eigenComplex ? 40 : 36;
        const double* const eigDst = in->eigen + eigStride * eigenScalar;
        const double* eigSrc = eigDst;
        const double* ratesSrc = in->rates;                                   // (rate set 0)
        mi355::HostCopyList L;
        L.n = 0;
        unsigned blocks = 0;
        for (const Instance::PendingCopy& pc : in->pendingCopies) {
            mi355::HostCopyList::Entry& e = L.e[L.n++];
            e.dst = pc.dst; e.src = in->hRingDev + pc.ringOff; e.bytes = (unsigned)pc.bytes; e.firstBlock = blocks;
            blocks += (unsigned)((pc.bytes + 4095) / 4096);
            // (the LAST queued upload of an array is the one that counts: compared with where the array lives, not with what an
            // earlier queued upload of it has already redirected the source to)
            if (pc.dst == (void*)eigDst && pc.bytes == eigStride * sizeof(double)) eigSrc = (const double*)(in->hRingDev + pc.ringOff);
            if (pc.dst == (void*)in->rates && pc.bytes >= (size_t)in->C * sizeof(double)) ratesSrc = (const double*)(in->hRingDev + pc.ringOff);
        }
        // (an array queued twice: the copies run side by side — an earlier one that a later one covers entirely is dropped; any
        // other overlap was excluded above)
        for (int a = 0; a < L.n; a++)
            for (int b = a + 1; b < L.n; b++)
                if ((const char*)L.e[b].dst <= (const char*)L.e[a].dst &&
                    (const char*)L.e[a].dst + L.e[a].bytes <= (const char*)L.e[b].dst + L.e[b].bytes) L.e[a].bytes = 0;
        in->pendingCopies.clear();
        mi355::launchTransitionMatrices4Fused(in->stream, in->matrices, eigSrc, ratesSrc, (const int*)(in->hRingDev + off + lenBytes),
                                              (const double*)(in->hRingDev + off), count, in->C, in->eigenComplex, L, (int)blocks);
        HIP_TRY(hipGetLastError());
        return BEAGLE_SUCCESS;
    }
    // 4 states, several eigen systems or rate sets (beagleUpdateTransitionMatricesWithMultipleModels — what every evaluation of a
    // partitioned chain issues): lengths and the three index lists stay in the staging ring as above and k_transition4 reads them from
    // there; queued uploads (an eigen system, a rate set) go first, in their own launch — a chain's steady state has none.  One launch
    // instead of a copy kernel (the ring's 20 bytes per branch over PCIe: 9 us for config E's 12 900 branches) and a transition
    // kernel (5 us) behind it: the reads now overlap the arithmetic.
    if (in->S == 4 && in->kernelUploads && in->fuseLaunches && (size_t)count * 20 <= RING_BYTES / 4) {
        const size_t lenBytes = (size_t)count * sizeof(double), idxBytes = (size_t)count * sizeof(int);
        const long off = stage(in, lens, lenBytes, lenBytes + 3 * idxBytes);
        if (off < 0) return BEAGLE_ERROR_GENERAL;
        memcpy(in->hRing + off + lenBytes, probIdx, idxBytes);
        int* rEig = (int*)(in->hRing + off + lenBytes + idxBytes);
        int* rRate = rEig + count;
        if (eigenIdx) memcpy(rEig, eigenIdx, idxBytes); else std::fill(rEig, rEig + count, eigenScalar);
        if (rateIdx) memcpy(rRate, rateIdx, idxBytes); else std::fill(rRate, rRate + count, 0);
        const int* rIdx = (const int*)(in->hRingDev + off + lenBytes);
        mi355::launchTransitionMatrices(live(in), in->matrices, in->eigen, in->rates, rIdx, (const double*)(in->hRingDev + off),
                                        rIdx + count, rIdx + 2 * (size_t)count, count, in->S, in->C, in->eigenComplex);
        HIP_TRY(hipGetLastError());
        return BEAGLE_SUCCESS;
    }
    // one packed upload: [lengths double[count] | matrix idx | eigen idx | rate idx] (each copy is a blit kernel)
    std::vector<char> pack((size_t)count * (sizeof(double) + 3 * sizeof(int)));
    double* pLen = (double*)pack.data();
    int* pIdx = (int*)(pack.data() + (size_t)count * sizeof(double));
    memcpy(pLen, lens, (size_t)count * sizeof(double));
    memcpy(pIdx, probIdx, (size_t)count * sizeof(int));
    if (eigenIdx) memcpy(pIdx + count, eigenIdx, (size_t)count * sizeof(int)); else std::fill(pIdx + count, pIdx + 2 * (size_t)count, eigenScalar);
    if (rateIdx) memcpy(pIdx + 2 * (size_t)count, rateIdx, (size_t)count * sizeof(int)); else std::fill(pIdx + 2 * (size_t)count, pIdx + 3 * (size_t)count, 0);
    void* dPack;
    int rc = uploadTransient(in, pack.data(), pack.size(), &dPack); if (rc) return rc;
    const double* dLen = (const double*)dPack;
    const int* dIdx = (const int*)((const char*)dPack + (size_t)count * sizeof(double));
    mi355::launchTransitionMatrices(live(in), in->matrices, in->eigen, in->rates, dIdx, dLen,
                                    dIdx + count, dIdx + 2 * (size_t)count, count, in->S, in->C, in->eigenComplex);
    HIP_TRY(hipGetLastError());
    return BEAGLE_SUCCESS;
}

int beagleUpdateTransitionMatrices(int instance, int eigenIndex, const int* probabilityIndices,
                                   const int* firstDerivativeIndices, const int* secondDerivativeIndices,
                                   const double* edgeLengths, int count) {
    if (mi355::isShardedHandle(instance)) {
        if (firstDerivativeIndices || secondDerivativeIndices) return BEAGLE_ERROR_NO_IMPLEMENTATION;
        if (count <= 0) return BEAGLE_SUCCESS;
        std::vector<int> p(probabilityIndices, probabilityIndices + count); std::vector<double> t(edgeLengths, edgeLengths + count);
        return mi355::shardedPost(instance, [=](int h) { return beagleUpdateTransitionMatrices(h, eigenIndex, p.data(), nullptr, nullptr, t.data(), count); });
    }
    GET_INSTANCE_KEEP_PENDING(instance);                      // (a held-back pre-order list waits unless one of ITS matrices is rewritten)
    if (firstDerivativeIndices || secondDerivativeIndices) return BEAGLE_ERROR_NO_IMPLEMENTATION;
    if (in->heldPre.held && probabilityIndices)
        for (int k = 0; k < count; k++) if (heldReadsMatrix(in, probabilityIndices[k])) { int rcp = executeHeldPre(in); if (rcp) return rcp; break; }
    return transitionMatrices(in, nullptr, eigenIndex, nullptr, probabilityIndices, edgeLengths, count);
}

int beagleUpdateTransitionMatricesWithMultipleModels(int instance, const int* eigenIndices, const int* categoryRateIndices,
                                   const int* probabilityIndices, const int* firstDerivativeIndices,
                                   const int* secondDerivativeIndices, const double* edgeLengths, int count) {
    if (mi355::isShardedHandle(instance)) {
        if (firstDerivativeIndices || secondDerivativeIndices) return BEAGLE_ERROR_NO_IMPLEMENTATION;
        if (!eigenIndices || !categoryRateIndices) return BEAGLE_ERROR_OUT_OF_RANGE;
        if (count <= 0) return BEAGLE_SUCCESS;
        std::vector<int> e(eigenIndices, eigenIndices + count), r(categoryRateIndices, categoryRateIndices + count), p(probabilityIndices, probabilityIndices + count);
        std::vector<double> t(edgeLengths, edgeLengths + count);
        return mi355::shardedPost(instance, [=](int h) { return beagleUpdateTransitionMatricesWithMultipleModels(h, e.data(), r.data(), p.data(), nullptr, nullptr, t.data(), count); });
    }
    GET_INSTANCE(instance);
    if (firstDerivativeIndices || secondDerivativeIndices) return BEAGLE_ERROR_NO_IMPLEMENTATION;
    if (!eigenIndices || !categoryRateIndices) return BEAGLE_ERROR_OUT_OF_RANGE;
    return transitionMatrices(in, eigenIndices, 0, categoryRateIndices, probabilityIndices, edgeLengths, count);
}

int beagleUpdatePartials(int instance, const int* operations, int operationCount, int cumulativeScaleIndex) {
    if (mi355::isShardedHandle(instance)) {
        if (operationCount <= 0) return BEAGLE_SUCCESS;
        std::vector<int> ops(operations, operations + (size_t)operationCount * BEAGLE_OP_COUNT);
        return mi355::shardedPost(instance, [=](int h) { return beagleUpdatePartials(h, ops.data(), operationCount, cumulativeScaleIndex); });
    }
    GET_INSTANCE_KEEP_PENDING(instance);
    if (operations && (in->heldPre.held || in->trackScales))               // (only on instances that have been asked for a pre-order pass)
        for (int k = 0; k < operationCount; k++) {
            const int* op = operations + (size_t)k * BEAGLE_OP_COUNT;
            // (a held-back pre-order list waits unless this list overwrites what it reads or touches what it writes)
            if (heldTouches(in, op[0]) || heldWrites(in, op[3]) || heldWrites(in, op[5])) { int rcp = executeHeldPre(in); if (rcp) return rcp; }
            noteScaleOfOp(in, op, BEAGLE_OP_COUNT);
        }
    if (operations && operationCount > 0 && in->partitionCount > 1) {
        // a partitioned instance: a 7-int list covers every pattern — it runs as the same list of 9-int tuples, each operation once per
        // (non-empty) partition in a row, the cumulative index on every tuple (include/beagle_mi355.h)
        std::vector<int> ops9;
        ops9.reserve((size_t)operationCount * in->partitionCount * BEAGLE_PARTITION_OP_COUNT);
        for (int k = 0; k < operationCount; k++) {
            const int* op = operations + (size_t)k * BEAGLE_OP_COUNT;
            for (int part = 0; part < in->partitionCount; part++) {
                if (in->partEnd[part] <= in->partStart[part]) continue;
                ops9.insert(ops9.end(), op, op + BEAGLE_OP_COUNT);
                ops9.push_back(part); ops9.push_back(cumulativeScaleIndex);
            }
        }
        return runOperations(in, ops9.data(), (int)(ops9.size() / BEAGLE_PARTITION_OP_COUNT), BEAGLE_PARTITION_OP_COUNT, BEAGLE_OP_NONE);
    }
    return runOperations(in, operations, operationCount, BEAGLE_OP_COUNT, cumulativeScaleIndex);
}

int beagleUpdatePartialsByPartition(int instance, const int* operations, int operationCount) {
    if (mi355::isShardedHandle(instance)) {
        if (operationCount <= 0) return BEAGLE_SUCCESS;
        std::vector<int> ops(operations, operations + (size_t)operationCount * BEAGLE_PARTITION_OP_COUNT);
        return mi355::shardedPost(instance, [=](int h) { return beagleUpdatePartialsByPartition(h, ops.data(), operationCount); });
    }
    GET_INSTANCE(instance);
    if (operations && in->trackScales)                         // (Instance::scaleOfPartial, as beagleUpdatePartials keeps it)
        for (int k = 0; k < operationCount; k++) noteScaleOfOp(in, operations + (size_t)k * BEAGLE_PARTITION_OP_COUNT, BEAGLE_PARTITION_OP_COUNT);
    return runOperations(in, operations, operationCount, BEAGLE_PARTITION_OP_COUNT, BEAGLE_OP_NONE);
}

int beagleWaitForPartials(int instance, const int* destinationPartials, int count) {
    if (mi355::isShardedHandle(instance)) {
        return mi355::shardedBroadcast(instance, [&](int h) { return beagleWaitForPartials(h, destinationPartials, count); });
    }
    (void)destinationPartials; (void)count;
    GET_INSTANCE(instance);
    HIP_TRY(hipStreamSynchronize(live(in)));
    ringIdle(in);
    return BEAGLE_SUCCESS;
}

// accumulate (sign +1) / remove (-1) the listed factors into / from a cumulative buffer, over partition `part` (< 0: every pattern)
static int accumulateCall(int instance, const int* scaleIndices, int count, int cumulativeScaleIndex, double sign, int part) {
    if (mi355::isShardedHandle(instance)) {
        std::vector<int> v(scaleIndices, scaleIndices + std::max(0, count));
        return mi355::shardedPost(instance, [=](int h) { return accumulateCall(h, v.data(), count, cumulativeScaleIndex, sign, part); });
    }
    GET_INSTANCE_KEEP_PENDING(instance);          // (scale buffers only: nothing a held-back pre-order list reads or writes)
    if (!badIndex(cumulativeScaleIndex, in->scaleCount)) in->scaleVersion[cumulativeScaleIndex]++;
    return accumulate(in, scaleIndices, count, cumulativeScaleIndex, sign, part);
}
int beagleAccumulateScaleFactors(int instance, const int* scaleIndices, int count, int cumulativeScaleIndex) {
    return accumulateCall(instance, scaleIndices, count, cumulativeScaleIndex, 1.0, -1);
}
int beagleAccumulateScaleFactorsByPartition(int instance, const int* scaleIndices, int count, int cumulativeScaleIndex, int partitionIndex) {
    return accumulateCall(instance, scaleIndices, count, cumulativeScaleIndex, 1.0, partitionIndex);
}
int beagleRemoveScaleFactors(int instance, const int* scaleIndices, int count, int cumulativeScaleIndex) {
    return accumulateCall(instance, scaleIndices, count, cumulativeScaleIndex, -1.0, -1);
}
int beagleRemoveScaleFactorsByPartition(int instance, const int* scaleIndices, int count, int cumulativeScaleIndex, int partitionIndex) {
    return accumulateCall(instance, scaleIndices, count, cumulativeScaleIndex, -1.0, partitionIndex);
}

// zero a cumulative buffer over every pattern, or (byPartition) over the patterns of partition `part`
static int resetCall(int instance, int cumulativeScaleIndex, bool byPartition, int part) {
    if (mi355::isShardedHandle(instance)) { return mi355::shardedPost(instance, [=](int h) { return resetCall(h, cumulativeScaleIndex, byPartition, part); }); }
    GET_INSTANCE_KEEP_PENDING(instance);          // (scale buffers only: nothing a held-back pre-order list reads or writes)
    if (!badIndex(cumulativeScaleIndex, in->scaleCount)) in->scaleVersion[cumulativeScaleIndex]++;
    if (badIndex(cumulativeScaleIndex, in->scaleCount) || (byPartition && badIndex(part, in->partitionCount))) return BEAGLE_ERROR_OUT_OF_RANGE;
    int rc = materializeScaleUsers(in, cumulativeScaleIndex); if (rc) return rc;
    rc = ensureScale(in, cumulativeScaleIndex); if (rc) return rc;
    if (in->scaleIsRaw[cumulativeScaleIndex] && byPartition && in->partitionCount > 1) {
        // a per-node (raw) buffer is being recycled as a cumulative one: clear all of it first
        mi355::launchFill(live(in), in->scale[cumulativeScaleIndex], 0.0, 0, in->P);
    }
    if (in->scaleIsRaw[cumulativeScaleIndex]) { in->resolveEpoch++; scalesWritten(in); }    // kept programs were validated against the raw flags
    in->scaleIsRaw[cumulativeScaleIndex] = 0;
    mi355::launchFill(live(in), in->scale[cumulativeScaleIndex], 0.0, byPartition ? in->partStart[part] : 0, byPartition ? in->partEnd[part] : in->P);
    HIP_TRY(hipGetLastError());
    return BEAGLE_SUCCESS;
}
int beagleResetScaleFactorsByPartition(int instance, int cumulativeScaleIndex, int partitionIndex) {
    return resetCall(instance, cumulativeScaleIndex, true, partitionIndex);
}
int beagleResetScaleFactors(int instance, int cumulativeScaleIndex) { return resetCall(instance, cumulativeScaleIndex, false, 0); }

int beagleCopyScaleFactors(int instance, int dest, int src) {
    if (mi355::isShardedHandle(instance)) { return mi355::shardedPost(instance, [=](int h) { return beagleCopyScaleFactors(h, dest, src); }); }
    GET_INSTANCE_KEEP_PENDING(instance);
    if (!badIndex(dest, in->scaleCount)) in->scaleVersion[dest]++;
    if (badIndex(dest, in->scaleCount) || badIndex(src, in->scaleCount)) return BEAGLE_ERROR_OUT_OF_RANGE;
    int rc = materializeScaleUsers(in, dest); if (rc) return rc;
    rc = ensureScale(in, dest); if (rc) return rc;
    rc = ensureScale(in, src); if (rc) return rc;
    const size_t scaleDoubles = in->walk ? 2 * in->scaleStride : (size_t)in->P;      // walk instances: factors and reciprocals
    HIP_TRY(hipMemcpyAsync(in->scale[dest], in->scale[src], scaleDoubles * sizeof(double), hipMemcpyDeviceToDevice, live(in)));
    if (in->scaleIsRaw[dest] != in->scaleIsRaw[src]) in->resolveEpoch++;
    if (in->scaleIsRaw[dest] || in->scaleIsRaw[src]) scalesWritten(in);
    in->scaleIsRaw[dest] = in->scaleIsRaw[src];
    return BEAGLE_SUCCESS;
}

// ---- outside SURVEY 8 (a)-(e): exported so the JNI shim links ---------------------------------
// ---- pre-order partials and branch gradients ----
int beagleSetRootPrePartials(int instance, const int* bufferIndices, const int* stateFrequenciesIndices, int count) {
    if (mi355::isShardedHandle(instance)) {
        return mi355::shardedBroadcast(instance, [&](int h) { return beagleSetRootPrePartials(h, bufferIndices, stateFrequenciesIndices, count); });
    }
    GET_INSTANCE(instance);
    for (int k = 0; k < count; k++) {
        const int b = bufferIndices[k], f = stateFrequenciesIndices[k];
        if (badIndex(b, in->partialsCount) || badIndex(f, in->eigenCount)) return BEAGLE_ERROR_OUT_OF_RANGE;
        int rc = materializeTipUsers(in, b); if (rc) return rc;
        clearVirtual(in, b);
        rc = ensurePartials(in, b); if (rc) return rc;
        in->tipStates[b] = nullptr; setCompact(in, b, false);
        mi355::launchFillFrequencies(live(in), in->partials[b], in->freqs + (size_t)f * in->S, in->P, in->S, in->C, in->tiled);
    }
    HIP_TRY(hipGetLastError());
    return BEAGLE_SUCCESS;
}

int beagleSetDifferentialMatrix(int instance, int matrixIndex, const double* inMatrix) {
    return beagleSetTransitionMatrix(instance, matrixIndex, inMatrix, 0.0);
}

// result[k] = first[k] + second[k], entry by entry and category by category (declared by BeagleJNIWrapper next to
// convolveTransitionMatrices; no caller in BEAST today).  A result may feed a later triple of the same call: dependent triples in order.
int beagleAddTransitionMatrices(int instance, const int* first, const int* second, const int* result, int count) {
    if (mi355::isShardedHandle(instance)) {
        return mi355::shardedBroadcast(instance, [&](int h) { return beagleAddTransitionMatrices(h, first, second, result, count); });
    }
    GET_INSTANCE(instance);
    if (count <= 0) return BEAGLE_SUCCESS;
    if (!first || !second || !result) return BEAGLE_ERROR_OUT_OF_RANGE;
    for (int k = 0; k < count; k++)
        if (badIndex(first[k], in->matrixCount) || badIndex(second[k], in->matrixCount) || badIndex(result[k], in->matrixCount)) return BEAGLE_ERROR_OUT_OF_RANGE;
    return runTriples(in, first, second, result, count, mi355::launchAddMatrices);
}

int beagleTransposeTransitionMatrices(int instance, const int* inputIndices, const int* resultIndices, int matrixCount) {
    if (mi355::isShardedHandle(instance)) {
        return mi355::shardedBroadcast(instance,
                                       [&](int h) { return beagleTransposeTransitionMatrices(h, inputIndices, resultIndices, matrixCount); });
    }
    GET_INSTANCE(instance);
    if (matrixCount <= 0) return BEAGLE_SUCCESS;
    std::vector<int> pairs((size_t)matrixCount * 2);
    for (int k = 0; k < matrixCount; k++) {
        if (badIndex(inputIndices[k], in->matrixCount) || badIndex(resultIndices[k], in->matrixCount) || inputIndices[k] == resultIndices[k])
            return BEAGLE_ERROR_OUT_OF_RANGE;
        pairs[2 * k] = inputIndices[k]; pairs[2 * k + 1] = resultIndices[k];
    }
    void* dPairs = nullptr;
    int rc = uploadTransient(in, pairs.data(), pairs.size() * sizeof(int), &dPairs); if (rc) return rc;
    mi355::launchTransposeMatrices(live(in), in->matrices, (const int*)dPairs, matrixCount, in->S, in->C);
    HIP_TRY(hipGetLastError());
    return BEAGLE_SUCCESS;
}

int beagleUpdatePrePartials(int instance, const int* operations, int operationCount, int cumulativeScaleIndex) {
    if (mi355::isShardedHandle(instance)) {
        return mi355::shardedBroadcast(instance, [&](int h) { return beagleUpdatePrePartials(h, operations, operationCount, cumulativeScaleIndex); });
    }
    GET_INSTANCE_KEEP_PENDING(instance);                      // (runPreOperations decides what becomes of a list still held back)
    DEMOTE_FOLDED_TIPS(in);                                   // (a pre-order pass reads tips' partials as data: engine_tipemission.cpp)
    return runPreOperations(in, operations, operationCount, cumulativeScaleIndex, true);
}

int beagleCalculateCrossProductDifferentials(int instance, const int* postBufferIndices, const int* preBufferIndices,
                                             const int* categoryRateIndices, const int* categoryWeightsIndices,
                                             const double* edgeLengths, int count,
                                             double* outSumDerivatives, double* outSumSquaredDerivatives) {
    if (mi355::isShardedHandle(instance)) {
        if (!outSumDerivatives) return BEAGLE_ERROR_OUT_OF_RANGE;
        const int len = shardedStates(instance) * shardedStates(instance);
        std::vector<double> tot(len, 0.0);
        const int rc = mi355::shardedSumDoubles(instance, len, [&](int h, double* out) { return beagleCalculateCrossProductDifferentials(h, postBufferIndices,
                              preBufferIndices, categoryRateIndices, categoryWeightsIndices, edgeLengths, count, out, outSumSquaredDerivatives); }, tot.data());
        for (int k = 0; k < len && !rc; k++) outSumDerivatives[k] += tot[k];
        return rc;
    }
    GET_INSTANCE(instance);
    DEMOTE_FOLDED_TIPS(in);
    if (outSumSquaredDerivatives) return BEAGLE_ERROR_NO_IMPLEMENTATION;       // BEAST passes null
    if (!postBufferIndices || !preBufferIndices || !categoryRateIndices || !categoryWeightsIndices || !edgeLengths || !outSumDerivatives)
        return BEAGLE_ERROR_OUT_OF_RANGE;
    if (badIndex(categoryRateIndices[0], in->eigenCount) || badIndex(categoryWeightsIndices[0], in->eigenCount)) return BEAGLE_ERROR_OUT_OF_RANGE;
    return crossProducts(in, postBufferIndices, preBufferIndices, categoryRateIndices[0], categoryWeightsIndices[0], edgeLengths, count,
                         outSumDerivatives);
}

int beagleCalculateEdgeDifferentials(int instance, const int* postBufferIndices, const int* preBufferIndices,
                                     const int* derivativeMatrixIndices, const int* categoryWeightsIndices, int count,
                                     double* outDerivatives, double* outSumDerivatives, double* outSumSquaredDerivatives) {
    if (mi355::isShardedHandle(instance)) {
        if (count <= 0) return BEAGLE_SUCCESS;
        const int P = mi355::shardedPatternCount(instance), n = mi355::shardedShardCount(instance);
        std::vector<std::vector<double>> per(n);
        std::vector<int> handleOf(n, -1);
        std::vector<double> tot((size_t)2 * count, 0.0);
        std::mutex mu; int next = 0;
        const int rc = mi355::shardedSumDoubles(instance, 2 * count, [&](int h, double* out) {
            int k; { std::lock_guard<std::mutex> l(mu); k = next++; handleOf[k] = h; }
            int a, b; mi355::shardedBoundsOfHandle(instance, h, &a, &b);
            if (outDerivatives) per[k].assign((size_t)count * (b - a), 0.0);
            const int r = beagleCalculateEdgeDifferentials(h, postBufferIndices, preBufferIndices, derivativeMatrixIndices, categoryWeightsIndices, count,
                                                           outDerivatives ? per[k].data() : nullptr, out, outSumSquaredDerivatives ? out + count : nullptr);   // (NULL lets a shard answer without writing pre-order partials)
            if (!r && outDerivatives)
                for (int e = 0; e < count; e++) memcpy(outDerivatives + (size_t)e * P + a, &per[k][(size_t)e * (b - a)], (size_t)(b - a) * sizeof(double));
            return r; }, tot.data());
        if (rc) return rc;
        for (int e = 0; e < count; e++) { if (outSumDerivatives) outSumDerivatives[e] = tot[e]; if (outSumSquaredDerivatives) outSumSquaredDerivatives[e] = tot[count + e]; }
        return BEAGLE_SUCCESS;
    }
    GET_INSTANCE_KEEP_PENDING(instance);                      // (a held-back pre-order list is what this call wants to run with)
    DEMOTE_FOLDED_TIPS(in);
    if (!postBufferIndices || !preBufferIndices || !derivativeMatrixIndices || !categoryWeightsIndices) return BEAGLE_ERROR_OUT_OF_RANGE;
    if (badIndex(categoryWeightsIndices[0], in->eigenCount)) return BEAGLE_ERROR_OUT_OF_RANGE;
    return edgeDifferentials(in, postBufferIndices, preBufferIndices, derivativeMatrixIndices, categoryWeightsIndices[0], count,
                             outDerivatives, outSumDerivatives, outSumSquaredDerivatives);
}

// 9-int tuples {pre(child), writeScale, readScale, pre(parent), matrix(child), post(sibling), matrix(sibling), partition,
// cumulativeScale}: beagleUpdatePrePartials over one partition's patterns (declared by BeagleJNIWrapper; no caller in BEAST today)
int beagleUpdatePrePartialsByPartition(int instance, const int* operations, int operationCount) {
    if (mi355::isShardedHandle(instance)) {
        return mi355::shardedBroadcast(instance, [&](int h) { return beagleUpdatePrePartialsByPartition(h, operations, operationCount); });
    }
    GET_INSTANCE(instance);
    DEMOTE_FOLDED_TIPS(in);
    return runPreOperations(in, operations, operationCount, BEAGLE_OP_NONE, false, BEAGLE_PARTITION_OP_COUNT);
}

static const BeagleApi g_api = {
    beagleGetVersion,
    beagleCreateInstance,
    beagleFinalizeInstance,
    beagleSetPatternWeights,
    beagleSetTipStates,
    beagleSetTipPartials,
    beagleSetPartials,
    beagleGetPartials,
    beagleGetLogScaleFactors,
    beagleSetEigenDecomposition,
    beagleSetStateFrequencies,
    beagleSetCategoryWeights,
    beagleSetCategoryRates,
    beagleSetTransitionMatrix,
    beagleGetTransitionMatrix,
    beagleUpdateTransitionMatrices,
    beagleUpdatePartials,
    beagleAccumulateScaleFactors,
    beagleRemoveScaleFactors,
    beagleResetScaleFactors,
    beagleCopyScaleFactors,
    beagleCalculateRootLogLikelihoods,
    beagleGetSiteLogLikelihoods,
    beagleMi355CalculateRootLogLikelihoodsDevice,
    beagleMi355CalculateRootLogLikelihoodsAllReduce,
};
const BeagleApi* beagleGetApiTable(void) { return &g_api; }

static const BeaglePartitionApi g_partitionApi = {
    beagleSetCategoryRatesWithIndex,
    beagleUpdateTransitionMatricesWithMultipleModels,
    beagleUpdatePartialsByPartition,
    beagleResetScaleFactorsByPartition,
    beagleAccumulateScaleFactorsByPartition,
    beagleCalculateRootLogLikelihoodsByPartition,
};
const BeaglePartitionApi* beagleGetPartitionApiTable(void) { return &g_partitionApi; }

}  // extern "C"
