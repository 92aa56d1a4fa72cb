// engine_create.cpp — instance creation: what an instance is (layouts, kernels, switches) is decided here once; and the -beagle_auto
// self-benchmark, which creates an instance per candidate resource.
#include "engine_internal.h"

using mi355::labEnv;
using namespace mi355::eng;

// an environment switch of the product library that is set to a non-zero number
static bool switchOn(const char* name) {
    const char* v = getenv(name);
    return v && atoi(v) != 0;
}

namespace mi355 {
namespace eng {

// Matrix slots of an instance: the caller's, the planner's private snapshot slots behind them and — T32 layout — one identity
// matrix and PRE_SCRATCH transposed-matrix slots behind those (the two-pass pre-order path, engine_preorder.cpp).  Sets
// preIdentity / preTransposed; used at creation and whenever the planner's slot count changes (beagleSetPatternPartitions).
size_t matrixSlotLayout(Instance* in) {
    size_t slots = std::max<size_t>(std::max<size_t>(1, in->matrixCount), (size_t)in->planner.matrixSlots());
    if (in->tiled) { in->preIdentity = (int)slots; in->preTransposed = (int)slots + 1; slots += 1 + PRE_SCRATCH; }
    // ... and, once a tip has an emission table, a shadow slot per caller matrix index behind everything else (engine_tipemission.cpp)
    if (in->emis) { in->emis->shadowBase = (int)slots; slots += (size_t)std::max(1, in->matrixCount); }
    return slots;
}
int uploadIdentityMatrix(Instance* in) {
    const size_t S = in->S, C = in->C;
    std::vector<double> eye(C * S * S, 0.0);
    for (size_t c = 0; c < C; c++) for (size_t i = 0; i < S; i++) eye[c * S * S + i * S + i] = 1.0;
    return upload(in, in->matrices + (size_t)in->preIdentity * C * S * S, eye.data(), eye.size() * sizeof(double));
}

}  // namespace eng
}  // namespace mi355

extern "C" {

// -beagle_auto: a full-tree evaluation of a synthetic alignment of the caller's shape on every candidate resource.
// Balanced tree over `tipCount` compact tips with pseudo-random states, one stochastic matrix on every branch (no eigen
// system needed: setTransitionMatrix), rescaling as the benchmark flags ask; 2 warm-up + 5 timed evaluations.
BeagleBenchmarkedResourceList* beagleGetBenchmarkedResourceList(int tipCount, int compactBufferCount, int stateCount, int patternCount,
                                      int categoryCount, const int* resourceList, int resourceCount, long preferenceFlags,
                                      long requirementFlags, int eigenModelCount, int partitionCount, int calculateDerivatives,
                                      long benchmarkFlags) {
    (void)compactBufferCount; (void)eigenModelCount; (void)partitionCount; (void)calculateDerivatives;
    static std::mutex mu;
    static std::vector<BeagleBenchmarkedResource> entries;
    static std::vector<std::string> strings;
    static BeagleBenchmarkedResourceList out;
    std::lock_guard<std::mutex> lock(mu);
    Resources* res = resources();
    std::vector<int> candidates;
    if (resourceList && resourceCount > 0) { for (int i = 0; i < resourceCount; i++) if (resourceList[i] >= 1 && resourceList[i] < res->rl.length) candidates.push_back(resourceList[i]); }
    else for (int r = 1; r < res->rl.length; r++) candidates.push_back(r);
    entries.clear(); strings.clear();
    strings.reserve(candidates.size() * 3 + 1);
    const int T = std::max(2, tipCount), S = stateCount, P = std::max(1, patternCount), C = std::max(1, categoryCount);
    const bool always = (benchmarkFlags & BEAGLE_BENCHFLAG_SCALING_ALWAYS) != 0;
    for (int r : candidates) {
        BeagleBenchmarkedResource e;
        memset(&e, 0, sizeof(e));
        e.number = r; e.name = res->rl.list[r].name; e.description = res->rl.list[r].description;
        e.supportFlags = res->rl.list[r].supportFlags; e.requiredFlags = 0; e.benchedFlags = benchmarkFlags;
        BeagleInstanceDetails det = {0, nullptr, nullptr, nullptr, 0};
        const int h = beagleCreateInstance(T, T + (T - 1), T, S, P, 1, 2 * T, C, always ? T : 0, &r, 1, preferenceFlags, requirementFlags, &det);
        e.returnCode = h < 0 ? h : 0;
        strings.push_back(det.implName ? det.implName : "");
        e.implName = (char*)strings.back().c_str();
        e.benchmarkResult = 0.0;
        if (h >= 0) {
            int rc = 0;
            std::vector<int> st(P);
            unsigned long long x = 88172645463325252ull;
            for (int t = 0; t < T && !rc; t++) {
                for (int p = 0; p < P; p++) { x ^= x << 13; x ^= x >> 7; x ^= x << 17; st[p] = (int)(x % (unsigned)S); }
                rc = beagleSetTipStates(h, t, st.data());
            }
            std::vector<double> m((size_t)C * S * S), w(C, 1.0 / C), f(S, 1.0 / S), pw(P, 1.0);
            for (int c = 0; c < C; c++) for (int i = 0; i < S; i++) for (int j = 0; j < S; j++)
                m[((size_t)c * S + i) * S + j] = i == j ? 0.9 - 0.05 * c / C : (0.1 + 0.05 * c / C) / (S - 1);
            for (int b = 0; b < 2 * T - 1 && !rc; b++) rc = beagleSetTransitionMatrix(h, b, m.data(), 0.0);
            if (!rc) rc = beagleSetCategoryWeights(h, 0, w.data());
            if (!rc) rc = beagleSetStateFrequencies(h, 0, f.data());
            if (!rc) rc = beagleSetPatternWeights(h, pw.data());
            // balanced tree: nodes 0..T-1 tips; internal node T+k joins the two oldest unjoined nodes
            std::vector<int> ops, scaleIdx;
            std::vector<int> queue(T);
            for (int t = 0; t < T; t++) queue[t] = t;
            size_t head = 0;
            for (int k = 0; k < T - 1; k++) {
                const int a = queue[head++], b = queue[head++], d = T + k;
                ops.insert(ops.end(), {d, always ? k : BEAGLE_OP_NONE, BEAGLE_OP_NONE, a, a, b, b});
                scaleIdx.push_back(k);
                queue.push_back(d);
            }
            const int root = 2 * T - 2, cum = always ? T - 1 : BEAGLE_OP_NONE, zero = 0;
            double lnl = 0.0, best = 1e300;
            for (int rep = 0; rep < 7 && !rc; rep++) {
                const auto t0 = std::chrono::steady_clock::now();
                rc = beagleUpdatePartials(h, ops.data(), T - 1, BEAGLE_OP_NONE);
                if (!rc && always) { rc = beagleResetScaleFactors(h, cum); if (!rc) rc = beagleAccumulateScaleFactors(h, scaleIdx.data(), T - 1, cum); }
                if (!rc) rc = beagleCalculateRootLogLikelihoods(h, &root, &zero, &zero, &cum, 1, &lnl);
                if (rc == BEAGLE_ERROR_FLOATING_POINT) rc = 0;
                const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
                if (rep >= 2) best = std::min(best, ms);
            }
            e.returnCode = rc;
            e.benchmarkResult = rc ? 0.0 : best;
            beagleFinalizeInstance(h);
        }
        entries.push_back(e);
    }
    std::stable_sort(entries.begin(), entries.end(), [](const BeagleBenchmarkedResource& a, const BeagleBenchmarkedResource& b) {
        const bool oa = a.returnCode == 0 && a.benchmarkResult > 0, ob = b.returnCode == 0 && b.benchmarkResult > 0;
        if (oa != ob) return oa;
        return a.benchmarkResult < b.benchmarkResult; });
    const double fastest = !entries.empty() && entries[0].benchmarkResult > 0 ? entries[0].benchmarkResult : 1.0;
    for (auto& e : entries) e.performanceRatio = e.benchmarkResult > 0 ? e.benchmarkResult / fastest : 0.0;
    out.list = entries.data(); out.length = (int)entries.size();
    return &out;
}

int beagleCreateInstance(int tipCount, int partialsBufferCount, int compactBufferCount, int stateCount,
                         int patternCount, int eigenBufferCount, int matrixBufferCount, int categoryCount,
                         int scaleBufferCount, const int* resourceList, int resourceCount,
                         long preferenceFlags, long requirementFlags, BeagleInstanceDetails* returnInfo) {
    if (tipCount < 0 || partialsBufferCount < 1 || compactBufferCount < 0 || stateCount < 2 || stateCount > 255 ||
        patternCount < 1 || eigenBufferCount < 0 || matrixBufferCount < 0 || categoryCount < 1 || scaleBufferCount < 0)
        return BEAGLE_ERROR_OUT_OF_RANGE;
    // (65..255 states — the large discrete-trait state spaces of phylogeography, GeneralLikelihoodCore.java:41-50 — run the
    // likelihood path on the general kernels, which read their matrices from L2 above ~90 states instead of staging them in LDS
    // (kernels.hip k_pruneGeneral<false>, k_transitionBig); the pre-order / gradient entry points run there too since round 5
    // (kernels_preorder.hip k_prePartialsBig, k_edgeDifferentialsBig, k_crossProductsBig: correctness paths, as k_pruneGeneral))
    // requirement flags this engine cannot honour
    if (requirementFlags & (BEAGLE_FLAG_PRECISION_SINGLE | BEAGLE_FLAG_PROCESSOR_CPU |
                            BEAGLE_FLAG_FRAMEWORK_CPU | BEAGLE_FLAG_FRAMEWORK_CUDA | BEAGLE_FLAG_FRAMEWORK_OPENCL |
                            BEAGLE_FLAG_SCALING_AUTO | BEAGLE_FLAG_VECTOR_SSE))
        return BEAGLE_ERROR_NO_RESOURCE;
    Resources* res = resources();
    int device = -1;
    if (resourceList == nullptr || resourceCount <= 0) {
        if (res->gpuCount > 0) device = 0;
    } else {
        for (int i = 0; i < resourceCount && device < 0; i++) {
            if (resourceList[i] >= 1 && resourceList[i] <= res->gpuCount) device = resourceList[i] - 1;
            else if (res->gpuCount > 0 && resourceList[i] == res->gpuCount + 1)       // "all GPUs": the pattern-sharded instance
                return mi355::shardedCreate(res->gpuCount, tipCount, partialsBufferCount, compactBufferCount, stateCount, patternCount,
                                            eigenBufferCount, matrixBufferCount, categoryCount, scaleBufferCount, preferenceFlags,
                                            requirementFlags, returnInfo);
        }
    }
    if (device < 0) return BEAGLE_ERROR_NO_RESOURCE;
    if (hipSetDevice(device) != hipSuccess) return BEAGLE_ERROR_NO_RESOURCE;

    Instance* in = new Instance();
    in->device = device;
    in->tipCount = tipCount; in->partialsCount = partialsBufferCount; in->compactCount = compactBufferCount;
    in->S = stateCount; in->P = patternCount; in->eigenCount = std::max(1, eigenBufferCount);
    // BEAST adds EIGEN_COMPLEX to the flags whenever the substitution model may have complex eigenvalues (the asymmetric
    // discrete-trait models: BeagleTreeLikelihood.java:353-355, BeagleDataLikelihoodDelegate.java:378); every eigen system of
    // such an instance then arrives in real block form with 2 S eigenvalue entries (ComplexSubstitutionModel.java:121-173)
    in->eigenComplex = (requirementFlags & BEAGLE_FLAG_EIGEN_COMPLEX) != 0;      // (a REQUIREMENT in both callers; a mere preference keeps EIGEN_REAL)
    (void)preferenceFlags;
    in->matrixCount = matrixBufferCount; in->C = categoryCount; in->scaleCount = scaleBufferCount;
    // 16..64 states: T32 layout + fp64 MFMA kernels (amino acids, codons); BEAGLE_MI355_NO_MFMA=1 keeps the VALU kernel
    in->tiled = stateCount >= 16 && stateCount <= 64 && !switchOn("BEAGLE_MI355_NO_MFMA");
    in->ntile = (patternCount + 31) / 32;
    // level order of the level kernels (engine_levels.cpp): as late as possible up to 20 states (every launch mixes the write-only
    // tip-tip nodes with read-heavy ones), as early as possible above (61 states: 214 -> 226 evals/s, profiles/r03_experiments.txt 11);
    // BEAGLE_MI355_SCHED=asap|alap overrides
    in->schedAlap = stateCount <= 20;
    if (labEnv("BEAGLE_MI355_SCHED")) {              // (LAB builds only: dfs is twice as slow, profiles/r04_experiments.txt 10)
        const char* sc = labEnv("BEAGLE_MI355_SCHED");
        in->schedAlap = strcmp(sc, "asap") != 0;
        if (strncmp(sc, "dfs", 3) == 0) in->schedDfs = sc[3] == ':' ? std::max(1, atoi(sc + 4)) : 4;
    }
    // 4 states (nucleotides), up to 16 rate categories: the pattern walk.  BEAGLE_MI355_NO_VIRTUAL=1 keeps every buffer real,
    // BEAGLE_MI355_VSTEPS=n caps the length of a virtual definition (A/B runs).
    in->walk = stateCount == 4 && categoryCount <= 16 &&
               (size_t)categoryCount * patternCount * 32 < ((size_t)1 << 32);     // the kernel addresses a buffer with 32-bit lane offsets
    const bool noVirtual = switchOn("BEAGLE_MI355_NO_VIRTUAL");
    // T32 instances with <= 20 states: tip-tip nodes ("cherries") are defined, not stored — their parent's kernel rebuilds
    // them from the tips' states (kernels_mfma.hip cherryOperands); a definition is ONE step here
    // 16..20 states: the pattern walk on the T32 layout (BEAGLE_MI355_NO_T32_WALK=1: the level kernels with virtual cherries)
    // 21..64 states (round 6): the same walk without hold slots (kernels_mfma.hip k_walkT64; BEAGLE_MI355_NO_T64_WALK=1: the level kernels)
    const bool walk64 = in->tiled && stateCount > 20 && categoryCount <= 16 && !switchOn("BEAGLE_MI355_NO_T64_WALK");
    in->walkT = in->tiled && categoryCount <= 16 && (stateCount <= 20 || walk64) && !switchOn("BEAGLE_MI355_NO_T32_WALK");
    // (above 20 states the cherries' matrices do not fit the LDS; with the tables in global memory — BEAGLE_MI355_CHERRY61=1 — a third
    // of config C's nodes is never stored and the time does not move: 232 against 234 evals/s, profiles/r03_experiments.txt 14 — so
    // that stays an experiment)
    in->cherry = in->tiled && !noVirtual && !in->walkT &&
                 (stateCount <= 20 || switchOn("BEAGLE_MI355_CHERRY61"));
    const bool virtualOn = ((in->walk || in->walkT) && !noVirtual) || in->cherry;
    in->virt = virtualOn;
    // Size of a virtual definition (internal nodes; any subtree shape whose evaluation needs at most two hold slots).
    // Evaluations at alignment sizes that keep the chip busy are bound by the bytes of the STORED nodes and their time
    // follows the cap (config A, profiles/r02_experiments.txt: cap 8 -> 207 stored nodes; 16 -> 112, 0.70 ms; 24 -> 78,
    // 0.64 ms; 32 -> 62, 0.63 ms) while a branch move — which re-evaluates the virtual siblings it passes instead of reading
    // 32 C P bytes each — costs 139 / 141 / 162 us at 16 / 24 / 32.  Small alignments are latency-bound: there the extra
    // micro-operations of long definitions show (12 500 patterns: branch move 65 -> 71 us from cap 8 to 16).
    // Round 6, the smallest alignments (a partials buffer under 64 KiB: the reference's benchmark1 alignment, 593 patterns): storing a
    // node costs next to nothing there, re-evaluating it costs stages — cap 2: a full evaluation 84.5 -> 78.6 us, a branch move 54 -> 46 us,
    // the mixed chain 12 070 -> 13 800 evaluations/s (tools/r06_vsteps_sweep.sh; at 5 565 patterns the full evaluation already prefers 8).
    const size_t bufferBytes = (size_t)categoryCount * std::max(patternCount, mi355::tlsWholePatternCount) * 32;      // (a shard of a sharded instance: as the whole would, sharded.h)
    int maxVirtSteps = bufferBytes >= ((size_t)2 << 20) ? 24 : bufferBytes < ((size_t)64 << 10) && stateCount == 4 ? 2 : 8;
    if (labEnv("BEAGLE_MI355_VSTEPS")) maxVirtSteps = std::max(1, std::min(mi355::PLAN_MAX_STEPS, atoi(labEnv("BEAGLE_MI355_VSTEPS"))));
    if (in->cherry) maxVirtSteps = 1;
    // (k_walkT64's definitions are ladders — no hold slots —, and a step's two matrix snapshots are 2 x 119 KB at 61 states and four categories)
    if (in->walkT && stateCount > 20) maxVirtSteps = std::min(maxVirtSteps, 8);
    // hold slots: three where the 4-state walk's LDS allows; TWO for the T32 walk (20 KiB each there: 3 workgroups per CU instead of 2)
    in->holdSlots = in->walkT ? (stateCount > 20 ? 0 : 2) : mi355::walkHoldSlots(categoryCount);
    if (labEnv("BEAGLE_MI355_HOLD_SLOTS") && !(in->walkT && stateCount > 20)) in->holdSlots = std::max(1, std::min(atoi(labEnv("BEAGLE_MI355_HOLD_SLOTS")), in->walkT ? 3 : mi355::walkHoldSlots(categoryCount)));
    in->fuseRootParts = !switchOn("BEAGLE_MI355_NO_ROOT_PARTS_FUSION");
    in->walkTWrite = in->walkT && stateCount <= 20 && categoryCount <= mi355::WALK_T32_WRITE_MAX_CATEGORIES && in->holdSlots <= mi355::WALK_T32_WRITE_MAX_HOLD &&
                     !switchOn("BEAGLE_MI355_NO_T32_WRITE_WALK");
    in->planner.init(partialsBufferCount, tipCount, matrixBufferCount, scaleBufferCount, maxVirtSteps, virtualOn, in->holdSlots);
    // Memory definitions (planner.h memStepCap): a node over ONE stored internal node and a tip or a small clade is defined over that
    // stored node instead of being stored itself — over half of config A's stored nodes are of that kind.  The 4-state walk
    // with hold slots, where a store is what an evaluation waits for (buffers of 2 MiB and more: the definition cap of 24); one
    // partition (the planner's users list of a stored operand is per buffer); not the gradient chain (planner.h stepLimit).  The T32 /
    // T64 walks (16..64 states) keep every such node stored.  BEAGLE_MI355_NO_MEM_DEFS=1: off;  BEAGLE_MI355_MEM_DEF_STEPS=n: the
    // cap, on any 4-state walk instance (0: off).  A full evaluation whose list has come before — the steady state of a chain of model
    // moves — is planned under the definition cap, 24: 43 stored nodes per evaluation of config A instead of 59 (planner.h memStepCapSeen,
    // profiles/table_reuse.txt); BEAGLE_MI355_MEM_DEF_SEEN_STEPS=n: that cap (at or below the other: one cap for every list, which
    // BEAGLE_MI355_MEM_DEF_STEPS alone asks for too).
    {
        int memSteps = maxVirtSteps == 24 ? MEM_DEF_STEPS : 0, seenSteps = maxVirtSteps == 24 ? MEM_DEF_SEEN_STEPS : 0;
        if (getenv("BEAGLE_MI355_MEM_DEF_STEPS")) { memSteps = std::max(0, std::min(maxVirtSteps, atoi(getenv("BEAGLE_MI355_MEM_DEF_STEPS")))); seenSteps = 0; }
        if (getenv("BEAGLE_MI355_MEM_DEF_SEEN_STEPS")) seenSteps = std::max(0, std::min(maxVirtSteps, atoi(getenv("BEAGLE_MI355_MEM_DEF_SEEN_STEPS"))));
        if (switchOn("BEAGLE_MI355_NO_MEM_DEFS") || !in->walk || in->walkT || !virtualOn || in->holdSlots < 2) memSteps = seenSteps = 0;
        in->planner.memStepCap = memSteps;
        in->planner.memStepCapSeen = seenSteps;
        // (a definition longer than this that a list only reads is stored when it is first read: engine_internal.h memDefInlineSteps)
        if (getenv("BEAGLE_MI355_MEM_DEF_INLINE_STEPS")) in->memDefInlineSteps = std::max(0, atoi(getenv("BEAGLE_MI355_MEM_DEF_INLINE_STEPS")));
    }
    // Repeated sub-patterns (engine_internal.h repeatsOn): where a node's vector is long enough for the arithmetic to be what an
    // evaluation costs — the gate of the memory definitions —; BEAGLE_MI355_REPEATS_ANY_SIZE=1: on any 4-state walk instance;
    // BEAGLE_MI355_NO_REPEATS=1: off;  BEAGLE_MI355_REPEAT_MAX_FRAC=1/n (or a decimal fraction): most classes a clade may have, of the pattern count
    {
        double frac = 1.0 / 8.0;
        if (const char* f = getenv("BEAGLE_MI355_REPEAT_MAX_FRAC")) {
            const char* slash = strchr(f, '/');
            const double num = atof(f), den = slash ? atof(slash + 1) : 1.0;
            if (num > 0.0 && den > 0.0) frac = num > 1.0 && !slash ? 1.0 / num : num / den;
        }
        frac = std::min(frac, 0.5);
        in->repeatsOn = in->walk && !in->walkT && virtualOn && stateCount == 4 && in->holdSlots >= 2 && !switchOn("BEAGLE_MI355_NO_REPEATS") &&
                        (bufferBytes >= ((size_t)2 << 20) || switchOn("BEAGLE_MI355_REPEATS_ANY_SIZE"));
        in->repeatMaxClasses = std::max(1, (int)((double)patternCount * frac));
        if (in->repeatsOn) { in->repeatIndex.init(tipCount, patternCount, in->repeatMaxClasses); in->hostTips.assign((size_t)tipCount, std::vector<uint8_t>()); }
        // BEAGLE_MI355_REPEAT_CAPACITY=n: the clades the index keeps before everything is dropped (planner.h RepeatIndex::capacity;
        // default 8 per tip + 1024) — small values make a short chain cross the reset a long one reaches (tests)
        if (in->repeatsOn && getenv("BEAGLE_MI355_REPEAT_CAPACITY")) in->repeatIndex.setCapacity((size_t)std::max(1, atoi(getenv("BEAGLE_MI355_REPEAT_CAPACITY"))));
    }
    // class tables for the plain clades inside memory definitions, and slices weighed by what that leaves (planner.h memDefTables)
    in->planner.memDefTables = !switchOn("BEAGLE_MI355_NO_MEMDEF_TABLES");
    in->planner.cacheEnabled = !switchOn("BEAGLE_MI355_NO_PLAN_CACHE");
    in->fastWalk = !switchOn("BEAGLE_MI355_NO_FAST_WALK");
    in->strictWaits = !(getenv("BEAGLE_MI355_STRICT_WAITS") && atoi(getenv("BEAGLE_MI355_STRICT_WAITS")) == 0);
    in->fuseGradient = !switchOn("BEAGLE_MI355_NO_FUSED_GRADIENT");
    in->preWalk = !switchOn("BEAGLE_MI355_NO_PRE_WALK");
    in->fuseLaunches = !switchOn("BEAGLE_MI355_NO_LAUNCH_FUSION");
    in->deferWalk = !switchOn("BEAGLE_MI355_NO_ROOT_FUSION");
    in->foldScales = !switchOn("BEAGLE_MI355_NO_SCALE_FOLD");
    // What a gradient chain's post-order passes leave unstored for the pre-order walk to re-evaluate (BEAGLE_MI355_GRADIENT_VIRTUAL):
    // 0 nothing; 1 (default) nodes over two compact tips — a third of a tree's nodes, evaluated INSIDE their parent's descriptor
    // (kernels.h PW_CHERRY); 2 also such a node under one more tip (descriptors of their own, PW_POSTOP: half the nodes, but a
    // descriptor costs a stage whatever it computes — slower than 1, for whoever needs the memory: profiles/r05_experiments.txt 5, 14)
    {
        const int gv = getenv("BEAGLE_MI355_GRADIENT_VIRTUAL") ? atoi(getenv("BEAGLE_MI355_GRADIENT_VIRTUAL")) : GRADIENT_VIRT_DEFAULT;
        in->gradientVirtual = in->walk && virtualOn && in->preWalk && in->fuseGradient && gv > 0;
        in->gradientVirtualSteps = std::max(1, std::min(GRADIENT_VIRT_STEPS, gv));
    }
    // matrix storage: the caller's buffers, then the private snapshot slots of virtual definitions (planner.h)
    const size_t matrixSlots = matrixSlotLayout(in);
    const size_t patternSlots = in->tiled ? (size_t)in->ntile * 32 : (size_t)patternCount;
    in->partialsBytes = (((size_t)categoryCount * patternSlots * stateCount * sizeof(double)) + 255 + (in->walk ? 256 : 0)) & ~(size_t)255;
    in->partials.assign(partialsBufferCount, nullptr);
    in->scaleOfPartial.assign(partialsBufferCount, -2); in->scaleVersionAtWrite.assign(partialsBufferCount, 0u);     // (-2: unknown)
    in->scaleVersion.assign(std::max(1, scaleBufferCount), 0u);
    in->tipStates.assign(partialsBufferCount, nullptr);
    in->scale.assign(std::max(1, scaleBufferCount), nullptr);
    in->scaleIsRaw.assign(std::max(1, scaleBufferCount), 0);
    in->partStart.assign(1, 0); in->partEnd.assign(1, patternCount);
    setPairLayout(in);                                                    // one partition: whole blocks of 128 patterns
    in->wStamp.assign(partialsBufferCount, 0); in->wLevel.assign(partialsBufferCount, 0); in->wOp.assign(partialsBufferCount, 0);
    in->rStamp.assign(partialsBufferCount, 0); in->rLevel.assign(partialsBufferCount, 0);
    in->resourceName = res->names[device + 1];

    bool ok = hipStreamCreateWithFlags(&in->ownStream, hipStreamNonBlocking) == hipSuccess;
    in->stream = in->ownStream;
    ok = ok && hipHostMalloc((void**)&in->hRing, RING_BYTES, hipHostMallocMapped | hipHostMallocCoherent) == hipSuccess;
    ok = ok && hipHostGetDevicePointer((void**)&in->hRingDev, in->hRing, 0) == hipSuccess;     // (the copies out of the ring are a kernel's: flushUploads)
    in->kernelUploads = !switchOn("BEAGLE_MI355_COPY_ENGINE_UPLOADS");
    in->sitePrefetch = !switchOn("BEAGLE_MI355_NO_SITE_PREFETCH");
    in->fuseWaves = !switchOn("BEAGLE_MI355_NO_WALK_FUSION");
    in->useTickets = !switchOn("BEAGLE_MI355_NO_WALK_TICKETS");
    in->xcdAware = !switchOn("BEAGLE_MI355_NO_XCD_MAP");
    in->fuseCherries = !switchOn("BEAGLE_MI355_NO_CHERRY_FUSION");
    in->skipTipLoads = !switchOn("BEAGLE_MI355_NO_LOAD_SKIP");
    in->sliceSums = !switchOn("BEAGLE_MI355_NO_SLICE_SUMS");
    in->hostTrace = getenv("BEAGLE_MI355_HOST_TIMING") && atoi(getenv("BEAGLE_MI355_HOST_TIMING")) > 1;     // (a line per slow updatePartials call)
    if (getenv("BEAGLE_MI355_WALK_SPIN_US")) in->walkSpinLimit = (unsigned long long)std::max(0L, atol(getenv("BEAGLE_MI355_WALK_SPIN_US"))) * 100ull;
    if (in->walk && in->fuseWaves && in->fastWalk) {
        // (on tickets — the default — a slice above the first wave costs no workgroup slots and no polling, and the first wave is the whole
        // grid: 8 above / about twice as long first-wave slices measured best at 12 500 patterns, tools/r06_ticket_sweep.sh)
        in->planner.chunkTopOps = labEnv("BEAGLE_MI355_CHUNK_TOP") ? atoi(labEnv("BEAGLE_MI355_CHUNK_TOP")) : in->useTickets ? 8 : 16;
        // slices the chip holds side by side: 4 workgroups per CU over the pattern groups of a slice (planner.h launchMachines)
        hipDeviceProp_t prop;
        const int cus = hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
        in->planner.launchMachines = (double)(4 * cus) / (double)std::max(1, (patternCount + 127) / 128);
        if (labEnv("BEAGLE_MI355_SCHED_SIM") && atoi(labEnv("BEAGLE_MI355_SCHED_SIM")) == 0) in->planner.launchMachines = 0.0;
    }
    // compressed evaluations are cut by their remaining work (engine_internal.h repeatSlicing)
    in->repeatSlicing = in->repeatsOn && in->fastWalk && in->fuseWaves && in->useTickets && !switchOn("BEAGLE_MI355_NO_REPEAT_SLICING");
    if (in->repeatSlicing) {
        Instance* const self = in;
        in->planner.repeatChunkRule = [self](long weight, int& chunk, int& top) { walkRepeatChunkOps(self, weight, chunk, top); };
    }
    // result words live in coherent, device-mapped host memory: the final reduction kernel writes the sum straight into it
    // and the host only waits for the stream (no device-to-host copy behind the last kernel)
    ok = ok && hipHostMalloc((void**)&in->hResult, 4096, hipHostMallocMapped | hipHostMallocCoherent) == hipSuccess;
    ok = ok && hipHostGetDevicePointer((void**)&in->hResultDev, in->hResult, 0) == hipSuccess;
    const size_t S = stateCount, C = categoryCount, E = in->eigenCount;
    const int rootBlocks = (patternCount + 63) / 64;          // (the T32 root kernel: a partial sum per 64 patterns; 4 states: per 256)
    ok = ok && devAlloc(in, (void**)&in->dRing, RING_BYTES) == 0;
    ok = ok && devAlloc(in, (void**)&in->matrices, matrixSlots * C * S * S * sizeof(double)) == 0;
    ok = ok && devAlloc(in, (void**)&in->eigen, E * (2 * S * S + 2 * S) * sizeof(double)) == 0;
    ok = ok && devAlloc(in, (void**)&in->rates, E * C * sizeof(double)) == 0;
    ok = ok && devAlloc(in, (void**)&in->weights, E * C * sizeof(double)) == 0;
    ok = ok && devAlloc(in, (void**)&in->freqs, E * S * sizeof(double)) == 0;
    ok = ok && devAlloc(in, (void**)&in->patternWeights, (size_t)patternCount * sizeof(double)) == 0;
    ok = ok && devAlloc(in, (void**)&in->siteLogL, (size_t)patternCount * sizeof(double)) == 0;
    ok = ok && devAlloc(in, (void**)&in->blockSums, ((size_t)rootBlocks + 1024) * sizeof(double)) == 0;    // (+ one partial block per partition)
    ok = ok && devAlloc(in, (void**)&in->dResult, 4096) == 0;
    ok = ok && devAlloc(in, (void**)&in->rootCounter, 256) == 0 && hipMemset(in->rootCounter, 0, 256) == hipSuccess;
    if (ok) in->walkSelfServed = in->rootCounter + 32;       // (its own 128-byte line of the same allocation)
    if (ok) {
        // defaults: category rates 1, weights 1/C, pattern weights 1 (beagle.jar!GeneralBeagleImpl#<init>)
        std::vector<double> ones(std::max<size_t>((size_t)patternCount, E * C), 1.0);
        ok = upload(in, in->rates, ones.data(), E * C * sizeof(double)) == 0;
        ok = ok && upload(in, in->patternWeights, ones.data(), (size_t)patternCount * sizeof(double)) == 0;
        std::vector<double> w(E * C, 1.0 / (double)C);
        ok = ok && upload(in, in->weights, w.data(), E * C * sizeof(double)) == 0;
        ok = ok && hipMemsetAsync(in->matrices, 0, matrixSlots * C * S * S * sizeof(double), live(in)) == hipSuccess;
        ok = ok && hipMemsetAsync(in->siteLogL, 0, (size_t)patternCount * sizeof(double), live(in)) == hipSuccess;
        if (ok && in->tiled) ok = uploadIdentityMatrix(in) == 0;   // for the two-pass pre-order path
    }
    if (!ok) { destroy(in); return BEAGLE_ERROR_OUT_OF_MEMORY; }

    int handle = -1;
    {
        std::lock_guard<std::mutex> lock(g_mutex);
        for (size_t i = 0; i < g_instances.size(); i++) if (!g_instances[i]) { handle = (int)i; break; }
        if (handle < 0) { g_instances.push_back(nullptr); handle = (int)g_instances.size() - 1; }
        g_instances[handle] = in;
    }
    if (returnInfo) {
        returnInfo->resourceNumber = device + 1;
        returnInfo->resourceName = (char*)in->resourceName.c_str();
        returnInfo->implName = (char*)"HIP-gfx950-fp64";
        returnInfo->implDescription = (char*)"hand-written CDNA4 kernels, level-batched pruning";
        returnInfo->flags = GPU_FLAGS & ~(BEAGLE_FLAG_SCALING_ALWAYS | BEAGLE_FLAG_SCALING_DYNAMIC) &
                            ~(in->eigenComplex ? BEAGLE_FLAG_EIGEN_REAL : BEAGLE_FLAG_EIGEN_COMPLEX);
    }
    return handle;
}

}  // extern "C"
