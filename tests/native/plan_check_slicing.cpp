// plan_check_slicing.cpp — slices cut by what compression leaves of a list (beast-mcmc_amd/csrc/planner.h WalkPlanner::repeatWeights) on the
// CPU.  TEST INFRASTRUCTURE, not product.
//
// On plan_harness.h's harness (its worlds, tree, buffer protocol and index-level interpreters):
// random and caterpillar trees of 24, 48 and 200 tips and one seeded random tree of 1 000, definition caps 8 and 24, memory-definition
// caps 0 and 8, every list planned twice — by two planners fed the same calls, one weighing a plain definition as its steps (the cut of
// the uncompressed list), one as the single gather it becomes.  Under the compressed weighting
//   * every stored buffer has the bits of list-order evaluation, and with folded reciprocals (caps 32, 4, 2 in turn) is within 1e-12 of it
//     (Harness::update, as for every plan of plan_check.cpp);
//   * the plan compresses (findRepeatRuns, emitRepeatPlan): the walk's micro-operations pay every fold member of the uncompressed plan, and
//     the compressed plan — tables at the representatives, consumers reading class rows — leaves the bits the uncompressed plan leaves;
//   * the slices form a forest, none is empty, and every slice stands behind the slices it reads in Plan::launchOrder;
//   * the stored set is that of the other weighting;
//   * no peeled slice weighs more than its chunk unless it holds one stored node only (nothing below it was left to peel);
//   * the 1 000-tip tree is cut into strictly fewer slices than by its list length, at the same chunk;
//   * the same list under the other weighting is a cache miss, and a hit again under the first.
#include "plan_harness.h"
#include <set>

static long g_compressedPlans = 0, g_runsTaken = 0;
// the plan the harness has just run (h.plan holds its results; the snapshot copies are idempotent), compressed
static void checkCompression(Harness& h) {
    if (h.pl.plannedTag == 0) return;
    const Plan& plan = *h.pl.planned;
    FoldMap fm;
    if (!foldScaleFactors(plan, 32, fm)) return;              // (a list that rescales in write mode)
    RepeatIndex idx; idx.init(h.T, P, std::max(1, P / 4));
    for (int t = 0; t < h.T; t++) if (h.compact[(size_t)t]) idx.setTip(t, h.plan.tips[(size_t)t].data());
    std::vector<RepeatRun> cand;
    findRepeatRuns(plan, &fm, idx, true, cand);
    if (cand.empty()) return;
    RepeatPlan rp;
    emitRepeatPlan(plan, cand, rp);
    g_compressedPlans++; g_runsTaken += (long)cand.size();
    size_t upperOps = 0, paid = 0;
    for (const PlanSeg& sg : rp.plan.segs) { REQUIRE(sg.progCount > 0, "a slice that compression emptied"); upperOps += (size_t)sg.progCount; }
    for (size_t k = 0; k < upperOps; k++) paid += (size_t)(fm.payStart[(size_t)rp.origin[k] + 1] - fm.payStart[(size_t)rp.origin[k]]);
    REQUIRE(paid == fm.members.size(), "%zu of %zu fold members are paid by the walk", paid, fm.members.size());
    World a = h.plan, b = h.plan;
    runPlan(a, plan, h.partStart, h.partEnd, &fm);
    runCompressed(b, rp, &fm, idx, h.partStart, h.partEnd);
    for (int buf = 0; buf < h.nBuf; buf++) {
        REQUIRE(a.partials[(size_t)buf].size() == b.partials[(size_t)buf].size(), "buffer %d", buf);
        if (!a.partials[(size_t)buf].empty()) REQUIRE(memcmp(a.partials[(size_t)buf].data(), b.partials[(size_t)buf].data(), a.partials[(size_t)buf].size() * 8) == 0, "buffer %d differs from the uncompressed plan", buf);
    }
}

static long g_peeled = 0, g_heavy = 0;
static void checkSlices(const Plan& plan, int chunk, int top, bool compressedWeights) {
    const int n = (int)plan.segs.size();
    if (plan.prog.empty()) return;                             // (a tree small enough to be ONE definition: nothing runs)
    REQUIRE(n > 0 && (int)plan.launchOrder.size() == n, "launch order of %d slices", n);
    std::vector<int> dependants((size_t)n, 0), pos((size_t)n, -1);
    for (int i = 0; i < n; i++) { REQUIRE(pos[(size_t)plan.launchOrder[(size_t)i]] < 0, "launch order names a slice twice"); pos[(size_t)plan.launchOrder[(size_t)i]] = i; }
    int lastWave = 0;
    for (int s = 0; s < n; s++) {
        const PlanSeg& sg = plan.segs[(size_t)s];
        REQUIRE(sg.progCount > 0, "slice %d is empty", s);
        lastWave = std::max(lastWave, sg.wave);
        for (int d = sg.depStart; d < sg.depStart + sg.depCount; d++) {
            const int by = plan.deps[(size_t)d];
            dependants[(size_t)by]++;
            REQUIRE(plan.segs[(size_t)by].wave < sg.wave, "slice %d reads slice %d of no earlier wave", s, by);
            REQUIRE(pos[(size_t)by] < pos[(size_t)s], "slice %d is launched before slice %d, which it reads", s, by);
        }
    }
    int leaves = 0;
    for (int s = 0; s < n; s++) { REQUIRE(dependants[(size_t)s] <= 1, "slice %d has %d dependants", s, dependants[(size_t)s]); if (plan.segs[(size_t)s].depCount == 0) leaves++; }
    REQUIRE(plan.leaves == leaves, "the planner counts %d leaves of %d", plan.leaves, leaves);
    if (chunk <= 0) return;
    for (int s = 0; s < n; s++) {
        const PlanSeg& sg = plan.segs[(size_t)s];
        if (sg.wave == lastWave) continue;                     // (what is left at the end is one slice whatever it weighs)
        int weight = sg.progCount, stores = 0;
        if (compressedWeights)
            for (const PlanRun& run : plan.runs)
                if (run.start >= sg.progStart && run.start < sg.progStart + sg.progCount && plainRun(plan, run)) weight -= run.count - 1;
        for (int k = sg.progStart; k < sg.progStart + sg.progCount; k++) stores += plan.prog[(size_t)k].storeBuf >= 0;
        const int limit = sg.wave == 0 || top <= 0 ? chunk : std::min(chunk, top);
        g_peeled++;
        if (weight > limit) { g_heavy++; REQUIRE(stores == 1, "slice %d of wave %d weighs %d over a chunk of %d and stores %d nodes", s, sg.wave, weight, limit, stores); }
    }
}

static std::set<int> storedSet(const Plan& plan) {
    std::set<int> s;
    for (const MicroOp& m : plan.prog) if (m.storeBuf >= 0) s.insert(m.storeBuf);
    return s;
}

static long g_fewer = 0, g_lists = 0, g_foldedCompared = 0, g_foldedDiffer = 0;
// returns the slices of the last read-mode plan under {list-length, compressed} weights
static std::pair<int, int> scenario(int T, bool caterpillar, int patterns, unsigned seed, int defCapSeed, int memCap, int chunk, int top, int lists) {
    P = patterns; C = 2;
    static char where[160]; snprintf(where, sizeof where, "slicing T=%d cat=%d P=%d seed=%u caps %d/%d chunk %d top %d", T, (int)caterpillar, patterns, seed, defCapSeed == 7 ? 8 : 24, memCap, chunk, top);
    g_where = where; g_list = 0;
    std::mt19937 rng(seed);
    Tree tree; tree.random(T, rng, caterpillar);
    const int N = 2 * T - 1;
    const auto tips = repeatingTips(T, patterns, rng);
    Harness hs[2];                                             // [0]: a definition weighs its steps;  [1]: a plain one weighs one gather
    for (int w = 0; w < 2; w++) {
        Harness& h = hs[w];
        h.init(T, T + 2 * (T - 1), 2 * N, 2 * (T - 1), true, (unsigned)defCapSeed);      // (7: definition cap 8, 10: cap 24; three hold slots both)
        h.rng.seed(seed);
        h.pl.memStepCap = memCap; h.pl.chunkTopOps = top; h.pl.launchMachines = 1024.0 / 782.0;
        h.pl.repeatWeights = w == 1;
        h.fixedChunk = chunk;
        for (int t = 0; t < T; t++) {
            h.truth.tips[(size_t)t] = tips[(size_t)t]; h.plan.tips[(size_t)t] = tips[(size_t)t];
            h.compact[(size_t)t] = 1; h.pl.setCompactTip(t, true); h.pl.setLeafPartials(t, false);
        }
        for (int s = 0; s < 2 * N; s++) h.setMatrix(s);
    }
    Protocol pr(tree);
    std::vector<int> order;
    if (seed % 2) order = tree.levelOrder(); else tree.postOrder(N - 1, order);
    std::pair<int, int> slices{0, 0};
    for (int it = 0; it < lists; it++) {
        for (int n : order) pr.pFlip[n] ^= 1;
        for (int n = 0; n < N - 1; n++) pr.mFlip[n] ^= 1;
        std::vector<int> ops; pr.emit(order, it == 0 ? 0 : it == 1 ? 1 : 2, ops);      // no scaling, write mode, then read mode
        for (int w = 0; w < 2; w++) {
            Harness& h = hs[w];
            for (int n = 0; n < N - 1; n++) h.setMatrix(pr.mBuf(n));
            h.update(ops, 7);                                  // (bits against list order; folded: within 1e-12)
            REQUIRE(h.pl.plannedTag != 0, "a full evaluation is a cached plan");
            const bool weighed = h.pl.lastWeighed > 0;
            if (!h.pl.planned->prog.empty()) REQUIRE(weighed == (w == 1 && it != 1), "weight %ld of list %d under mode %d", h.pl.lastWeighed, it, w);
            checkSlices(*h.pl.planned, chunk, top, weighed);
            if (w == 1) checkCompression(h);
        }
        const Plan &a = *hs[0].pl.planned, &b = *hs[1].pl.planned;
        REQUIRE(storedSet(a) == storedSet(b), "the stored sets differ: %zu nodes against %zu", storedSet(a).size(), storedSet(b).size());
        REQUIRE(a.prog.size() == b.prog.size(), "%zu micro-operations against %zu", a.prog.size(), b.prog.size());
        if (it == 1) REQUIRE(a.segs.size() == b.segs.size(), "a list that rescales is cut as before: %zu slices against %zu", a.segs.size(), b.segs.size());
        else { REQUIRE(b.segs.size() <= a.segs.size(), "%zu slices where the list's length gives %zu", b.segs.size(), a.segs.size()); g_fewer += b.segs.size() < a.segs.size(); }
        if (it >= 2 && hs[0].nBuf <= 1200) {                   // folded reciprocals under the two cuts: the same members in the same order?
            FoldMap fa, fb;
            if (foldScaleFactors(a, 32, fa) && foldScaleFactors(b, 32, fb)) {
                World wa = hs[0].plan, wb = hs[1].plan;
                runPlan(wa, a, hs[0].partStart, hs[0].partEnd, &fa);
                runPlan(wb, b, hs[1].partStart, hs[1].partEnd, &fb);
                for (int buf = 0; buf < hs[0].nBuf; buf++)
                    if (!wa.partials[(size_t)buf].empty() && memcmp(wa.partials[(size_t)buf].data(), wb.partials[(size_t)buf].data(), wa.partials[(size_t)buf].size() * 8) != 0) g_foldedDiffer++;
                g_foldedCompared++;
            }
        }
        slices = {(int)a.segs.size(), (int)b.segs.size()};
        g_lists++;
    }
    {   // the weighting is part of a cached plan's identity
        Harness& h = hs[1];
        std::vector<int> ops; pr.emit(order, 2, ops);          // (the last list once more)
        const int count = (int)ops.size() / 7;
        Plan scratch;
        long hits = h.pl.cacheHits;
        REQUIRE(h.pl.plan(ops.data(), count, 7, 1, true, scratch, chunk) == 0 && h.pl.cacheHits == hits + 1, "the same list under the same weighting is a hit");
        h.pl.repeatWeights = false;
        hits = h.pl.cacheHits;
        bool simple = false;
        REQUIRE(!h.pl.replayCached(ops.data(), count, 7, 1, true, chunk, &simple), "replayed under the other weighting");
        REQUIRE(h.pl.plan(ops.data(), count, 7, 1, true, scratch, chunk) == 0 && h.pl.cacheHits == hits, "the same list under the other weighting is a miss");
        REQUIRE(h.pl.lastWeighed == 0 && h.pl.planned->segs.size() == (size_t)slices.first, "... and is cut by its length: %zu slices, %d", h.pl.planned->segs.size(), slices.first);
        h.pl.repeatWeights = true;
        REQUIRE(h.pl.plan(ops.data(), count, 7, 1, true, scratch, chunk) == 0 && h.pl.cacheHits == hits + 1 && (h.pl.lastWeighed > 0 || h.pl.planned->prog.empty()) &&
                h.pl.planned->segs.size() == (size_t)slices.second, "back under the first weighting: a hit");
    }
    return slices;
}

int main() {
    unsigned seed = 1;
    for (int T : {24, 48, 200})
        for (int cat = 0; cat < 2; cat++)
            for (int defCapSeed : {7, 10})
                for (int memCap : {0, 8}) {
                    const int chunk = T == 200 ? 20 : 8;
                    scenario(T, cat != 0, T == 200 ? 40 : 129, seed, defCapSeed, memCap, chunk, seed % 3 == 0 ? 0 : 8, 6);
                    seed++;
                }
    printf("  %ld lists, %ld of them in fewer slices; %ld plans compressed (%ld runs); %ld peeled slices, %ld of them one node heavier than its chunk\n",
           g_lists, g_fewer, g_compressedPlans, g_runsTaken, g_peeled, g_heavy);
    printf("  folded reciprocals under the two cuts: %ld lists compared, %ld stored buffers with other bits\n", g_foldedCompared, g_foldedDiffer);
    REQUIRE(g_fewer > 0 && g_compressedPlans > 0 && g_peeled > 0, "nothing was cut differently, compressed or peeled");
    // the engine's large case: 1 000 tips, definitions of up to 24 steps, memory definitions of up to 8, the chunk of a long list
    const std::pair<int, int> big = scenario(1000, false, 16, 1, 10, 8, 150, 8, 3);
    printf("  1000 tips, chunk 150: %d slices by the list's length, %d by what compression leaves\n", big.first, big.second);
    REQUIRE(big.second < big.first, "%d slices against %d", big.second, big.first);
    printDigest();
    printf("plan_check_slicing: OK\n");
    return 0;
}
