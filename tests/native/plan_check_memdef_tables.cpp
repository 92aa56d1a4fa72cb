// plan_check_memdef_tables.cpp — class tables for the plain clades inside memory definitions (beast-mcmc_amd/csrc/planner.h RepeatRun: sub-runs,
// WalkPlanner::memDefTables) on the CPU.  TEST INFRASTRUCTURE, not product.
//
// On plan_harness.h's harness (its worlds, tree, buffer protocol and index-level interpreters).  Random and caterpillar trees of 24, 48 and 200 tips and two seeded
// random trees of 1 000, definition caps 8 and 24, memory-definition caps 8 and 24 — for every list, and as the engine has them: 8 when a closed
// list is first seen, 24 when it comes again.  Every list is planned by two planners fed the same calls, one with the feature and one with the
// switch set (memDefTables = false), both weighing for compression.  Asserted:
//   * every stored buffer has the bits of list-order evaluation, and with folded reciprocals is within 1e-12 of it (Harness::update);
//   * after compression every stored buffer has the bits the uncompressed plan leaves, and the walk pays every fold member (fold caps 32, 4, 2);
//   * no micro-operation left in the upper program heads a sub-tree, within its slice, that reads tips only and meets the conditions of a
//     whole run: nothing stored, nothing paid, its result read in the same slice;
//   * with the switch set nothing is taken but whole runs, a slice weighs what the whole-run rule gives it (plan_check_slicing.cpp's check),
//     and the feature is part of a cached plan's identity; a plan without memory definitions is the same bytes on both sides;
//   * the 1 000-tip trees planned under the longer cap leave no more micro-operations in the walk than under cap 8 plus their path steps,
//     and are cut into no more slices and waves than under cap 8 plus one each.
#include "plan_harness.h"

// micro-operations of the upper program that head a sub-tree over tips only which a class table could have stood for: within the slice it
// reads tips, the ACC or a hold slot of such sub-trees only, stores and pays nothing, and a micro-operation of the slice reads its result
static int plainHeadsLeft(const RepeatPlan& rp, const FoldMap& fm, int tipCount) {
    const Plan& plan = rp.plan;
    int left = 0;
    for (const PlanSeg& sg : plan.segs) {
        std::vector<char> plain((size_t)sg.progCount, 0);
        int parked[3] = {-1, -1, -1};
        for (int k = sg.progStart; k < sg.progStart + sg.progCount; k++) {
            const MicroOp& m = plan.prog[(size_t)k];
            const int o = rp.origin[(size_t)k];
            bool ok = m.storeBuf < 0 && fm.payStart[(size_t)o + 1] == fm.payStart[(size_t)o];
            if (m.k1 == PK_TIPS) ok = ok && m.a1 < tipCount;
            else if (isHoldKind(m.k1)) { const int h = parked[m.k1 - PK_H0]; ok = ok && h >= 0 && plain[(size_t)(h - sg.progStart)]; parked[m.k1 - PK_H0] = -1; }
            else ok = false;
            if (m.k2 == PK_TIPS) ok = ok && m.a2 < tipCount;
            else if (m.k2 == PK_ACC) ok = ok && k > sg.progStart && plain[(size_t)(k - 1 - sg.progStart)];
            else ok = false;
            plain[(size_t)(k - sg.progStart)] = ok;
            if (m.hold) parked[m.hold - 1] = k;
        }
        for (int k = sg.progStart; k < sg.progStart + sg.progCount; k++) {
            if (!plain[(size_t)(k - sg.progStart)]) continue;
            const MicroOp& m = plan.prog[(size_t)k];
            bool read = false;
            if (m.hold) { for (int j = k + 1; j < sg.progStart + sg.progCount && !read; j++) read = plan.prog[(size_t)j].k1 == PK_H0 + m.hold - 1; }
            else read = k + 1 < sg.progStart + sg.progCount && plan.prog[(size_t)k + 1].k2 == PK_ACC;
            if (read) left++;
        }
    }
    return left;
}

struct Compressed { bool any = false; int upper = 0, unstored = 0, taken = 0, sub = 0, subOps = 0; };
static long g_compressed = 0, g_subRuns = 0, g_subOps = 0, g_wholeRuns = 0;
// the plan the harness has just run (h.plan holds its results; the snapshot copies are idempotent), compressed
static Compressed checkCompression(Harness& h, int foldCap) {
    Compressed out;
    if (h.pl.plannedTag == 0) return out;
    const Plan& plan = *h.pl.planned;
    FoldMap fm;
    if (!foldScaleFactors(plan, foldCap, fm)) return out;     // (a list that rescales in write mode)
    RepeatIndex idx; idx.init(h.T, P, 65535);                 // (no clade is over the class limit)
    for (int t = 0; t < h.T; t++) if (h.compact[(size_t)t]) idx.setTip(t, h.plan.tips[(size_t)t].data());
    std::vector<RepeatRun> cand;
    findRepeatRuns(plan, &fm, idx, true, cand, nullptr, h.pl.memDefTables);
    if (cand.empty()) return out;
    int at = -1;
    for (const RepeatRun& r : cand) {
        REQUIRE(r.start > at && r.count > 0, "candidates out of program order, or overlapping, at %d", r.start);
        at = r.start + r.count - 1;
        bool whole = false;
        for (const PlanRun& run : plan.runs) whole = whole || (run.start == r.start && run.count == r.count);
        REQUIRE(whole == !r.sub, "a range [%d, +%d) that is %s run is marked %s", r.start, r.count, whole ? "a whole" : "no whole", r.sub ? "a sub-run" : "whole");
        REQUIRE(h.pl.memDefTables || !r.sub, "a sub-run with the switch set");
        if (r.sub) {
            bool inside = false;
            for (const PlanRun& run : plan.runs) inside = inside || (r.start >= run.start && r.consumer < run.start + run.count);
            REQUIRE(inside, "the sub-run at %d is read at %d, outside its run", r.start, r.consumer);
        }
    }
    RepeatPlan rp;
    emitRepeatPlan(plan, cand, rp);
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
    if (h.pl.memDefTables) {
        const int left = plainHeadsLeft(rp, fm, h.T);
        REQUIRE(left == 0, "%d micro-operations left in the walk head a sub-tree over tips that meets the conditions of a whole run", left);
    }
    out.any = true; out.upper = (int)upperOps; out.taken = (int)cand.size(); out.sub = rp.subRuns; out.subOps = rp.subRunOps;
    for (size_t k = 0; k < upperOps; k++) out.unstored += rp.plan.prog[k].storeBuf < 0;
    int subs = 0; for (const RepeatRun& r : cand) subs += r.sub;
    REQUIRE(subs == rp.subRuns, "the compressed plan counts %d sub-runs of %d", rp.subRuns, subs);
    g_compressed++; g_subRuns += rp.subRuns; g_subOps += rp.subRunOps; g_wholeRuns += (long)cand.size() - rp.subRuns;
    return out;
}

// ... and its check of a peeled slice's weight: with the switch set that rule is the planner's
static long g_peeled = 0;
static void checkWholeRunWeights(const Plan& plan, int chunk, int top) {
    int lastWave = 0;
    for (const PlanSeg& sg : plan.segs) lastWave = std::max(lastWave, sg.wave);
    for (size_t s = 0; s < plan.segs.size() && chunk > 0; s++) {
        const PlanSeg& sg = plan.segs[s];
        if (sg.wave == lastWave) continue;
        int weight = sg.progCount, stores = 0;
        for (const PlanRun& run : plan.runs)
            if (run.start >= sg.progStart && run.start < sg.progStart + sg.progCount && plainRun(plan, run)) weight -= run.count - 1;
        for (int k = sg.progStart; k < sg.progStart + sg.progCount; k++) stores += plan.prog[(size_t)k].storeBuf >= 0;
        const int limit = sg.wave == 0 || top <= 0 ? chunk : std::min(chunk, top);
        g_peeled++;
        if (weight > limit) REQUIRE(stores == 1, "switch set: slice %zu of wave %d weighs %d over a chunk of %d and stores %d nodes", s, sg.wave, weight, limit, stores);
    }
}

static bool samePlan(const Plan& a, const Plan& b) {
    auto same = [](const auto& x, const auto& y) { return x.size() == y.size() && (x.empty() || memcmp(x.data(), y.data(), x.size() * sizeof(x[0])) == 0); };
    if (a.prog.size() != b.prog.size() || a.segs.size() != b.segs.size() || a.leaves != b.leaves) return false;
    for (size_t i = 0; i < a.prog.size(); i++) {
        const MicroOp &x = a.prog[i], &y = b.prog[i];
        if (x.storeBuf != y.storeBuf || x.k1 != y.k1 || x.a1 != y.a1 || x.k2 != y.k2 || x.a2 != y.a2 || x.mat1 != y.mat1 || x.mat2 != y.mat2 || x.scaleIdx != y.scaleIdx || x.smode != y.smode || x.hold != y.hold) return false;
    }
    for (size_t i = 0; i < a.segs.size(); i++) {
        const PlanSeg &x = a.segs[i], &y = b.segs[i];
        if (x.progStart != y.progStart || x.progCount != y.progCount || x.partition != y.partition || x.wave != y.wave || x.depStart != y.depStart || x.depCount != y.depCount || x.tail != y.tail || x.next != y.next) return false;
    }
    return same(a.deps, b.deps) && same(a.launchOrder, b.launchOrder) && same(a.snapPairs, b.snapPairs);
}

static int wavesOf(const Plan& plan) { int w = 0; for (const PlanSeg& sg : plan.segs) w = std::max(w, sg.wave + 1); return plan.segs.empty() ? 0 : w; }

struct Outcome { Compressed on, off; int slices = 0, waves = 0, stored = 0, slicesOff = 0, wavesOff = 0; long weighed = 0, weighedOff = 0; };      // (off: with the switch set)
static long g_lists = 0, g_samePlans = 0, g_otherCuts = 0;
// the last read-mode plan with the feature on
static Outcome scenario(int T, bool caterpillar, int patterns, unsigned seed, int defCapSeed, int memCap, int seenCap, int chunk, int top, int lists) {
    P = patterns; C = 2;
    static char where[200]; snprintf(where, sizeof where, "memdef tables T=%d cat=%d P=%d seed=%u caps %d/%d/%d chunk %d top %d", T, (int)caterpillar, patterns, seed, defCapSeed == 7 ? 8 : 24, memCap, seenCap, chunk, top);
    g_where = where; g_list = 0;
    std::mt19937 rng(seed);
    Tree tree; tree.random(T, rng, caterpillar);
    const int N = 2 * T - 1;
    const auto tips = repeatingTips(T, patterns, rng);
    Harness hs[2];                                             // [0]: the feature;  [1]: the switch set
    for (int w = 0; w < 2; w++) {
        Harness& h = hs[w];
        h.init(T, T + 2 * (T - 1), 2 * N, 2 * (T - 1), true, (unsigned)defCapSeed);      // (7: definition cap 8, 10: cap 24; three hold slots both)
        h.rng.seed(seed);
        h.pl.memStepCap = memCap; h.pl.memStepCapSeen = seenCap; h.pl.chunkTopOps = top; h.pl.launchMachines = 1024.0 / 782.0;
        h.pl.repeatWeights = true; h.pl.memDefTables = w == 0;
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
    Outcome last;
    static const int foldCaps[3] = {32, 4, 2};
    for (int it = 0; it < lists; it++) {
        for (int n : order) pr.pFlip[n] ^= 1;
        for (int n = 0; n < N - 1; n++) pr.mFlip[n] ^= 1;
        std::vector<int> ops; pr.emit(order, it == 0 ? 0 : it == 1 ? 1 : 2, ops);      // no scaling, write mode, then read mode: two lists alternate
        Compressed got[2];
        for (int w = 0; w < 2; w++) {
            Harness& h = hs[w];
            for (int n = 0; n < N - 1; n++) h.setMatrix(pr.mBuf(n));
            h.update(ops, 7);                                  // (bits against list order; folded: within 1e-12)
            REQUIRE(h.pl.plannedTag != 0, "a full evaluation is a cached plan");
            got[w] = checkCompression(h, foldCaps[it % 3]);
            if (w == 1 && h.pl.lastWeighed > 0) checkWholeRunWeights(*h.pl.planned, chunk, top);
        }
        const Plan &a = *hs[0].pl.planned, &b = *hs[1].pl.planned;
        REQUIRE(a.prog.size() == b.prog.size(), "%zu micro-operations against %zu with the switch set", a.prog.size(), b.prog.size());
        bool memRuns = false;                                  // does the plan evaluate a memory definition anywhere (a run with a leaf from memory)?
        for (const PlanRun& run : b.runs) memRuns = memRuns || !plainRun(b, run);
        bool pathSteps = false;                                // ... or behind its operand's program (an unstored micro-operation outside every run)
        {
            std::vector<char> inRun(b.prog.size(), 0);
            for (const PlanRun& run : b.runs) for (int i = run.start; i < run.start + run.count; i++) inRun[(size_t)i] = 1;
            for (size_t i = 0; i < b.prog.size(); i++) pathSteps = pathSteps || (!inRun[i] && b.prog[i].storeBuf < 0);
        }
        if (!memRuns && !pathSteps) { REQUIRE(samePlan(a, b), "a plan without memory definitions differs under the switch"); g_samePlans++; }
        else if (!samePlan(a, b)) g_otherCuts++;
        if (got[0].any && got[1].any) REQUIRE(got[0].upper <= got[1].upper || !samePlan(a, b), "%d micro-operations left in the walk, %d with the switch set, of the same plan", got[0].upper, got[1].upper);
        last.on = got[0]; last.slices = (int)a.segs.size(); last.waves = wavesOf(a); last.stored = hs[0].pl.lastStored; last.weighed = hs[0].pl.lastWeighed;
        last.off = got[1]; last.slicesOff = (int)b.segs.size(); last.wavesOff = wavesOf(b); last.weighedOff = hs[1].pl.lastWeighed;
        g_lists++;
    }
    {   // the switch is part of a cached plan's identity
        Harness& h = hs[0];
        std::vector<int> ops; pr.emit(order, 2, ops);          // (the last list once more)
        const int count = (int)ops.size() / 7;
        Plan scratch;
        long hits = h.pl.cacheHits;
        REQUIRE(h.pl.plan(ops.data(), count, 7, 1, true, scratch, chunk) == 0 && h.pl.cacheHits == hits + 1, "the same list with the feature is a hit");
        h.pl.memDefTables = false;
        bool simple = false;
        REQUIRE(!h.pl.replayCached(ops.data(), count, 7, 1, true, chunk, &simple), "replayed under the switch");
        hits = h.pl.cacheHits;
        REQUIRE(h.pl.plan(ops.data(), count, 7, 1, true, scratch, chunk) == 0 && h.pl.cacheHits == hits, "the same list under the switch is a miss");
        h.pl.memDefTables = true;
    }
    return last;
}

int main() {
    unsigned seed = 1;
    for (int T : {24, 48, 200})
        for (int cat = 0; cat < 2; cat++)
            for (int defCapSeed : {7, 10})
                for (int caps = 0; caps < 3; caps++) {         // memory cap 8, 24, and 8 at first sight / 24 from the second
                    const int chunk = T == 200 ? 20 : 8;
                    scenario(T, cat != 0, T == 200 ? 40 : 129, seed, defCapSeed, caps == 1 ? 24 : 8, caps == 2 ? 24 : 0, chunk, seed % 3 == 0 ? 0 : 8, 8);
                    seed++;
                }
    printf("  %ld lists; %ld plans compressed: %ld whole runs, %ld sub-runs of %ld micro-operations; %ld plans without memory definitions the same under the switch, %ld cut or ordered differently; %ld peeled slices under the switch\n",
           g_lists, g_compressed, g_wholeRuns, g_subRuns, g_subOps, g_samePlans, g_otherCuts, g_peeled);
    REQUIRE(g_compressed > 0 && g_subRuns > 0 && g_samePlans > 0 && g_peeled > 0, "nothing was compressed, no sub-run taken, no plan compared or no slice peeled");
    // the engine's large case: 1 000 tips, definitions of up to 24 steps, chunk 64, top 8 — memory definitions of up to 8 steps for every list
    // against 8 at first sight and 24 from the second coming on
    for (unsigned big : {16u, 3u}) {
        const Outcome c8 = scenario(1000, false, 16, big, 10, 8, 0, 64, 8, 7), c24 = scenario(1000, false, 16, big, 10, 8, 24, 64, 8, 7);      // (seven lists: the last one folds by 32, as the engine does)
        printf("  1000 tips, seed %u: cap 8: %d stored, %d slices in %d waves, weight %ld, %d micro-operations left in the walk (%d of them unstored), %d sub-runs\n",
               big, c8.stored, c8.slices, c8.waves, c8.weighed, c8.on.upper, c8.on.unstored, c8.on.sub);
        printf("                       cap 24: %d stored, %d slices in %d waves, weight %ld, %d micro-operations left in the walk (%d of them unstored), %d sub-runs\n",
               c24.stored, c24.slices, c24.waves, c24.weighed, c24.on.upper, c24.on.unstored, c24.on.sub);
        printf("                       cap 24 with the switch set: %d slices in %d waves, weight %ld, %d micro-operations left in the walk (%d of them unstored)\n",
               c24.slicesOff, c24.wavesOff, c24.weighedOff, c24.off.upper, c24.off.unstored);
        static char bigWhere[80]; snprintf(bigWhere, sizeof bigWhere, "1000 tips, seed %u, cap 24 against cap 8", big); g_where = bigWhere;
        REQUIRE(c8.on.any && c24.on.any, "the 1000-tip plans are compressed");
        REQUIRE(c24.stored <= c8.stored, "%d stored nodes under the longer cap, %d under cap 8", c24.stored, c8.stored);
        // (every micro-operation left is a stored node or a step on a memory definition's path: the unstored ones are the path steps)
        REQUIRE(c24.on.upper <= c8.on.upper + c24.on.unstored, "%d micro-operations left at cap 24, %d at cap 8 plus %d path steps", c24.on.upper, c8.on.upper, c24.on.unstored);
        REQUIRE(c24.slices <= c8.slices + 1 && c24.waves <= c8.waves + 1, "%d slices in %d waves at cap 24, %d in %d at cap 8", c24.slices, c24.waves, c8.slices, c8.waves);
    }
    // chains that change the topology (plan_harness.h scenarioTopology) in this program's configuration: weighing for compression, caps 8 at first
    // sight and 24 from the second coming, sub-runs taken from the chain's one index — with the feature and with the switch set
    {
        TopologyStats topology;
        C = 2;
        for (int on = 1; on >= 0; on--)
            for (int T : {24, 48, 96}) {
                P = T == 96 ? 40 : 129;
                TopologyOptions o; o.repeats = true; o.classLimit = 65535; o.memStepCap = 8; o.memStepCapSeen = 24; o.initSeed = T == 24 ? 7 : 10; o.fixedChunk = 8; o.weights = true; o.memDefTables = on != 0;
                o.caterpillar = T == 48;
                const TopologyStats st = scenarioTopology(T, true, 40u + (unsigned)T, 60, o);
                if (!on) REQUIRE(st.subRuns == 0, "%ld sub-runs with the switch set", st.subRuns);
                topology.add(st);
            }
        topology.print("plan_check_memdef_tables");
        REQUIRE(topology.compressed > 50 && topology.subRuns > 0 && topology.cladesAcrossMoves > 0 && topology.resets == 0, "%ld plans compressed, %ld sub-runs, %ld clades behind topology moves, %ld resets", topology.compressed, topology.subRuns, topology.cladesAcrossMoves, topology.resets);
    }
    printDigest();
    printf("plan_check_memdef_tables: OK\n");
    return 0;
}
