// plan_check_repeats.cpp — repeated sub-patterns (beast-mcmc_amd/csrc/planner.h RepeatIndex, findRepeatRuns, emitRepeatPlan, RepeatRows) on
// the CPU.  TEST INFRASTRUCTURE, not product.
//
// 1. The class index against a brute-force count on random data (8..40 tips; 1, 127, 128, 129, 300 patterns; states 0..5, every code >= 4
//    "missing"; alignments that repeat and alignments that do not): patterns share a class exactly when they agree on every tip of the
//    clade, D is the number of distinct sub-patterns, the representative of a class is its smallest pattern, a second index over the same
//    data is the same index, a clade over the limit has no index and one exactly at it has, and after a subtree swap only the clades on
//    the two paths to the root are indexed again (RepeatIndex::builds).
// 2. The emitted plan, on plan_harness.h's worlds, tree, buffer protocol and index-level interpreters: every PK_TAB operand names a
//    clade that has a class-table program in the same plan, class-table programs pay no factors and store nothing but their table, the payments of the whole plan are those of the uncompressed plan (FoldMap through
//    RepeatPlan::origin), and the compressed plan — tables evaluated at the representatives, consumers reading a pattern's class row —
//    leaves every stored buffer with the bits the uncompressed plan leaves, with folding at two caps and without folding.
// 3. RepeatRows: tables start at multiples of 128 rows and stay inside one arena.
#include "plan_harness.h"
#include <string>

// ---- 1. the index ------------------------------------------------------------------------------------------------------------
struct CladeIds { std::vector<int> id; };       // RepeatIndex id of every node of a tree
static CladeIds internTree(const Tree& tree, RepeatIndex& idx) {
    const int N = 2 * tree.T - 1;
    CladeIds c; c.id.assign((size_t)N, -1);
    for (int t = 0; t < tree.T; t++) c.id[(size_t)t] = t;
    std::vector<int> order; tree.postOrder(N - 1, order);
    for (int n : order) c.id[(size_t)n] = idx.intern(c.id[(size_t)tree.left[n]], c.id[(size_t)tree.right[n]]);
    return c;
}
static void tipsBelow(const Tree& tree, int n, std::vector<int>& out) {
    std::vector<int> st{n};
    while (!st.empty()) { const int x = st.back(); st.pop_back(); if (x < tree.T) out.push_back(x); else { st.push_back(tree.left[x]); st.push_back(tree.right[x]); } }
}
static std::string subPattern(const std::vector<std::vector<uint8_t>>& tips, const std::vector<int>& below, int p) {
    std::string s;
    for (int t : below) s.push_back((char)('0' + std::min<int>(tips[(size_t)t][(size_t)p], 4)));
    return s;
}

static long g_indexNodes = 0, g_overNodes = 0;
static void checkIndex(int T, int patterns, bool divergent, unsigned seed) {
    std::mt19937 rng(seed);
    const auto tips = randomTips(T, patterns, divergent, rng);
    Tree tree; tree.random(T, rng, seed % 5 == 0);
    const int N = 2 * T - 1;
    RepeatIndex idx; idx.init(T, patterns, patterns);
    for (int t = 0; t < T; t++) idx.setTip(t, tips[(size_t)t].data());
    const CladeIds ids = internTree(tree, idx);
    REQUIRE(idx.build(ids.id[(size_t)N - 1]), "the root has an index with the limit at P");
    REQUIRE(idx.builds == T - 1, "%ld builds for %d internal nodes", idx.builds, T - 1);
    std::vector<int> distinct((size_t)N, 0);
    for (int n = T; n < N; n++) {
        const RepeatIndex::Clade& c = idx.clade(ids.id[(size_t)n]);
        REQUIRE(c.built && !c.over, "node %d", n);
        std::vector<int> below; tipsBelow(tree, n, below);
        std::sort(below.begin(), below.end());
        std::vector<int> ct(c.tips); std::sort(ct.begin(), ct.end());
        REQUIRE(ct == below, "tips of node %d", n);
        std::map<std::string, int> firstOf;
        for (int p = 0; p < patterns; p++) {
            const std::string s = subPattern(tips, below, p);
            const auto ins = firstOf.emplace(s, p);
            const int d = c.cls[(size_t)p];
            REQUIRE(d < c.D, "class %d of %d", d, c.D);
            // the class's representative is the smallest pattern with this sub-pattern, and has it on every tip
            REQUIRE(c.rep[(size_t)d] == ins.first->second, "node %d pattern %d: representative %d, first pattern with the sub-pattern %d", n, p, c.rep[(size_t)d], ins.first->second);
            REQUIRE(subPattern(tips, below, c.rep[(size_t)d]) == s, "node %d pattern %d", n, p);
        }
        REQUIRE((int)firstOf.size() == c.D, "node %d: %d classes, %zu distinct sub-patterns", n, c.D, firstOf.size());
        for (int d = 1; d < c.D; d++) REQUIRE(c.rep[(size_t)d] > c.rep[(size_t)d - 1], "classes are numbered by their first pattern");
        distinct[(size_t)n] = c.D;
        g_indexNodes++;
    }
    {   // deterministic: the same data, the same index
        RepeatIndex again; again.init(T, patterns, patterns);
        for (int t = 0; t < T; t++) again.setTip(t, tips[(size_t)t].data());
        const CladeIds ids2 = internTree(tree, again);
        again.build(ids2.id[(size_t)N - 1]);
        for (int n = T; n < N; n++) {
            const RepeatIndex::Clade &a = idx.clade(ids.id[(size_t)n]), &b = again.clade(ids2.id[(size_t)n]);
            REQUIRE(a.D == b.D && a.cls == b.cls && a.rep == b.rep, "node %d differs between two builds", n);
        }
    }
    {   // the limit: a clade with more classes has no index (nor has anything above it), one exactly at the limit has
        const int probe = T + (int)(rng() % (unsigned)(T - 1));
        const int D = distinct[(size_t)probe];
        for (int limit : {D - 1, D}) {
            if (limit < 1) continue;
            RepeatIndex lim; lim.init(T, patterns, limit);
            for (int t = 0; t < T; t++) lim.setTip(t, tips[(size_t)t].data());
            const CladeIds il = internTree(tree, lim);
            lim.build(il.id[(size_t)N - 1]);
            for (int n = T; n < N; n++) {
                bool want = true;                         // every clade below and at n within the limit
                std::vector<int> st{n};
                while (!st.empty()) { const int x = st.back(); st.pop_back(); if (x < T) continue; if (distinct[(size_t)x] > limit) want = false; st.push_back(tree.left[x]); st.push_back(tree.right[x]); }
                const RepeatIndex::Clade& c = lim.clade(il.id[(size_t)n]);
                REQUIRE(c.built && (!c.over) == want, "node %d with %d classes under a limit of %d: index %d, wanted %d", n, distinct[(size_t)n], limit, (int)!c.over, (int)want);
                REQUIRE(lim.build(il.id[(size_t)n]) == want, "build() of node %d", n);
                if (c.over) { REQUIRE(c.cls.empty() && c.D == 0, "a clade over the limit keeps nothing"); g_overNodes++; }
                else REQUIRE(c.D == distinct[(size_t)n], "node %d", n);
            }
        }
    }
    if (T >= 8) {   // a subtree swap: only the clades on the two paths to the root are indexed again
        int a = -1, b = -1;
        for (int tries = 0; tries < 1000 && a < 0; tries++) {
            const int x = (int)(rng() % (unsigned)(N - 1)), y = (int)(rng() % (unsigned)(N - 1));
            if (x == y || tree.parent[x] == tree.parent[y]) continue;
            bool nested = false;
            for (int u = tree.parent[x]; u >= 0; u = tree.parent[u]) nested = nested || u == y;
            for (int u = tree.parent[y]; u >= 0; u = tree.parent[u]) nested = nested || u == x;
            if (!nested) { a = x; b = y; }
        }
        if (a >= 0) {
            Tree t2 = tree;
            const int pa = tree.parent[a], pb = tree.parent[b];
            (t2.left[pa] == a ? t2.left[pa] : t2.right[pa]) = b;
            (t2.left[pb] == b ? t2.left[pb] : t2.right[pb]) = a;
            t2.parent[a] = pb; t2.parent[b] = pa;
            std::vector<char> onPath((size_t)N, 0);
            for (int u = pa; u >= 0; u = t2.parent[u]) onPath[(size_t)u] = 1;
            for (int u = pb; u >= 0; u = t2.parent[u]) onPath[(size_t)u] = 1;
            long expect = 0;
            for (int n = T; n < N; n++) expect += onPath[(size_t)n];
            const long before = idx.builds;
            // (post-order of the new tree: node numbers are no longer children-first)
            CladeIds c2; c2.id.assign((size_t)N, -1);
            for (int t = 0; t < T; t++) c2.id[(size_t)t] = t;
            std::vector<int> order; t2.postOrder(N - 1, order);
            for (int n : order) c2.id[(size_t)n] = idx.intern(c2.id[(size_t)t2.left[n]], c2.id[(size_t)t2.right[n]]);
            REQUIRE(idx.build(c2.id[(size_t)N - 1]), "the root after the swap");
            REQUIRE(idx.builds - before <= expect, "%ld clades indexed after a swap that changes %ld", idx.builds - before, expect);
            REQUIRE(idx.builds - before >= 1, "a swap between different parents changes at least one clade");
            for (int n = T; n < N; n++) if (!onPath[(size_t)n]) REQUIRE(c2.id[(size_t)n] == ids.id[(size_t)n], "an unchanged clade (node %d) is found again", n);
        }
    }
}

// ---- 2. the emitted plan -----------------------------------------------------------------------------------------------------
static long g_unstoredConsumers = 0;
static long g_plans = 0, g_runsTaken = 0, g_runsSeen = 0, g_twoTables = 0, g_tabFirst = 0, g_tabSecond = 0, g_memWithTable = 0, g_unparked = 0, g_noFoldTaken = 0;
static void checkCompressed(Harness& h, int limit) {
    if (h.pl.plannedTag == 0) return;                      // (only cached full-evaluation plans are compressed)
    const Plan& plan = *h.pl.planned;
    bool anyWrite = false;
    for (const MicroOp& m : plan.prog) anyWrite = anyWrite || m.smode == PS_WRITE;
    RepeatIndex idx; idx.init(h.T, P, limit);
    for (int t = 0; t < h.T; t++) if (h.compact[(size_t)t]) idx.setTip(t, h.plan.tips[(size_t)t].data());
    for (int cap : {32, 4, 0}) {                           // (0: no folding — every read-mode micro-operation pays for itself)
        FoldMap fm;
        const bool folded = cap > 0 && foldScaleFactors(plan, cap, fm);
        if (cap > 0 && !folded) { REQUIRE(anyWrite, "a read-mode plan folds"); continue; }
        std::vector<RepeatRun> cand;
        findRepeatRuns(plan, folded ? &fm : nullptr, idx, true, cand);
        if (anyWrite) { REQUIRE(cand.empty(), "a plan that rescales in write mode is left alone"); continue; }
        g_runsSeen += (long)plan.runs.size();
        if (cand.empty()) continue;
        RepeatPlan rp;
        emitRepeatPlan(plan, cand, rp);
        g_plans++; g_runsTaken += (long)cand.size();
        if (!folded) g_noFoldTaken += (long)cand.size();
        // structure
        REQUIRE(rp.plan.segs.size() == plan.segs.size() && rp.lower.size() == cand.size() && rp.origin.size() == rp.plan.prog.size(), "shape");
        REQUIRE(rp.plan.deps == plan.deps && rp.plan.launchOrder == plan.launchOrder && rp.plan.leaves == plan.leaves && rp.plan.snapPairs == plan.snapPairs, "the walk's slices keep their order and dependencies");
        std::vector<char> hasProgram;
        auto named = [&](int clade) { for (const PlanSeg& sg : rp.lower) if (sg.partition == clade) return true; return false; };
        size_t upperOps = 0, tabs = 0;
        std::vector<char> kept(plan.prog.size(), 0);
        for (size_t s = 0; s < rp.plan.segs.size(); s++) {
            const PlanSeg& sg = rp.plan.segs[s];
            REQUIRE(sg.progCount > 0 && sg.depCount == plan.segs[s].depCount && sg.next == plan.segs[s].next && sg.partition == plan.segs[s].partition, "slice %zu", s);
            for (int k = sg.progStart; k < sg.progStart + sg.progCount; k++) {
                const MicroOp& m = rp.plan.prog[(size_t)k];
                const int o = rp.origin[(size_t)k];
                REQUIRE(o >= plan.segs[s].progStart && o < plan.segs[s].progStart + plan.segs[s].progCount && !kept[(size_t)o], "origin of %d", k);
                kept[(size_t)o] = 1;
                REQUIRE(m.storeBuf == plan.prog[(size_t)o].storeBuf && m.smode == plan.prog[(size_t)o].smode && m.scaleIdx == plan.prog[(size_t)o].scaleIdx, "micro-operation %d keeps what it stores and pays", k);
                if (m.k1 == PK_TAB) { REQUIRE(named(m.a1), "table operand of %d", k); tabs++; g_tabFirst++; }
                if (m.k2 == PK_TAB) { REQUIRE(named(m.a2), "table operand of %d", k); tabs++; g_tabSecond++; }
                if (m.k1 == PK_TAB && m.k2 == PK_TAB) g_twoTables++;
                if ((m.k1 == PK_TAB && m.k2 == PK_MEM) || (m.k2 == PK_TAB && m.k1 == PK_MEM)) g_memWithTable++;
                if (m.k1 == PK_TAB && m.k2 == PK_ACC) g_unparked++;
                upperOps++;
            }
        }
        REQUIRE(tabs == cand.size() && (int)tabs == rp.tableReads, "one table operand per class-table program");
        {   // the plan's own counts of the two rarer consumers (what the engine reports: beagleMi355RepeatStats)
            int two = 0, unstored = 0;
            for (size_t k = 0; k < upperOps; k++) {
                const MicroOp& m = rp.plan.prog[k];
                if (m.k1 == PK_TAB && m.k2 == PK_TAB) two++;
                if ((m.k1 == PK_TAB || m.k2 == PK_TAB) && m.storeBuf < 0) unstored++;
            }
            REQUIRE(two == rp.twoTables && unstored == rp.unstoredConsumers, "two-table nodes %d / %d, unstored consumers %d / %d", two, rp.twoTables, unstored, rp.unstoredConsumers);
            g_unstoredConsumers += unstored;
        }
        size_t lowerOps = 0;
        for (const PlanSeg& sg : rp.lower) {
            REQUIRE(sg.progStart >= (int)upperOps && sg.depCount == 0 && sg.next < 0, "a class-table program waits for nothing");
            const RepeatIndex::Clade& c = idx.clade(sg.partition);
            REQUIRE(c.built && !c.over && c.D <= limit, "clade %d", sg.partition);
            for (int k = sg.progStart; k < sg.progStart + sg.progCount; k++) {
                const MicroOp& m = rp.plan.prog[(size_t)k];
                REQUIRE(m.storeBuf < 0 && m.smode == PS_NONE && m.k1 != PK_MEM && m.k2 != PK_MEM && m.k1 != PK_TAB && m.k2 != PK_TAB, "class-table micro-operation %d", k);
                REQUIRE(!kept[(size_t)rp.origin[(size_t)k]], "a micro-operation is in one program");
                if (folded) REQUIRE(fm.payStart[(size_t)rp.origin[(size_t)k] + 1] == fm.payStart[(size_t)rp.origin[(size_t)k]], "a class-table program pays no factors");
                else REQUIRE(plan.prog[(size_t)rp.origin[(size_t)k]].smode == PS_NONE, "a class-table program pays no factors");
                lowerOps++;
            }
        }
        REQUIRE(upperOps + lowerOps == plan.prog.size(), "every micro-operation is in exactly one program");
        if (folded) {   // the payments of the whole plan: every member list of the uncompressed plan is paid by a micro-operation of the walk
            size_t paid = 0;
            for (size_t k = 0; k < upperOps; k++) paid += (size_t)(fm.payStart[(size_t)rp.origin[k] + 1] - fm.payStart[(size_t)rp.origin[k]]);
            REQUIRE(paid == fm.members.size(), "%zu of %zu fold members are paid", paid, fm.members.size());
        }
        // values: the same stored bits as the uncompressed plan (both on copies of the planned world: the list has just run, its
        // snapshot copies are idempotent)
        World a = h.plan, b = h.plan;
        runPlan(a, plan, h.partStart, h.partEnd, folded ? &fm : nullptr);
        runCompressed(b, rp, folded ? &fm : nullptr, idx, h.partStart, h.partEnd);
        for (int buf = 0; buf < h.nBuf; buf++) {
            REQUIRE(a.partials[(size_t)buf].size() == b.partials[(size_t)buf].size(), "buffer %d", buf);
            if (!a.partials[(size_t)buf].empty()) REQUIRE(memcmp(a.partials[(size_t)buf].data(), b.partials[(size_t)buf].data(), a.partials[(size_t)buf].size() * 8) == 0, "buffer %d differs from the uncompressed plan (fold cap %d) [%s]", buf, cap, g_where);
        }
    }
}

static void scenarioRepeats(int T, int patterns, unsigned seed, int chunk, int tipPartialsAt, bool shortDefinitions = false) {
    P = patterns; C = 2;
    std::mt19937 rng(seed);
    static char where[128]; snprintf(where, sizeof where, "repeats T=%d P=%d seed=%u chunk=%d", T, patterns, seed, chunk); g_where = where; g_list = 0;
    Tree tree; tree.random(T, rng, false);
    const int N = 2 * T - 1;
    // (three hold slots; a definition cap of 24 as on large alignments, or of 8 as on small ones: many nodes over two definitions)
    Harness h; h.init(T, T + 2 * (T - 1), 2 * N, 2 * (T - 1), true, (shortDefinitions ? 7u : 10u) + 18 * (seed % 3));
    h.pl.memStepCap = 8;
    h.fixedChunk = chunk;
    const auto tips = randomTips(T, patterns, false, rng);
    for (int t = 0; t < T; t++) {
        if (t == tipPartialsAt) { h.setTipPartials(t); continue; }
        h.truth.tips[(size_t)t] = tips[(size_t)t]; h.plan.tips[(size_t)t] = tips[(size_t)t];
        h.compact[(size_t)t] = 1; h.pl.setCompactTip(t, true); h.pl.setLeafPartials(t, false);
    }
    for (int s = 0; s < 2 * N; s++) h.setMatrix(s);
    Protocol pr(tree);
    std::vector<int> lvl = tree.levelOrder();
    const int limit = std::max(1, patterns / 4);
    for (int it = 0; it < 7; it++) {
        for (int n : lvl) pr.pFlip[n] ^= 1;
        for (int n = 0; n < N - 1; n++) { pr.mFlip[n] ^= 1; h.setMatrix(pr.mBuf(n)); }
        std::vector<int> ops; pr.emit(lvl, it == 0 ? 0 : it == 1 ? 1 : 2, ops);      // no scaling, write mode, then read mode
        h.update(ops, 7);
        checkCompressed(h, limit);
    }
    if (tipPartialsAt >= 0 && h.pl.plannedTag != 0) {       // a tip with uploaded partials: no clade that holds it has a table
        const Plan& plan = *h.pl.planned;
        RepeatIndex idx; idx.init(T, P, limit);
        for (int t = 0; t < T; t++) if (h.compact[(size_t)t]) idx.setTip(t, h.plan.tips[(size_t)t].data());
        FoldMap fm; foldScaleFactors(plan, 32, fm);
        std::vector<RepeatRun> cand;
        findRepeatRuns(plan, &fm, idx, true, cand);
        for (const RepeatRun& r : cand) for (int t : idx.clade(r.clade).tips) REQUIRE(t != tipPartialsAt, "a clade over a tip with uploaded partials is compressed");
    }
}

// The index forgets nothing clade by clade; its owner drops it at its capacity.  A long chain of subtree swaps, driven as the engine drives
// it (engine_walk.cpp prepareRepeats): the number of clades and the bytes stay bounded, and every list still gets its index.
static void checkCapacity() {
    const int T = 24, patterns = 300, N = 2 * T - 1;
    std::mt19937 rng(9);
    const auto tips = randomTips(T, patterns, false, rng);
    RepeatIndex idx; idx.init(T, patterns, patterns);
    REQUIRE(idx.capacity() == (size_t)8 * T + 1024, "default capacity %zu", idx.capacity());
    idx.setCapacity(200);
    for (int t = 0; t < T; t++) idx.setTip(t, tips[(size_t)t].data());
    size_t most = 0, mostBytes = 0; long resets = 0, interned = 0;
    for (int move = 0; move < 2000; move++) {
        Tree tree; tree.random(T, rng, false);            // (a new topology every time: far more new clades than a swap makes)
        if (idx.overCapacity()) { idx.clear(); resets++; }
        const size_t before = idx.size();
        const CladeIds ids = internTree(tree, idx);
        interned += (long)(idx.size() - before);
        REQUIRE(idx.build(ids.id[(size_t)N - 1]), "move %d: the root has its index", move);
        most = std::max(most, idx.size()); mostBytes = std::max(mostBytes, idx.bytes());
    }
    REQUIRE(interned > 20000 && resets > 50, "the chain made %ld clades and %ld resets", interned, resets);
    REQUIRE(most <= 200 + (size_t)(T - 1), "%zu clades kept under a capacity of 200 and lists of %d", most, T - 1);
    REQUIRE(mostBytes <= (200 + (size_t)T) * ((size_t)patterns * 2 + 4096), "%zu bytes kept", mostBytes);
    printf("  capacity: %ld clades made over 2000 topologies, %ld resets, %zu kept at most (%zu bytes)\n", interned, resets, most, mostBytes);
}

int main() {
    checkCapacity();
    {
        int k = 0;
        for (int patterns : {1, 127, 128, 129, 300})
            for (int T : {8, 13, 24, 40})
                for (int div = 0; div < 2; div++) checkIndex(T, patterns, div != 0, 100u + (unsigned)(k++));
        printf("  index: %ld clades against brute force, %ld over a limit\n", g_indexNodes, g_overNodes);
        REQUIRE(g_overNodes > 0, "the limit was never exceeded");
    }
    {   // RepeatRows: whole groups of 128 rows, inside one arena
        RepeatRows rows; rows.init(2, 300);
        int arena = -1, row = -1;
        REQUIRE(rows.place(1, arena, row) && arena == 0 && row == 0, "first table");
        REQUIRE(rows.place(129, arena, row) && arena == 1 && row == 0, "a table of two groups does not straddle arenas (arena %d row %d)", arena, row);
        REQUIRE(!rows.place(100, arena, row), "two groups of the second arena's 300 rows are taken: a third does not fit");
        REQUIRE(!rows.place(301, arena, row) && !rows.place(0, arena, row), "a table no arena holds");
        rows.init(3, 1000);
        for (int i = 0; i < 40; i++) {
            const int D = 1 + (i * 37) % 260;
            if (!rows.place(D, arena, row)) break;
            REQUIRE(row % 128 == 0 && row + ((D + 127) & ~127) <= 1000 && arena < 3, "table %d: arena %d row %d", i, arena, row);
        }
    }
    unsigned seed = 1;
    for (int T : {24, 40})
        for (int patterns : {129, 300})
            for (int chunk : {0, 8}) { scenarioRepeats(T, patterns, seed, chunk, -1); seed++; }
    for (int T : {24, 48})
        for (int chunk : {0, 8}) { scenarioRepeats(T, 300, seed, chunk, -1, true); seed++; }
    scenarioRepeats(24, 300, 77, 0, 5);
    // chains that change the topology (plan_harness.h scenarioTopology): ONE index through the chain, every cached read-mode plan run compressed,
    // a capacity small enough that the index is dropped in the middle of the chain — and one chain under the default capacity, which never is
    {
        TopologyStats topology;
        C = 2;
        for (unsigned s : {1u, 2u})
            for (int T : {24, 48}) {
                P = T == 24 ? 129 : 300;
                TopologyOptions o; o.repeats = true; o.classLimit = std::max(1, P / 2); o.capacity = (size_t)T; o.memStepCap = 8; o.memStepCapSeen = s == 1 ? 24 : 0;
                o.initSeed = s == 1 && T == 48 ? 10 : 7; o.fixedChunk = s == 1 ? 8 : 0; o.weights = true;      // (definition cap 24 on 48 tips, else 8: under 24, a 24-tip tree stores nothing)
                topology.add(scenarioTopology(T, true, 700 * s + (unsigned)T, 60, o));
            }
        P = 129;
        { TopologyOptions o; o.repeats = true; o.classLimit = 64; o.memStepCap = 8; o.memStepCapSeen = 24; o.initSeed = 7; o.fixedChunk = 8; o.weights = true;
          const TopologyStats st = scenarioTopology(24, true, 33, 60, o); REQUIRE(st.resets == 0, "%ld resets under the default capacity", st.resets); topology.add(st); }
        topology.print("plan_check_repeats");
        REQUIRE(topology.compressed > 50 && topology.cladesAcrossMoves > 0 && topology.resets >= 4, "%ld plans compressed, %ld clades behind topology moves, %ld resets", topology.compressed, topology.cladesAcrossMoves, topology.resets);
    }
    printf("  plans: %ld compressed, %ld of %ld definition runs taken (%ld without folding); table operands first %ld / second %ld, two-table nodes %ld, "
           "stored sibling of a table %ld, parked siblings freed %ld\n", g_plans, g_runsTaken, g_runsSeen, g_noFoldTaken, g_tabFirst, g_tabSecond, g_twoTables, g_memWithTable, g_unparked);
    REQUIRE(g_plans > 0 && g_runsTaken > 0 && g_noFoldTaken > 0, "nothing was compressed");
    REQUIRE(g_tabFirst > 0 && g_tabSecond > 0 && g_twoTables > 0, "no node with two table children was seen");
    REQUIRE(g_unstoredConsumers > 0, "no memory definition with a table clade as its other child was seen");
    printf("  memory definitions over a table clade: %ld\n", g_unstoredConsumers);
    printDigest();
    printf("plan_check_repeats: OK\n");
    return 0;
}
