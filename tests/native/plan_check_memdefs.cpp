// plan_check_memdefs.cpp — the walk planner's MEMORY definitions (beast-mcmc_amd/csrc/planner.h memStepCap) against list-order
// evaluation, on the CPU.  TEST INFRASTRUCTURE, not product.
//
// The two worlds, the index-level interpreter of the walk kernel's register model, the tree and BEAST's buffer-index protocol are
// plan_harness.h's; what is new here is the planner setting — WalkPlanner::memStepCap > 0, which
// plan_check.cpp leaves at 0 — and what is asserted on top of bitwise equality with list-order evaluation:
//   * no definition reads more than one stored internal node, and one that reads one has at most memStepCap steps;
//   * a program never reads back a buffer its own slice stores, except as the first child of a micro-operation that stores itself (the
//     rule a stored parent short of hold slots has always had) — a memory definition takes the operand its program has just produced
//     from ACC or a hold slot;
//   * fewer nodes are stored than with memStepCap = 0;
//   * a list that overwrites a stored operand without redefining the definition that reads it finds that definition in the
//     materialise-before set, and the definition keeps the value from before the overwrite.
#include "plan_harness.h"

static long g_memDefs = 0, g_inlineEvaluations = 0, g_memoryEvaluations = 0, g_forcedBefore = 0;

// the stored internal operands of a definition (a leaf read from memory that is no uploaded tip)
static int storedOperands(const WalkPlanner& pl, const VirtDef& v) {
    int n = 0;
    for (int s = 0; s < v.nSteps; s++) {
        const VirtStep& h = v.steps[s];
        if (h.tipA >= 0 && h.memA && !pl.leafPartials[h.tipA]) n++;
        if (h.tipB >= 0 && h.memB && !pl.leafPartials[h.tipB]) n++;
    }
    return n;
}

static void checkDefinitions(const Harness& h, int memCap = -1) {      // memCap: the cap in force (default: memStepCap)
    if (memCap < 0) memCap = h.pl.memStepCap;
    for (int b = 0; b < h.nBuf; b++) {
        if (!h.pl.isVirtualKey(b)) continue;
        const VirtDef& v = h.pl.definition(b);
        const int n = storedOperands(h.pl, v);
        if (n > 1 || (n == 1) != (v.memKey >= 0) || (n == 1 && v.nSteps > memCap)) {
            fprintf(stderr, "definition of buffer %d: %d stored operands, memKey %d, %d steps under a cap of %d [%s, list %ld]\n", b, n, v.memKey, v.nSteps, memCap, g_where, g_list);
            exit(1);
        }
        if (n == 1) {
            const VirtStep& s = v.steps[v.memStep];
            const bool there = (s.type == VT_CHERRY && ((s.memA && s.tipA == v.memKey) || (s.memB && s.tipB == v.memKey))) || (s.type == VT_EXTEND && s.memB && s.tipB == v.memKey);
            if (!there || h.pl.isVirtualKey(v.memKey)) { fprintf(stderr, "definition of buffer %d: operand %d not at step %d, or not stored [%s, list %ld]\n", b, v.memKey, v.memStep, g_where, g_list); exit(1); }
            g_memDefs++;
        }
    }
}

// no slice reads back what it stores itself, but for a storing micro-operation's first child
static void checkNoReadBack(const Plan& p) {
    for (const PlanSeg& sg : p.segs) {
        std::vector<int> storedHere;
        for (int k = sg.progStart; k < sg.progStart + sg.progCount; k++) {
            const MicroOp& m = p.prog[k];
            auto mine = [&](int b) { return std::find(storedHere.begin(), storedHere.end(), b) != storedHere.end(); };
            CHECK(!(m.k2 == PK_MEM && mine(m.a2)), m, k);
            CHECK(!(m.k1 == PK_MEM && mine(m.a1) && m.storeBuf < 0), m, k);
            if (m.storeBuf >= 0) storedHere.push_back(m.storeBuf);
        }
    }
}

// how the last plan evaluated its memory definitions: an unstored micro-operation that takes a stored result of the same slice from ACC or a
// hold slot (inline), or reads a stored internal buffer (from memory)
static void countEvaluations(const Harness& h, const Plan& p) {
    for (size_t k = 0; k < p.prog.size(); k++) {
        const MicroOp& m = p.prog[k];
        if (m.storeBuf >= 0) continue;
        if (m.k1 == PK_MEM && m.a1 >= h.T && !h.pl.leafPartials[m.a1]) g_memoryEvaluations++;
        if (m.k2 == PK_ACC && k > 0 && p.prog[k - 1].storeBuf >= 0) g_inlineEvaluations++;
    }
}

static void update(Harness& h, const std::vector<int>& ops) {
    h.update(ops, 7);
    checkDefinitions(h);
    if (h.pl.plannedTag == 0) return;                    // (a list outside the plan cache: its program was the harness's own and is gone)
    checkNoReadBack(*h.pl.planned);
    countEvaluations(h, *h.pl.planned);
}

struct Chain {
    Tree tree; int T, N;
    Harness h;
    Protocol* pr = nullptr;
    std::vector<int> all, lvl;
    std::mt19937 rng;
    ~Chain() { delete pr; }
    void init(int tips, bool caterpillar, unsigned seed, int vcap, int memCap, int holdSlots, int chunk, bool tipPartials) {
        rng.seed(seed);
        T = tips; N = 2 * T - 1;
        tree.random(T, rng, caterpillar);
        h.init(T, T + 2 * (T - 1), 2 * N, 2 * (T - 1), true, seed + 1);
        h.pl.init(h.nBuf, T, 2 * N, 2 * (T - 1), vcap, true, holdSlots);       // (the settings this test is about, not the seed's)
        h.pl.chunkTopOps = chunk > 0 ? 8 : 0; h.pl.launchMachines = 3.0;
        h.pl.memStepCap = memCap;
        for (World* w : {&h.truth, &h.plan}) w->mats.assign(h.pl.matrixSlots(), std::vector<double>((size_t)C * 16, 0.0));
        h.fixedChunk = chunk;
        for (int i = 0; i < T; i++) { if (tipPartials && i % 9 == 4) h.setTipPartials(i); else h.setTipStates(i); }
        for (int s = 0; s < 2 * N; s++) h.setMatrix(s);
        pr = new Protocol(tree);
        tree.postOrder(N - 1, all);
        lvl = tree.levelOrder();
    }
    void full(int mode, bool level) {                   // every node flips, every branch gets a new matrix
        const std::vector<int>& order = level ? lvl : all;
        for (int n : order) pr->pFlip[n] ^= 1;
        for (int n = 0; n < N - 1; n++) { pr->mFlip[n] ^= 1; h.setMatrix(pr->mBuf(n)); }
        std::vector<int> ops; pr->emit(order, mode, ops);
        update(h, ops);
    }
    void branchMove(bool reject, bool level) {
        pr->store();
        std::vector<char> dirty(N, 0);
        const int n = rng() % (N - 1);
        pr->mFlip[n] ^= 1; h.setMatrix(pr->mBuf(n));
        for (int a = tree.parent[n]; a >= 0; a = tree.parent[a]) dirty[a] = 1;
        std::vector<int> nodes;
        for (int x : (level ? lvl : all)) if (dirty[x]) nodes.push_back(x);
        for (int x : nodes) pr->pFlip[x] ^= 1;
        std::vector<int> ops; pr->emit(nodes, 2, ops);
        update(h, ops);
        if (reject) pr->restore();
    }
    void finish() {
        std::vector<int> every; for (int b = T; b < h.nBuf; b++) every.push_back(b);
        h.materialise(every);
        h.compareAll();
    }
};

// full evaluations on flipped indices, branch moves with rejections, a rescaling cycle, random materialisations, a changed tip
static long scenarioChain(int T, bool caterpillar, unsigned seed, int vcap, int memCap, int holdSlots, int chunk, bool level, bool tipPartials) {
    static char where[160]; snprintf(where, sizeof where, "memdefs chain T=%d cat=%d seed=%u vcap=%d memcap=%d hold=%d chunk=%d level=%d", T, (int)caterpillar, seed, vcap, memCap, holdSlots, chunk, (int)level); g_where = where; g_list = 0;
    Chain c; c.init(T, caterpillar, seed, vcap, memCap, holdSlots, chunk, tipPartials);
    c.full(0, level);
    c.full(1, level);                                    // the rescaling evaluation ...
    for (int it = 0; it < 4; it++) c.full(2, level);     // ... and the read-mode ones behind it: from the third on out of the plan cache
    const long storedFull = c.h.pl.lastStored;
    for (int step = 0; step < 12; step++) {
        c.branchMove(step % 3 == 1, level);
        if (step % 4 == 2) c.full(2, level);
        if (step % 4 == 3) { std::vector<int> xs; for (int q = 0; q < 3; q++) xs.push_back(T + c.rng() % (2 * (T - 1))); c.h.materialise(xs); }
        if (step == 5) c.full(1, level);                 // a second rescaling cycle, into the other scale-buffer set
    }
    // a changed tip below a memory definition: its users are materialised from the OLD states (and compared), the path is re-evaluated
    for (int b = T; b < c.h.nBuf; b++) {
        if (!c.h.pl.isVirtualKey(b) || c.h.pl.definition(b).memKey < 0) continue;
        const VirtDef& v = c.h.pl.definition(b);
        int tip = -1;
        for (int s = 0; s < v.nSteps && tip < 0; s++) { if (v.steps[s].tipA >= 0 && !v.steps[s].memA) tip = v.steps[s].tipA; else if (v.steps[s].tipB >= 0 && !v.steps[s].memB) tip = v.steps[s].tipB; }
        if (tip < 0) continue;
        c.h.setTipStates(tip);
        if (c.h.pl.isVirtualKey(b)) { fprintf(stderr, "buffer %d is still defined over tip %d after its states changed [%s]\n", b, tip, g_where); exit(1); }
        break;
    }
    c.full(2, level); c.full(2, level);
    c.finish();
    return storedFull;
}

// A list that rewrites a stored operand WITHOUT redefining the definition that reads it: the definition must be in the materialise-before
// set and keep the value from before the overwrite (BEAGLE: a buffer keeps the value its operation gave it).
static void scenarioOverwrite(int T, bool caterpillar, unsigned seed) {
    static char where[96]; snprintf(where, sizeof where, "memdefs overwrite T=%d cat=%d seed=%u", T, (int)caterpillar, seed); g_where = where; g_list = 0;
    Chain c; c.init(T, caterpillar, seed, 6, 4, 3, 0, false);
    c.full(1, false); c.full(2, false);
    int user = -1, operand = -1;
    for (int b = T; b < c.h.nBuf && user < 0; b++)
        if (c.h.pl.isVirtualKey(b) && c.h.pl.definition(b).memKey >= 0) { user = b; operand = c.h.pl.definition(b).memKey; }
    if (user < 0) { fprintf(stderr, "no memory definition to overwrite the operand of [%s]\n", g_where); exit(1); }
    const std::vector<int> ops = {operand, -1, -1, 0, 0, 1, 2};          // operand = node(tip 0, tip 1): nothing of the tree
    std::vector<int> need;
    c.h.pl.mustMaterializeBefore(ops.data(), 1, 7, need);
    if (std::find(need.begin(), need.end(), user) == need.end()) { fprintf(stderr, "buffer %d reads %d and is not materialised before %d is overwritten [%s]\n", user, operand, operand, g_where); exit(1); }
    g_forcedBefore++;
    update(c.h, ops);                                    // (the harness drives the planner as the engine does: it materialises `need` itself)
    if (c.h.pl.isVirtualKey(user)) { fprintf(stderr, "buffer %d is still a definition over the overwritten %d [%s]\n", user, operand, g_where); exit(1); }
    c.h.compareRange(user, 0, P, "kept across the overwrite of its operand");
    // ... and a branch move that leaves a reader of a full evaluation's destination behind, then that evaluation again out of the cache
    c.branchMove(true, false); c.full(2, false); c.branchMove(false, false); c.full(2, false); c.full(2, false);
    c.finish();
}

// what update() above asserts, behind every list of a topology chain (a closed list that has come twice is planned under memStepCapSeen)
static void afterTopologyList(Harness& h) {
    checkDefinitions(h, h.pl.memCapSeen());
    if (h.pl.plannedTag == 0) return;
    checkNoReadBack(*h.pl.planned);
    countEvaluations(h, *h.pl.planned);
}

int main() {
    // chains that change the topology (plan_harness.h scenarioTopology) with memory definitions as the engine sets them: 8 steps when a
    // closed list is first seen, 24 when it comes again; definition caps 8 and 24, two and three hold slots, in slices and in one piece
    {
        TopologyStats topology;
        const long seenBefore = g_memDefs;
        for (unsigned seed : {1u, 2u})
            for (int T : {9, 40, 150})
                for (int initSeed : {7, 10, 1}) {                // (Harness::init: definition cap 8 / 24 with three hold slots, 8 with two)
                    TopologyOptions o; o.memStepCap = 8; o.memStepCapSeen = 24; o.initSeed = initSeed; o.fixedChunk = (seed + (unsigned)T) % 2 ? 8 : 0; o.afterList = afterTopologyList;
                    topology.add(scenarioTopology(T, true, 500 * seed + (unsigned)T + (unsigned)initSeed, 60, o));
                }
        { TopologyOptions o; o.memStepCap = 8; o.memStepCapSeen = 24; o.initSeed = 10; o.fixedChunk = 20; o.caterpillar = true; o.afterList = afterTopologyList; topology.add(scenarioTopology(80, true, 91, 60, o)); }
        { TopologyOptions o; o.memStepCap = 8; o.memStepCapSeen = 24; o.initSeed = 10; o.fixedChunk = 8; o.mixStepLimit = true; o.afterList = afterTopologyList; topology.add(scenarioTopology(40, true, 92, 60, o)); }
        for (int T : {40, 150}) { TopologyOptions o; o.memStepCap = 8; o.memStepCapSeen = 24; o.initSeed = 10; o.fixedChunk = 8; o.afterList = afterTopologyList; topologyWithoutPlanCache(T, 93u + (unsigned)T, 60, o); }
        topology.print("plan_check_memdefs");
        printf("  memory definitions seen in topology chains: %ld\n", g_memDefs - seenBefore);
        if (g_memDefs - seenBefore < 1000 || topology.closedAgain < 10 || topology.rejectedTopology < 10) { fprintf(stderr, "the topology chains hardly met memory definitions\n"); return 1; }
    }
    // (T, caterpillar): stored nodes of a full evaluation with and without memory definitions, same tree, same settings
    for (unsigned seed : {1u, 2u, 3u}) {
        for (int T : {3, 5, 8, 13, 40, 150, 400}) {
            for (int chunk : {0, 20}) {
                const int vcap = T >= 150 ? 24 : 6, memCap = seed == 1 ? vcap : seed == 2 ? vcap / 2 : 4;
                const int hold = seed == 3 ? 2 : 3;
                const long off = scenarioChain(T, false, 100 * seed + T, vcap, 0, hold, chunk, seed == 2, seed == 3);
                const long on = scenarioChain(T, false, 100 * seed + T, vcap, memCap, hold, chunk, seed == 2, seed == 3);
                printf("  T=%d seed=%u chunk=%d cap %d / memory cap %d, %d hold slots: %ld stored nodes per full evaluation, %ld with memory definitions\n", T, seed, chunk, vcap, memCap, hold, off, on);
                if (on > off || (T >= 40 && on >= off)) { fprintf(stderr, "memory definitions did not reduce the stored nodes\n"); return 1; }
            }
        }
        scenarioOverwrite(40, false, 7 + seed);
        scenarioOverwrite(60, true, 17 + seed);
    }
    // a 200-tip caterpillar: every spine node has one stored (or memory-defined) child and a tip
    for (int memCap : {4, 8, 24}) {
        const long off = scenarioChain(200, true, 5, 24, 0, 3, 0, false, false);
        const long on = scenarioChain(200, true, 5, 24, memCap, 3, 0, false, false);
        const long onChunked = scenarioChain(200, true, 5, 24, memCap, 3, 20, true, false);
        printf("  caterpillar T=200, memory cap %d: %ld stored nodes per full evaluation, %ld with memory definitions (%ld in slices)\n", memCap, off, on, onChunked);
        // (without, every spine node above the first 24 is stored: 175; with, one in memCap + 1 of them)
        if (off < 170 || on * (memCap + 1) > 176 + 2 * (memCap + 1) || onChunked > on + 12) { fprintf(stderr, "caterpillar: %ld stored nodes\n", on); return 1; }
    }
    printf("memory definitions seen: %ld; micro-operations behind their operand's own program: %ld, reading a stored node from memory: %ld; forced before an overwrite: %ld\n",
           g_memDefs, g_inlineEvaluations, g_memoryEvaluations, g_forcedBefore);
    if (g_memDefs < 1000 || g_inlineEvaluations < 1000 || g_memoryEvaluations < 100 || g_forcedBefore < 6) { fprintf(stderr, "memory definitions were hardly exercised\n"); return 1; }
    printDigest();
    printf("plan_check_memdefs: OK\n");
    return 0;
}
