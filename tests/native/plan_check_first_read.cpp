// plan_check_first_read.cpp — long memory definitions stored when a list first reads them (beast-mcmc_amd/csrc/planner.h
// longMemoryOperands; the engine's use of it: engine_walk.cpp runOperationsWalk), on the CPU.  TEST INFRASTRUCTURE, not product.
//
// The worlds, the interpreter, the tree and the buffer-index protocol are plan_harness.h's.  Chains of
// full evaluations and branch moves — half of them rejected — are driven as the engine drives them: before a list that is not a full
// evaluation is planned, the planner names the memory definitions of more than `minSteps` steps that the list reads as a child without
// writing them or their stored operand, and they are materialised.  Asserted:
//   * the set named is exactly that (recomputed here from the definitions), without duplicates;
//   * every materialised buffer, and after every list every real buffer and scale buffer, agrees BITWISE with list-order evaluation;
//   * a definition stored this way is not named again by later moves until a list has defined its buffer again, and the moves of a
//     chain walk fewer micro-operations than those of the same chain with the threshold at the cap (never);
//   * the two caps (planner.h memStepCapSeen): a closed list is planned under memStepCap when it is first seen and once more, under the longer
//     cap, when it comes the second time — fewer stored nodes —, and from the third time on it is replayed from the plan cache; a move's
//     list never makes a memory definition longer than memStepCap; with preferSeenCap set a new closed list stores no more nodes than
//     the lists that had come again.
#include "plan_harness.h"

static long g_named = 0, g_namedAgain = 0;

struct MoveChain {
    Tree tree; int T, N;
    Harness h;
    Protocol* pr = nullptr;
    std::vector<int> all;
    std::mt19937 rng;
    int minSteps = 0;
    long moveMicro = 0;
    std::vector<char> storedSinceFull;                  // per buffer: materialised on a first read since the last full evaluation
    ~MoveChain() { delete pr; }
    void init(int tips, bool caterpillar, unsigned seed, int vcap, int memCap, int seenCap, int chunk, int inlineSteps) {
        rng.seed(seed);
        T = tips; N = 2 * T - 1; minSteps = inlineSteps;
        tree.random(T, rng, caterpillar);
        h.init(T, T + 2 * (T - 1), 2 * N, 2 * (T - 1), true, seed + 1);
        h.pl.init(h.nBuf, T, 2 * N, 2 * (T - 1), vcap, true, 3);
        h.pl.chunkTopOps = chunk > 0 ? 8 : 0; h.pl.launchMachines = 3.0;
        h.pl.memStepCap = memCap; h.pl.memStepCapSeen = seenCap;
        for (World* w : {&h.truth, &h.plan}) w->mats.assign(h.pl.matrixSlots(), std::vector<double>((size_t)C * 16, 0.0));
        h.fixedChunk = chunk;
        for (int i = 0; i < T; i++) h.setTipStates(i);
        for (int s = 0; s < 2 * N; s++) h.setMatrix(s);
        pr = new Protocol(tree);
        tree.postOrder(N - 1, all);
        storedSinceFull.assign(h.nBuf, 0);
    }
    void full(int mode) {
        for (int n : all) pr->pFlip[n] ^= 1;
        for (int n = 0; n < N - 1; n++) { pr->mFlip[n] ^= 1; h.setMatrix(pr->mBuf(n)); }
        std::vector<int> ops; pr->emit(all, mode, ops);
        std::vector<int> need;
        h.pl.longMemoryOperands(ops.data(), (int)(ops.size() / 7), 7, minSteps, need);
        if (!need.empty()) { fprintf(stderr, "a full evaluation reads nothing from outside, yet %zu definitions were named [%s]\n", need.size(), g_where); exit(1); }
        h.update(ops, 7);
        std::fill(storedSinceFull.begin(), storedSinceFull.end(), 0);
    }
    // what longMemoryOperands must name, from the definitions themselves
    std::vector<int> expected(const std::vector<int>& ops) const {
        const int count = (int)(ops.size() / 7);
        std::vector<char> written(h.nBuf, 0);
        for (int k = 0; k < count; k++) written[ops[(size_t)k * 7]] = 1;
        std::vector<int> out;
        for (int k = 0; k < count; k++)
            for (int c : {ops[(size_t)k * 7 + 3], ops[(size_t)k * 7 + 5]}) {
                if (!h.pl.isVirtualKey(c) || written[c]) continue;
                const VirtDef& v = h.pl.definition(c);
                if (v.memKey < 0 || v.nSteps <= minSteps || written[v.memKey]) continue;
                if (std::find(out.begin(), out.end(), c) == out.end()) out.push_back(c);
            }
        return out;
    }
    void branchMove(bool reject) {
        pr->store();
        std::vector<char> dirty(N, 0);
        const int n = rng() % (N - 1);
        pr->mFlip[n] ^= 1; h.setMatrix(pr->mBuf(n));
        for (int a = tree.parent[n]; a >= 0; a = tree.parent[a]) dirty[a] = 1;
        std::vector<int> nodes;
        for (int x : all) if (dirty[x]) nodes.push_back(x);
        for (int x : nodes) pr->pFlip[x] ^= 1;
        std::vector<int> ops; pr->emit(nodes, 2, ops);
        std::vector<int> need, want = expected(ops);
        h.pl.longMemoryOperands(ops.data(), (int)(ops.size() / 7), 7, minSteps, need);
        if (minSteps >= h.pl.memCapSeen()) want.clear();                                                  // (at the cap: never)
        std::vector<int> a = need, b = want;
        std::sort(a.begin(), a.end()); std::sort(b.begin(), b.end());
        if (a != b || std::adjacent_find(a.begin(), a.end()) != a.end()) {
            fprintf(stderr, "a move's list: %zu definitions named, %zu expected [%s, list %ld]\n", need.size(), want.size(), g_where, g_list); exit(1);
        }
        for (int x : need) { if (storedSinceFull[x]) g_namedAgain++; storedSinceFull[x] = 1; g_named++; }
        h.materialiseKeys(need);                         // (compares every one of them with list-order evaluation)
        for (int x : need) if (h.pl.isVirtualKey(x)) { fprintf(stderr, "buffer %d is still a definition after its materialisation [%s]\n", x, g_where); exit(1); }
        const long before = h.micro;
        h.update(ops, 7);
        moveMicro += h.micro - before;
        for (int k = 0; k < (int)(ops.size() / 7); k++) {       // (a partial update is planned under the first-sight cap)
            const int d = ops[(size_t)k * 7];
            if (h.pl.isVirtualKey(d) && h.pl.definition(d).memKey >= 0 && h.pl.definition(d).nSteps > h.pl.memStepCap) {
                fprintf(stderr, "a move's list made a memory definition of %d steps under a cap of %d [%s, list %ld]\n", h.pl.definition(d).nSteps, h.pl.memStepCap, g_where, g_list); exit(1);
            }
        }
        for (int k = 0; k < (int)(ops.size() / 7); k++) storedSinceFull[ops[(size_t)k * 7]] = 0;      // (a destination is defined anew)
        if (reject) pr->restore();
    }
    void finish() {
        std::vector<int> every; for (int b = T; b < h.nBuf; b++) every.push_back(b);
        h.materialise(every);
        h.compareAll();
    }
};

static long g_promoted = 0, g_atOnce = 0;
static long scenario(int T, bool caterpillar, unsigned seed, int vcap, int memCap, int seenCap, int chunk, int inlineSteps) {
    static char where[160]; snprintf(where, sizeof where, "first read T=%d cat=%d seed=%u vcap=%d memcap=%d/%d chunk=%d inline=%d", T, (int)caterpillar, seed, vcap, memCap, seenCap, chunk, inlineSteps); g_where = where; g_list = 0;
    MoveChain c; c.init(T, caterpillar, seed, vcap, memCap, seenCap, chunk, inlineSteps);
    c.full(0); c.full(1);
    // read mode: two lists alternate (both buffer flips).  First sight, first sight, second sight twice (planned again), then the cache
    long stored[6], hits[6];
    for (int it = 0; it < 6; it++) { c.full(2); stored[it] = c.h.pl.lastStored; hits[it] = c.h.pl.cacheHits; }
    if (T >= 16) {
        const bool two = seenCap > memCap && memCap > 0;
        if (hits[3] != hits[1] + (two ? 0 : 2) || hits[5] != hits[3] + 2 || stored[4] != stored[2] || stored[5] != stored[3] || stored[2] > stored[0] || stored[3] > stored[1]) {
            fprintf(stderr, "second sight: stored %ld %ld %ld %ld %ld %ld, cache hits %ld %ld %ld %ld %ld %ld [%s]\n", stored[0], stored[1], stored[2], stored[3], stored[4], stored[5],
                    hits[0], hits[1], hits[2], hits[3], hits[4], hits[5], g_where); exit(1);
        }
        if (two && stored[2] < stored[0]) g_promoted++;
    }
    for (int step = 0; step < 40; step++) {
        c.branchMove(step % 2 == 1);
        if (step % 10 == 9) c.full(2);
    }
    // a new closed list while the caller says that full evaluations are all it is asked for: the long cap at once (planner.h preferSeenCap)
    if (T >= 16) {
        for (int q = 0; q < 3; q++) c.branchMove(false);
        c.full(2);
        const long firstSight = c.h.pl.lastStored;
        for (int q = 0; q < 3; q++) c.branchMove(false);
        c.h.pl.preferSeenCap = true;
        const long hitsBefore = c.h.pl.cacheHits;
        c.full(2);
        c.h.pl.preferSeenCap = false;
        if (c.h.pl.cacheHits == hitsBefore) {            // (planned, not replayed)
            if (c.h.pl.lastStored > std::max(stored[4], stored[5])) { fprintf(stderr, "at once: %ld stored nodes, %ld / %ld when the list had come again [%s]\n", (long)c.h.pl.lastStored, stored[4], stored[5], g_where); exit(1); }
            if (c.h.pl.lastStored < firstSight) g_atOnce++;
        }
    }
    c.finish();
    return c.moveMicro;
}

int main() {
    for (unsigned seed : {1u, 2u})
        for (int T : {13, 40, 150, 400})
            for (int chunk : {0, 20}) {
                if (T == 400 && (seed == 1 || chunk == 0)) continue;      // (the largest tree once: two caps, in slices)
                const int vcap = T >= 150 ? 24 : 8, seenCap = vcap, memCap = seed == 1 ? vcap : vcap / 3;      // (seed 1: one cap for every list)
                const long never = scenario(T, false, 100 * seed + T, vcap, memCap, seenCap, chunk, seenCap);
                for (int inlineSteps : {0, 8}) {
                    if (inlineSteps >= seenCap) continue;
                    const long namedBefore = g_named;
                    const long on = scenario(T, false, 100 * seed + T, vcap, memCap, seenCap, chunk, inlineSteps);
                    printf("  T=%d seed=%u chunk=%d caps %d / %d, stored past %d steps: %ld definitions stored on a first read; the moves' micro-operations %ld (never: %ld)\n",
                           T, seed, chunk, memCap, seenCap, inlineSteps, g_named - namedBefore, on, never);
                    if (on > never) { fprintf(stderr, "the moves walk more micro-operations than with the threshold at the cap\n"); return 1; }
                }
            }
    for (int inlineSteps : {0, 8}) {
        const long never = scenario(200, true, 5, 24, 8, 24, 0, 24), on = scenario(200, true, 5, 24, 8, 24, 0, inlineSteps);
        printf("  caterpillar T=200, stored past %d steps: the moves' micro-operations %ld (never: %ld)\n", inlineSteps, on, never);
        if (on > never) { fprintf(stderr, "caterpillar: the moves walk more micro-operations\n"); return 1; }
    }
    printf("definitions stored on a first read: %ld; named a second time before a list defined them again: %ld\n", g_named, g_namedAgain);
    printf("chains whose lists stored fewer nodes when they came the second time: %ld\n", g_promoted);
    printf("new lists planned under the long cap at once that stored fewer nodes than a first sight: %ld\n", g_atOnce);
    if (g_named < 100 || g_namedAgain != 0 || g_promoted < 10 || g_atOnce < 10) { fprintf(stderr, "first-read storing or the second-sight cap was hardly exercised, or a stored definition was named again\n"); return 1; }
    printDigest();
    printf("plan_check_first_read: OK\n");
    return 0;
}
