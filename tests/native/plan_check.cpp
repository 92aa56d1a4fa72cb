// plan_check.cpp — CPU check of the walk planner (beast-mcmc_amd/csrc/planner.cpp).  TEST INFRASTRUCTURE, not product.
//
// Two worlds are driven by the same sequence of BEAGLE-style calls:
//   truth   every buffer index is real storage; an operation list is evaluated in list order, one op after the other
//           (the semantics of lib/beagle.jar!beagle/GeneralBeagleImpl#updatePartials)
//   planned the planner's micro-operation programs are executed by an index-level interpreter of the walk kernel's
//           register model (ACC + two hold slots per (pattern, category)); virtual buffers hold no data
// After every list all real buffers and scale buffers must agree BITWISE; virtual buffers are compared when they are
// materialised (at random, and all of them at the end).  Scenarios: full evaluations in both traversal orders, rescaling
// write / read mode, MCMC-style partial updates with BufferIndexHelper flips and rejections
// (src/dr/evomodel/treedatalikelihood/BufferIndexHelper.java:71-106), tip-state changes, partitioned 9-int lists,
// lists with hazards, a 5000-tip caterpillar (4999 dependency levels: the emission must not recurse on the native stack).
// The worlds, the interpreter, the harness, the tree and the buffer protocol are in plan_harness.h, shared with plan_check_*.cpp.
#include "plan_harness.h"

static void scenarioMcmc(int T, bool virt, bool caterpillar, unsigned seed, int steps, bool someTipPartials) {
    std::mt19937 rng(seed);
    static char where[128]; snprintf(where, sizeof where, "mcmc T=%d virt=%d cat=%d seed=%u tipPartials=%d", T, (int)virt, (int)caterpillar, seed, (int)someTipPartials); g_where = where; g_list = 0;
    Tree tree; tree.random(T, rng, caterpillar);
    const int N = 2 * T - 1;
    Harness h; h.init(T, T + 2 * (T - 1), 2 * N, 2 * (T - 1), virt, seed + 1);
    h.mixStepLimit = true;
    for (int i = 0; i < T; i++) { if (someTipPartials && rng() % 7 == 0) h.setTipPartials(i); else h.setTipStates(i); }
    for (int s = 0; s < 2 * N; s++) h.setMatrix(s);
    Protocol pr(tree);
    std::vector<int> all; tree.postOrder(N - 1, all);
    std::vector<int> lvl = tree.levelOrder();
    // full evaluation, no scaling, post-order; then level order with rescaling (write), then read mode
    { std::vector<int> ops; for (int n : all) pr.pFlip[n] ^= 1; pr.emit(all, 0, ops); h.update(ops, 7); }
    { std::vector<int> ops; for (int n : lvl) pr.pFlip[n] ^= 1; pr.emit(lvl, 1, ops); h.update(ops, 7); }
    { std::vector<int> ops; for (int n : lvl) pr.pFlip[n] ^= 1; pr.emit(lvl, 2, ops); h.update(ops, 7); }
    for (int step = 0; step < steps; step++) {
        pr.store();
        // a proposal: change one or two branches -> their matrices and the path(s) to the root
        std::vector<char> dirty(N, 0);
        const int nChanges = 1 + rng() % 2;
        for (int q = 0; q < nChanges; q++) {
            const int n = rng() % (N - 1);
            pr.mFlip[n] ^= 1; h.setMatrix(pr.mBuf(n));
            for (int a = tree.parent[n]; a >= 0; a = tree.parent[a]) dirty[a] = 1;
        }
        std::vector<int> nodes;
        const bool level = rng() % 2;
        for (int n : (level ? lvl : all)) if (dirty[n]) nodes.push_back(n);
        const int mode = step % 9 == 4 ? 1 : 2;      // every ninth proposal recomputes the scale factors of ITS nodes
        if (mode == 1) {                               // BEAST recomputes all of them: full traversal in write mode
            nodes = level ? lvl : all;
        }
        for (int n : nodes) pr.pFlip[n] ^= 1;
        std::vector<int> ops; pr.emit(nodes, mode, ops);
        h.update(ops, 7);
        if (rng() % 3 == 0) pr.restore();              // rejected: the unflipped buffers must still hold their values
        if (rng() % 4 == 0) { std::vector<int> xs; for (int q = 0; q < 3; q++) xs.push_back(T + rng() % (2 * (T - 1))); h.materialise(xs); }
        if (rng() % 11 == 0) { const int tip = rng() % T; if (h.compact[tip]) {
            // new tip data invalidates everything above it: BEAST would re-evaluate; here only the planner hooks are exercised
            h.setTipStates(tip);
            std::vector<int> nodes2; std::vector<char> d2(N, 0);
            for (int a = tree.parent[tip]; a >= 0; a = tree.parent[a]) d2[a] = 1;
            for (int n : all) if (d2[n]) nodes2.push_back(n);
            pr.store(); for (int n : nodes2) pr.pFlip[n] ^= 1;
            std::vector<int> ops2; pr.emit(nodes2, 2, ops2); h.update(ops2, 7);
            // the OTHER flip of those nodes is now stale in BEAST too (it never reads it again before rewriting it)
        } }
    }
    std::vector<int> every; for (int b = T; b < h.nBuf; b++) every.push_back(b);
    h.materialise(every);
    h.compareAll();
    printf("  mcmc T=%d virt=%d cat=%d: %ld lists, %ld micro-ops, %ld stored, %ld holds, %ld memory reads, %ld materialised, %ld slices in %ld waves\n",
           T, (int)virt, (int)caterpillar, h.lists, h.micro, h.stored, h.holds, h.memReads, h.materialised, h.segsTotal, h.waves);
}

// The chain's steady state when a model parameter changes every iteration: the SAME two full-evaluation lists alternate
// (all nodes flip between their two buffers), with partial updates and rejected proposals in between.  The planner
// serves the repeats from its plan cache; every evaluation is still checked against list-order evaluation.
static void scenarioSteady(int T, bool level, unsigned seed) {
    std::mt19937 rng(seed);
    static char where[128]; snprintf(where, sizeof where, "steady T=%d level=%d seed=%u", T, (int)level, seed); g_where = where; g_list = 0;
    Tree tree; tree.random(T, rng, false);
    const int N = 2 * T - 1;
    Harness h; h.init(T, T + 2 * (T - 1), 2 * N, 2 * (T - 1), true, seed + 1);
    { static const int chunks[4] = {0, 8, 20, 64}; h.fixedChunk = chunks[seed % 4]; }
    for (int i = 0; i < T; i++) h.setTipStates(i);
    for (int s = 0; s < 2 * N; s++) h.setMatrix(s);
    Protocol pr(tree);
    std::vector<int> all; tree.postOrder(N - 1, all);
    std::vector<int> lvl = tree.levelOrder();
    const std::vector<int>& order = level ? lvl : all;
    for (int it = 0; it < 14; it++) {
        for (int n : order) pr.pFlip[n] ^= 1;
        for (int n = 0; n < N - 1; n++) { pr.mFlip[n] ^= 1; h.setMatrix(pr.mBuf(n)); }        // new branch matrices every time
        std::vector<int> ops; pr.emit(order, it % 5 == 0 ? 1 : 2, ops);
        h.update(ops, 7);
        h.compareAll();
        if (it % 3 == 1) {                                   // a proposal on one branch, accepted or not
            pr.store();
            std::vector<char> dirty(N, 0);
            const int n = rng() % (N - 1);
            pr.mFlip[n] ^= 1; h.setMatrix(pr.mBuf(n));
            for (int a = tree.parent[n]; a >= 0; a = tree.parent[a]) dirty[a] = 1;
            std::vector<int> nodes;
            for (int x : order) if (dirty[x]) nodes.push_back(x);
            for (int x : nodes) pr.pFlip[x] ^= 1;
            std::vector<int> ops2; pr.emit(nodes, 2, ops2);
            h.update(ops2, 7);
            if (it != 10) pr.restore();                      // rejected (the accepted one changes the lists that follow)
            h.compareAll();
        }
        if (it == 7) { std::vector<int> xs; for (int q = 0; q < 4; q++) xs.push_back(T + rng() % (2 * (T - 1))); h.materialise(xs); }
        if (it == 9) h.setTipStates(rng() % T);                // new tip data: the next evaluation recomputes everything anyway
    }
    std::vector<int> every; for (int b = T; b < h.nBuf; b++) every.push_back(b);
    h.materialise(every);
    h.compareAll();
    if (T >= 16 && (h.pl.cacheHits < 4 || h.fastReplays < 3)) { fprintf(stderr, "steady T=%d: only %ld plan-cache hits, %ld fast replays\n", T, h.pl.cacheHits, h.fastReplays); exit(1); }
    printf("  steady T=%d level=%d: %ld lists, %ld plan-cache hits, %ld micro-ops, %ld stored\n", T, (int)level, h.lists, h.pl.cacheHits, h.micro, h.stored);
}

static void scenarioPartitions(unsigned seed, int T) {
    g_where = "partitions"; g_list = 0;
    std::mt19937 rng(seed);
    Tree tree; tree.random(T, rng, false);
    const int N = 2 * T - 1;
    Harness h; h.init(T, T + 2 * (T - 1), 2 * N * 3, 2 * (T - 1) * 3, true, seed);
    h.parts = 3; h.partStart = {0, 2, 5}; h.partEnd = {2, 5, P};
    h.pl.setPartitionCount(3);               // definitions per (buffer, partition); more snapshot slots
    for (World* w : {&h.truth, &h.plan}) w->mats.assign(h.pl.matrixSlots(), std::vector<double>((size_t)C * 16, 0.0));
    for (int i = 0; i < T; i++) h.setTipStates(i);
    for (int s = 0; s < 2 * N * 3; s++) h.setMatrix(s);
    std::vector<int> all; tree.postOrder(N - 1, all);
    for (int rep = 0; rep < 6; rep++) {
        std::vector<int> ops;
        const int mode = rep == 1 ? 1 : rep == 0 ? 0 : 2;
        for (int part = 0; part < 3; part++)
            for (int n : all) {
                if (rep > 2 && rng() % 3 == 0 && n != N - 1) continue;   // partial lists (a node above a skipped one re-reads it)
                auto pb = [&](int x) { return x < T ? x : T + 2 * (x - T) + (rep & 1); };
                auto pbOld = [&](int x) { return x < T ? x : T + 2 * (x - T) + ((rep & 1) ^ 0); };
                (void)pbOld;
                const int s = (2 * (n - T)) * 3 + part;
                ops.insert(ops.end(), {pb(n), mode == 1 ? s : -1, mode == 2 ? s : -1, pb(tree.left[n]), (2 * tree.left[n]) * 3 + part,
                                       pb(tree.right[n]), (2 * tree.right[n]) * 3 + part, part, -1});
            }
        if (rep > 2) {   // skipped nodes must exist in this flip: run a full list first in that case
            std::vector<int> full;
            for (int part = 0; part < 3; part++) for (int n : all) {
                auto pb = [&](int x) { return x < T ? x : T + 2 * (x - T) + (rep & 1); };
                const int s = (2 * (n - T)) * 3 + part;
                full.insert(full.end(), {pb(n), -1, 2 > 1 ? s : -1, pb(tree.left[n]), (2 * tree.left[n]) * 3 + part, pb(tree.right[n]), (2 * tree.right[n]) * 3 + part, part, -1});
            }
            h.update(full, 9);
        }
        h.update(ops, 9);
    }
    // per-partition buffer flips, as MultiPartitionDataLikelihoodDelegate's partialBufferHelper[i] does: partial updates of
    // ONE partition at a time on the path to the root, with rejections; definitions of the other partitions must survive
    {
        std::vector<std::vector<int>> flip(3, std::vector<int>(N, 1));       // the last full lists above wrote flip (5 & 1) = 1
        auto pbk = [&](int part, int x) { return x < T ? x : T + 2 * (x - T) + flip[part][x]; };
        for (int step = 0; step < 30; step++) {
            const int part = rng() % 3;
            std::vector<char> dirty(N, 0);
            const int n0 = rng() % (N - 1);
            h.setMatrix((2 * n0) * 3 + part);
            for (int a = tree.parent[n0]; a >= 0; a = tree.parent[a]) dirty[a] = 1;
            std::vector<int> saved = flip[part], ops;
            for (int n : all) if (dirty[n]) flip[part][n] ^= 1;
            for (int n : all) {
                if (!dirty[n]) continue;
                const int sc = (2 * (n - T)) * 3 + part;
                ops.insert(ops.end(), {pbk(part, n), -1, sc, pbk(part, tree.left[n]), (2 * tree.left[n]) * 3 + part,
                                       pbk(part, tree.right[n]), (2 * tree.right[n]) * 3 + part, part, -1});
            }
            h.update(ops, 9);
            if (rng() % 3 == 0) flip[part] = saved;            // rejected
            if (rng() % 5 == 0) { std::vector<int> xs; for (int q = 0; q < 3; q++) xs.push_back(T + rng() % (2 * (T - 1))); h.materialise(xs); }
        }
    }
    std::vector<int> every; for (int b = T; b < h.nBuf; b++) every.push_back(b);
    h.materialise(every);
    h.compareAll();
    printf("  partitions T=%d: %ld lists, %ld micro-ops, %ld stored, %ld materialised\n", T, h.lists, h.micro, h.stored, h.materialised);
}

static void scenarioHazards(unsigned seed) {
    g_where = "hazards"; g_list = 0;
    Harness h; h.init(4, 12, 16, 8, true, seed);
    for (int i = 0; i < 4; i++) h.setTipStates(i);
    for (int s = 0; s < 16; s++) h.setMatrix(s);
    // X(4) = f(0,1); Y(5) = g(X, 2); X(4) = h(2,3) [WAW + WAR]; Z(6) = k(X, Y); Z(6) = k'(Z, 3) [in place]
    std::vector<int> ops = {4, -1, -1, 0, 0, 1, 1,   5, -1, -1, 4, 2, 2, 3,   4, -1, -1, 2, 4, 3, 5,   6, -1, -1, 4, 6, 5, 7,   6, -1, -1, 6, 8, 3, 9};
    h.update(ops, 7);
    // the same scale buffer written by one op and read by a later one of the same list
    std::vector<int> ops2 = {7, 0, -1, 0, 0, 1, 1,   8, -1, 0, 7, 2, 2, 3,   9, 1, -1, 8, 4, 7, 5};
    h.update(ops2, 7);
    std::vector<int> every; for (int b = 4; b < 12; b++) every.push_back(b);
    h.materialise(every);
    printf("  hazards: %ld lists, %ld micro-ops\n", h.lists, h.micro);
}

// A DYNAMIC chain's rescaling cycles (BeagleTreeLikelihood.java:1059-1113): full evaluations in read mode alternating between the two
// buffer parities, every few of them one in WRITE mode into the other scale-buffer set, after which the read-mode lists name that set —
// closed lists throughout, so from the second cycle on every plan comes out of the cache, and right behind a rescaling evaluation it is
// replayed over definitions another entry left behind (same leaves, other scale buffers: WalkPlanner::replay edits the user lists in place).
static void scenarioRescaleCycles(int T, unsigned seed, int cycles, int chunk) {
    std::mt19937 rng(seed);
    static char where[96]; snprintf(where, sizeof where, "rescale cycles T=%d seed=%u chunk=%d", T, seed, chunk); g_where = where; g_list = 0;
    Tree tree; tree.random(T, rng, false);
    const int N = 2 * T - 1;
    Harness h; h.init(T, T + 2 * (T - 1), 2 * N, 2 * (T - 1), true, seed + 1);
    h.fixedChunk = chunk;
    for (int i = 0; i < T; i++) h.setTipStates(i);
    for (int s = 0; s < 2 * N; s++) h.setMatrix(s);
    Protocol pr(tree);
    std::vector<int> lvl = tree.levelOrder();
    auto evaluation = [&](int mode) {
        for (int n : lvl) pr.pFlip[n] ^= 1;
        for (int n = 0; n < N - 1; n++) { pr.mFlip[n] ^= 1; h.setMatrix(pr.mBuf(n)); }
        std::vector<int> ops; pr.emit(lvl, mode, ops); h.update(ops, 7);
    };
    for (int c = 0; c < cycles; c++) {
        evaluation(1);                                   // the rescaling evaluation: new factors into the other set
        for (int k = 0; k < 5; k++) evaluation(2);
        if (c % 2) {                                     // ... and a branch move with its rejection in between, as a chain has them
            pr.store();
            const int n = rng() % (N - 1);
            pr.mFlip[n] ^= 1; h.setMatrix(pr.mBuf(n));
            std::vector<int> path;
            for (int x : lvl) { bool on = false; for (int a = tree.parent[n]; a >= 0; a = tree.parent[a]) on = on || a == x; if (on) path.push_back(x); }
            for (int x : path) pr.pFlip[x] ^= 1;
            std::vector<int> ops; pr.emit(path, 2, ops); h.update(ops, 7);
            pr.restore();
        }
    }
}

// `plan_check bench`: what the planner costs the host on a list it has not seen — config A's shape (1000 taxa, full evaluation, read
// mode, the engine's settings for 1e5 patterns) with a few accepted branch moves between the lists, as a chain produces them
// (bench.py partial_update.full_evaluation_on_a_new_list; profiles/r05_experiments.txt 12).  Microseconds per plan() call.
static void benchPlanner() {
    std::mt19937 rng(7);
    const int T = 1000, N = 2 * T - 1;
    Tree tree; tree.random(T, rng, false);
    WalkPlanner pl;
    pl.init(T + 2 * (T - 1), T, 2 * N, 2 * (T - 1), 24, true, 3);
    pl.launchMachines = 1024.0 / 782.0; pl.chunkTopOps = 16;
    for (int i = 0; i < T; i++) pl.setCompactTip(i, true);
    Protocol pr(tree);
    std::vector<int> lvl = tree.levelOrder();
    Plan out;
    { std::vector<int> ops; for (int n : lvl) pr.pFlip[n] ^= 1; pr.emit(lvl, 1, ops); pl.plan(ops.data(), (int)ops.size() / 7, 7, 1, true, out, 150); }
    double total = 0.0; long micro = 0; const int reps = 200;
    for (int it = 0; it < reps; it++) {
        for (int q = 0; q < 3; q++) {                               // three accepted branch moves: their paths flip
            const int n = rng() % (N - 1);
            pr.mFlip[n] ^= 1;
            std::vector<int> nodes;
            for (int a = tree.parent[n]; a >= 0; a = tree.parent[a]) nodes.push_back(a);
            std::reverse(nodes.begin(), nodes.end());
            std::vector<int> path;                                  // (list order: children before parents)
            for (int x : lvl) if (std::find(nodes.begin(), nodes.end(), x) != nodes.end()) path.push_back(x);
            for (int x : path) pr.pFlip[x] ^= 1;
            std::vector<int> ops2; pr.emit(path, 2, ops2);
            pl.plan(ops2.data(), (int)ops2.size() / 7, 7, 1, true, out, 0);
        }
        for (int n : lvl) pr.pFlip[n] ^= 1;
        for (int n = 0; n < N - 1; n++) pr.mFlip[n] ^= 1;
        std::vector<int> ops; pr.emit(lvl, 2, ops);
        const long hits = pl.cacheHits;
        const auto t0 = std::chrono::steady_clock::now();
        pl.plan(ops.data(), (int)ops.size() / 7, 7, 1, true, out, 150);
        total += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
        if (pl.cacheHits != hits) { fprintf(stderr, "bench: the list was found in the cache\n"); exit(1); }
        micro += (long)pl.planned->prog.size();
    }
    printf("planner, %d-taxon full evaluation on a new list: %.1f us per plan() (%ld micro-operations each)\n", T, total / reps, micro / reps);
}

// `plan_check bench-replay`: what a plan out of the cache costs when the definitions its list leaves behind are another entry's — the
// evaluations of a DYNAMIC chain right behind a rescaling evaluation (the scale-buffer set has flipped: every definition of the tree is
// registered again under the other entry; profiles/r06_experiments.txt 23).  Four lists: two buffer parities x two scale sets, read mode.
static void benchReplay() {
    std::mt19937 rng(7);
    const int T = 1000, N = 2 * T - 1;
    Tree tree; tree.random(T, rng, false);
    WalkPlanner pl;
    pl.init(T + 2 * (T - 1), T, 2 * N, 2 * (T - 1), 24, true, 3);
    pl.launchMachines = 1024.0 / 782.0; pl.chunkTopOps = 16;
    for (int i = 0; i < T; i++) pl.setCompactTip(i, true);
    Protocol pr(tree);
    std::vector<int> lvl = tree.levelOrder();
    std::vector<std::vector<int>> lists;
    for (int sset = 0; sset < 2; sset++) {
        for (int n : lvl) pr.sFlip[n] = sset;
        for (int parity = 0; parity < 2; parity++) {
            for (int n : lvl) pr.pFlip[n] = parity;
            for (int n = 0; n < N - 1; n++) pr.mFlip[n] = parity;
            std::vector<int> ops; pr.emit(lvl, 2, ops); lists.push_back(ops);
        }
    }
    Plan out;
    for (auto& ops : lists) pl.plan(ops.data(), (int)ops.size() / 7, 7, 1, true, out, 150);
    double same = 0.0, other = 0.0; const int reps = 300;
    for (int it = 0; it < reps; it++) {
        const int sset = it & 1;
        for (int k = 0; k < 4; k++) {            // parity 0, 1 (both behind the flip: the other entry's definitions), then 0, 1 again (their own)
            std::vector<int>& ops = lists[(size_t)(2 * sset + (k & 1))];
            const long hits = pl.cacheHits;
            const auto t0 = std::chrono::steady_clock::now();
            pl.plan(ops.data(), (int)ops.size() / 7, 7, 1, true, out, 150);
            const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
            if (pl.cacheHits == hits) { fprintf(stderr, "bench-replay: the list was planned again\n"); exit(1); }
            (k < 2 ? other : same) += us;
            if (it < 3) checkUserLists(pl, T + 2 * (T - 1), 2 * (T - 1), "bench-replay");
        }
    }
    printf("planner, %d-taxon full evaluation out of the cache: %.1f us behind a flipped scale-buffer set, %.1f us in steady state\n", T, other / (2 * reps), same / (2 * reps));
}

int main(int argc, char** argv) {
    if (argc > 1 && !strcmp(argv[1], "bench")) { benchPlanner(); return 0; }
    if (argc > 1 && !strcmp(argv[1], "bench-replay")) { benchReplay(); return 0; }
    const int reps = argc > 1 ? atoi(argv[1]) : 3;
    TopologyStats topology;
    for (int r = 0; r < reps; r++) {
        for (int T : {2, 3, 5, 8, 13, 40, 150}) {
            scenarioMcmc(T, true, false, 1000 * r + T, 60, false);
            scenarioMcmc(T, true, false, 2000 * r + T, 40, true);
            scenarioMcmc(T, false, false, 3000 * r + T, 20, false);
            scenarioMcmc(T, true, true, 4000 * r + T, 30, false);
        }
        for (int T : {9, 40, 150, 600}) { scenarioSteady(T, false, 6000 * r + T); scenarioSteady(T, true, 7000 * r + T); }
        scenarioPartitions(77 + r, 9); scenarioPartitions(177 + r, 40);
        scenarioHazards(5 + r);
        // chains that change the topology (plan_harness.h scenarioTopology): plain virtual buffers and real ones, random chunk sizes and
        // the engine's fixed ones (the plan cache's fast replay), a caterpillar, the step limit of a gradient chain mixed in
        for (int T : {9, 40, 150}) {
            TopologyOptions o;
            topology.add(scenarioTopology(T, true, 8000 * r + T, 60, o));
            o.fixedChunk = T == 9 ? 0 : T == 40 ? 8 : 20;
            topology.add(scenarioTopology(T, true, 8100 * r + T, 60, o));
            o.mixStepLimit = true;
            topology.add(scenarioTopology(T, true, 8200 * r + T, 45, o));
            topology.add(scenarioTopology(T, false, 8300 * r + T, 30, TopologyOptions()));
        }
        { TopologyOptions o; o.caterpillar = true; o.fixedChunk = 8; topology.add(scenarioTopology(60, true, 8400 * r + 60, 60, o)); o.mixStepLimit = true; topology.add(scenarioTopology(17, true, 8500 * r + 17, 60, o)); }
    }
    for (int T : {40, 150}) { TopologyOptions o; o.fixedChunk = 8; topologyWithoutPlanCache(T, 8600u + (unsigned)T, 60, o); }
    topology.print("plan_check");
    if (topology.rejectedTopology < 10 || topology.rootRestored < 1 || topology.closedAgain < 10 || topology.cacheHits < 10 || topology.writeCycles < 10) { fprintf(stderr, "the topology chains hardly exercised rejections, repeated closed lists or rescaling\n"); return 1; }
    P = 2; C = 1;
    scenarioMcmc(5000, true, true, 9, 3, false);     // 4999 dependency levels
    scenarioMcmc(5000, false, true, 11, 2, false);
    scenarioMcmc(3000, true, false, 10, 5, false);
    printf("read-mode folding: %ld programs, %ld factor reads became %ld (%ld members)\n", foldedPlans, unfoldedReads, foldedPays, foldedMembers);
    if (foldedPlans < 100 || foldedPays * 3 > unfoldedReads * 2) { fprintf(stderr, "read-mode folding was hardly exercised\n"); return 1; }
    for (int T : {17, 40, 150}) { scenarioRescaleCycles(T, 77 + T, 6, 8); scenarioRescaleCycles(T, 99 + T, 4, 0); }
    printf("definitions taken over in place by a replayed plan (same leaves, the other scale-buffer set): %ld\n", g_replayInPlace);
    if (g_replayInPlace < 500) { fprintf(stderr, "the in-place replay was hardly exercised\n"); return 1; }
    printf("programs executed on tickets (slices as a forest, leaves in reverse launch order): %ld\n", g_ticketRuns);
    if (g_ticketRuns < 100) { fprintf(stderr, "the ticket form of the one-launch walk was hardly exercised\n"); return 1; }
    printDigest();
    printf("plan_check: OK\n");
    return 0;
}
