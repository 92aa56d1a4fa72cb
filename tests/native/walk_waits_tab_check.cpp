// walk_waits_tab_check.cpp — kernels.h walkStageWaits in the mode the assembly loop runs under since a table child's class ids are
// requested two stages ahead (the seventh argument, tableIds), against a model of the loop's vector-memory loads in issue order.
// CPU only (tests/test_walk_waits_tab.py): a wrong wait is a silent data race on the device.
//
// What k_walk4_fast issues (tools/gen_walk4_fast.py), stage by stage:
//   prologue:  fetch(0) | fetch(1) | first child of 0
//   stage i:   fetch(i+2) | WAIT(i) | under WF_TABFAR: the class ids of the table children of i+2, first child's first |
//              second child of i from memory or a table: 4 loads, then a full wait |
//              first child of i+1 from memory or a table: 4 loads | stores of i
// a fetch = the matrix table, the two tip-state pairs (one less per WF_NOLOAD bit), three loads of a fused cherry, the reciprocals
// under WF_INV.  A table block of a micro-operation under WF_TABSYNC (a slice's first two: no stage two in front of them) loads the ids
// itself and waits for everything.
// Loads return in the order they were issued, so behind "at most N outstanding" every load but the N youngest has landed (stores share
// the counter: they only make a wait longer).  Required:
//   behind WAIT(i): every load of fetch(i), the ids of a table second child of i, and a first child of i (requested in stage i-1);
//   behind WAIT(i): the class ids of a table FIRST child of i+1 — its rows are requested from them in the middle of stage i;
//   the ids of every table child that is not under WF_TABSYNC were requested at all (WF_TABFAR two stages before).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>
#include "../../beast-mcmc_amd/csrc/kernels.h"

using namespace mi355;

static const int WAIT_N[16] = {4, 3, 5, 2, 6, 7, 8, 9, 10, 11, 12, 1, 13, 14, 15, 16};      // tools/gen_walk4_fast.py WAIT_N
static long g_stages = 0, g_tabFirst = 0, g_tabSecond = 0, g_twoTables = 0, g_behindCherry = 0, g_behindInv = 0, g_behindMem = 0, g_behindHold = 0,
            g_behindSkip = 0, g_frontOfCherry = 0, g_unchangedWithoutTables = 0, g_tighter = 0;

#define CHECK(cond, ...) do { if (!(cond)) { fprintf(stderr, "walk_waits_tab_check: " __VA_ARGS__); fprintf(stderr, " (%s:%d)\n", __FILE__, __LINE__); exit(1); } } while (0)


// ---- the model: loads in issue order; `landed` = how many of them, oldest first, have certainly returned
enum Kind { L_FETCH, L_ID1, L_ID2, L_CHILD1 };
struct Load { int op; Kind kind; };
struct Model {
    std::vector<Load> q;
    size_t landed = 0;
    void issue(int op, Kind k, int n = 1) { for (int j = 0; j < n; j++) q.push_back(Load{op, k}); }
    void wait(int n) { if (q.size() > (size_t)n && q.size() - (size_t)n > landed) landed = q.size() - (size_t)n; }
    bool allLanded(int op, Kind k) const { for (size_t j = landed; j < q.size(); j++) if (q[j].op == op && q[j].kind == k) return false; return true; }
    int issued(int op, Kind k) const { int n = 0; for (const Load& l : q) if (l.op == op && l.kind == k) n++; return n; }
    void fetch(unsigned f, int op) {
        issue(op, L_FETCH);                                   // the matrix table
        if (!(f & WF_NOLOAD1)) issue(op, L_FETCH);
        if (!(f & WF_NOLOAD2)) issue(op, L_FETCH);
        if (f & WF_CHERRY2) issue(op, L_FETCH, 3);
        if (f & WF_INV) issue(op, L_FETCH);
    }
};

struct Slice { std::vector<unsigned> flags; int first, count; };

static unsigned opFlags(int k1, int k2, int hold, int smode, bool store, unsigned skip) {
    unsigned f = walkFlags(k1, k2, hold, smode, store);
    if (k1 == WK_TAB) f |= WF_X | WF_TAB1;                   // the bits the engine adds for the assembly loop
    if (k2 == WK_TAB) f |= WF_MEM2 | WF_TAB2;
    if (k1 != WK_TIPS) f |= skip & WF_NOLOAD1;
    if (k2 != WK_TIPS) f |= skip & WF_NOLOAD2;
    return f;
}

// a random slice with table children, in front of its three no-ops, behind `first` words that belong to somebody else
static Slice randomSlice(std::mt19937& rng) {
    auto pick = [&](int n) { return (int)(rng() % (unsigned)n); };
    Slice s;
    s.first = pick(4); s.count = 1 + pick(14);
    const bool writes = pick(4) == 0;                        // a program that rescales in write mode: no fused cherries, every fetch at its full size
    const unsigned skip = !writes && pick(3) ? (WF_NOLOAD1 | WF_NOLOAD2) : 0u;
    for (int k = 0; k < s.first; k++) s.flags.push_back(0xdeadbeefu);
    for (int k = 0; k < s.count; k++) {
        static const int K1[] = {WK_MEM, WK_TIPS, WK_H0, WK_H1, WK_H2, WK_TAB, WK_TAB, WK_TAB};
        static const int K2[] = {WK_MEM, WK_TIPS, WK_ACC, WK_TAB, WK_TAB, WK_CHERRY, WK_CHERRY};
        const int k1 = K1[pick(8)];
        int k2 = K2[pick(!writes ? 7 : 5)];
        if (k2 == WK_ACC && k == 0) k2 = WK_TIPS;
        const bool table = k1 == WK_TAB || k2 == WK_TAB;
        int smode = pick(writes && !table ? 3 : 2);          // WS_NONE, WS_READ, WS_WRITE
        if (k2 == WK_CHERRY) smode = WS_NONE;               // (WF_INV and WK_CHERRY exclude each other)
        s.flags.push_back(opFlags(k1, k2, pick(4), smode, pick(3) == 0, skip));
    }
    for (int k = 0; k < 3; k++) s.flags.push_back((unsigned)((WK_TIPS << 5) | (WK_TIPS << 8)) | skip);
    return s;
}

// the wait codes of the six-argument call, restated: N = the loads behind the stage's own, a fetch counted without class ids
static int oldFetchLoads(unsigned f) { return 1 + ((f & WF_NOLOAD1) ? 0 : 1) + ((f & WF_NOLOAD2) ? 0 : 1) + ((f & WF_INV) ? 1 : 0) + ((f & WF_CHERRY2) ? 3 : 0); }

static void checkSlice(const Slice& s, int padMode) {
    const size_t n = s.flags.size();
    // exactly as long as the slice and its no-ops: a read past them is a heap overflow the sanitizer reports
    WalkOp* w = (WalkOp*)malloc(n * sizeof(WalkOp));
    WalkOp* w6 = (WalkOp*)malloc(n * sizeof(WalkOp));
    WalkOp* w7 = (WalkOp*)malloc(n * sizeof(WalkOp));
    memset(w, 0x5a, n * sizeof(WalkOp));
    for (size_t k = 0; k < n; k++) w[k].flags = s.flags[k];
    memcpy(w6, w, n * sizeof(WalkOp)); memcpy(w7, w, n * sizeof(WalkOp));
    std::vector<WalkOp> before(w, w + n);
    walkStageWaits(w, s.first, s.count, true, true, padMode, true);
    walkStageWaits(w6, s.first, s.count, true, true, padMode);
    walkStageWaits(w7, s.first, s.count, true, true, padMode, false);
    CHECK(memcmp(w6, w7, n * sizeof(WalkOp)) == 0, "the six-argument call is not the call with tableIds = false");
    std::vector<unsigned> f(n), f6(n);
    for (size_t k = 0; k < n; k++) { f[k] = w[k].flags; f6[k] = w6[k].flags; }
    for (size_t k = 0; k < n; k++) {                         // nothing but the flags of first .. first + count - 1 changes
        WalkOp a = before[k], b = w[k], c = w6[k];
        if ((int)k >= s.first && (int)k < s.first + s.count) a.flags = b.flags = c.flags = 0;
        CHECK(memcmp(&a, &b, sizeof(WalkOp)) == 0 && memcmp(&a, &c, sizeof(WalkOp)) == 0, "descriptor %zu outside the slice's flags was written", k);
    }
    free(w); free(w6); free(w7);
    const int first = s.first, end = s.first + s.count;
    // ---- the six-argument call: what it returned before the mode existed
    for (int i = first; i < end; i++) {
        const unsigned wide = (0xfu << WF_WAIT_SHIFT) | WF_TABFAR | WF_TABSYNC;
        CHECK((f6[(size_t)i] & ~wide) == (f[(size_t)i] & ~wide) && !(f6[(size_t)i] & (WF_TABFAR | WF_TABSYNC)), "stage %d: the two modes differ outside the wait code and the two table bits", i);
        const bool sync = i - first < 2 && (s.flags[(size_t)i] & (WF_TAB1 | WF_TAB2));
        CHECK(((f[(size_t)i] & WF_TABSYNC) != 0) == sync, "stage %d: WF_TABSYNC %s", i, sync ? "missing" : "set");
        const int x1 = i > first && (f6[(size_t)i - 1] & WF_X) ? 4 : 0;
        const int N = (f6[(size_t)i] & WF_X) ? oldFetchLoads(f6[(size_t)i + 2]) : oldFetchLoads(f6[(size_t)i + 1]) + oldFetchLoads(f6[(size_t)i + 2]) + x1;
        CHECK((f6[(size_t)i] & (0xfu << WF_WAIT_SHIFT)) == walkWaitCode(N), "six-argument call: stage %d: code %u, N = %d expected", i, (f6[(size_t)i] >> WF_WAIT_SHIFT) & 15u, N);
        bool tables = false;
        for (int j = i; j <= i + 2; j++) tables = tables || (f[(size_t)j] & (WF_TAB1 | WF_TAB2));
        if (!tables) { CHECK(f[(size_t)i] == f6[(size_t)i], "stage %d: no table child in sight, yet the new mode waits differently", i); g_unchangedWithoutTables++; }
    }
    // ---- the new mode against the model
    Model m;
    auto tableBlock = [&](int op, Kind ids, unsigned tabBit) {          // the block that reads a table child's rows: the ids are there, or it loads them and waits
        if (!(f[(size_t)op] & tabBit)) return;
        if (f[(size_t)op] & WF_TABSYNC) { m.issue(op, ids); m.wait(0); }
        CHECK(m.issued(op, ids) == 1 && m.allLanded(op, ids), "micro-operation %d: the class ids of its table %s child were %s", op, ids == L_ID1 ? "first" : "second",
              m.issued(op, ids) ? "not waited for" : "never requested");
    };
    m.fetch(f[(size_t)first], first);
    m.fetch(f[(size_t)first + 1], first + 1);
    if (f[(size_t)first] & WF_X) { tableBlock(first, L_ID1, WF_TAB1); m.issue(first, L_CHILD1, 4); }
    for (int i = first; i < end; i++) {
        const unsigned fi = f[(size_t)i], fn = f[(size_t)i + 1], ff = f[(size_t)i + 2];
        g_stages++;
        m.fetch(ff, i + 2);
        const int N = WAIT_N[(fi >> WF_WAIT_SHIFT) & 15u];
        m.wait(N);
        CHECK(m.allLanded(i, L_FETCH) && m.allLanded(i, L_ID1) && m.allLanded(i, L_ID2), "stage %d waits with vmcnt(%d): a small load of its own may be in flight", i, N);
        CHECK(m.allLanded(i, L_CHILD1), "stage %d waits with vmcnt(%d): its first child may be in flight", i, N);
        if ((fn & WF_TAB1) && !(fn & WF_TABSYNC))
            CHECK(m.allLanded(i + 1, L_ID1), "stage %d waits with vmcnt(%d): the class ids of the next micro-operation's table first child may be in flight", i, N);
        if (fi & WF_TABFAR) {                                               // behind the wait: the ids of the micro-operation just fetched
            CHECK(ff & (WF_TAB1 | WF_TAB2), "stage %d: WF_TABFAR, but the micro-operation two ahead reads no table", i);
            if (ff & WF_TAB1) m.issue(i + 2, L_ID1);
            if (ff & WF_TAB2) m.issue(i + 2, L_ID2);
        }
        if (fn & WF_TAB1) {
            g_tabFirst++;
            if (fi & WF_CHERRY2) g_behindCherry++;
            if (fi & WF_INV) g_behindInv++;
            if ((fi & WF_X) && !(fi & WF_TAB1)) g_behindMem++;
            if (fi & WF_HREAD) g_behindHold++;
            if (fi & (WF_NOLOAD1 | WF_NOLOAD2)) g_behindSkip++;
            if (ff & WF_CHERRY2) g_frontOfCherry++;
            if (N < WAIT_N[(f6[(size_t)i] >> WF_WAIT_SHIFT) & 15u]) g_tighter++;
        }
        if (fi & WF_TAB2) { g_tabSecond++; if (fi & WF_TAB1) g_twoTables++; }
        if (fi & WF_MEM2) { tableBlock(i, L_ID2, WF_TAB2); m.issue(i, L_FETCH, 4); m.wait(0); }   // a second child from memory or a table: blocking
        if (fn & WF_X) { tableBlock(i + 1, L_ID1, WF_TAB1); m.issue(i + 1, L_CHILD1, 4); }
    }
}

int main() {
    std::mt19937 rng(20261020u);
    for (int round = 0; round < 20000; round++) {
        const Slice s = randomSlice(rng);
        for (int padMode = 0; padMode <= 2; padMode++) checkSlice(s, padMode);
    }
    {   // directed: a table first child behind each of the neighbours, with and without skipped tip loads, table children on both sides
        const unsigned skips[2] = {0u, WF_NOLOAD1 | WF_NOLOAD2};
        for (unsigned skip : skips)
            for (int prev = 0; prev < 6; prev++)
                for (int tab2 = 0; tab2 < 2; tab2++)
                    for (int inv = 0; inv < 2; inv++) {
                        Slice s; s.first = 1; s.flags.push_back(0xdeadbeefu);
                        s.flags.push_back(opFlags(WK_TIPS, WK_TIPS, 1, WS_NONE, false, skip));
                        static const int P1[6] = {WK_TIPS, WK_MEM, WK_H0, WK_H2, WK_TAB, WK_TIPS}, P2[6] = {WK_CHERRY, WK_ACC, WK_ACC, WK_TIPS, WK_TAB, WK_ACC};
                        s.flags.push_back(opFlags(P1[prev], P2[prev], 0, prev == 5 ? WS_READ : WS_NONE, prev == 3, skip));
                        s.flags.push_back(opFlags(WK_TAB, tab2 ? WK_TAB : WK_ACC, 2, inv ? WS_READ : WS_NONE, false, skip));
                        s.flags.push_back(opFlags(WK_TAB, WK_CHERRY, 0, WS_NONE, true, skip));
                        s.count = 4;
                        for (int k = 0; k < 3; k++) s.flags.push_back((unsigned)((WK_TIPS << 5) | (WK_TIPS << 8)) | skip);
                        for (int padMode = 0; padMode <= 2; padMode++) checkSlice(s, padMode);
                    }
    }
    CHECK(g_tabFirst > 10000 && g_tabSecond > 10000 && g_twoTables > 1000, "table children: %ld first, %ld second, %ld both", g_tabFirst, g_tabSecond, g_twoTables);
    CHECK(g_behindCherry > 1000 && g_behindInv > 1000 && g_behindMem > 1000 && g_behindHold > 1000 && g_behindSkip > 1000 && g_frontOfCherry > 1000,
          "neighbours of a table first child: cherry %ld, reciprocals %ld, memory %ld, hold slot %ld, skipped tip load %ld, cherry behind %ld",
          g_behindCherry, g_behindInv, g_behindMem, g_behindHold, g_behindSkip, g_frontOfCherry);
    CHECK(g_tighter > 1000 && g_unchangedWithoutTables > 1000, "tightened waits %ld, stages without tables %ld", g_tighter, g_unchangedWithoutTables);
    printf("walk_waits_tab_check: OK (%ld stages; table first children %ld — behind a fused cherry %ld, reciprocals %ld, a first child from memory %ld, "
           "a hold slot %ld, a skipped tip load %ld; second %ld, both %ld; waits tightened %ld)\n", g_stages, g_tabFirst, g_behindCherry, g_behindInv, g_behindMem,
           g_behindHold, g_behindSkip, g_tabSecond, g_twoTables, g_tighter);
    return 0;
}
