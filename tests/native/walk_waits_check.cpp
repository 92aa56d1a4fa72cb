// walk_waits_check.cpp — kernels.h walkStageWaits against an independent restatement of the order in which the walk kernels issue
// their vector-memory instructions.  CPU only (tests/test_walk_waits.py): a wrong wait is a silent data race on the device.
//
// k_walk4_fast, around stage i of a slice (kernels.h):
//   ... fetch(i) | first child of i-1 | store(i-2) | fetch(i+1) | first child of i | store(i-1) | fetch(i+2) | WAIT
// a fetch = the matrix table, two tip-state loads (one less per WF_NOLOAD bit), the reciprocals under WF_INV, three more with a fused
// cherry; a first child from memory (WF_X) = four loads.  Stage i needs fetch(i) and its own first child: its wait may leave in flight
// the LOADS issued behind the youngest of those, and no more.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>
#include "../../beast-mcmc_amd/csrc/kernels.h"

using namespace mi355;

static const int WAIT_N[16] = {4, 3, 5, 2, 6, 7, 8, 9, 10, 11, 12, 1, 13, 14, 15, 16};      // tools/gen_walk4_fast.py WAIT_N
static long g_checked = 0, g_padded = 0;

#define CHECK(cond, ...) do { if (!(cond)) { fprintf(stderr, "walk_waits_check: " __VA_ARGS__); fprintf(stderr, " (%s:%d)\n", __FILE__, __LINE__); exit(1); } } while (0)

static unsigned scaleMode(unsigned f) { return (f >> 13) & 3u; }

// the loads of a micro-operation's fetch, from its FINAL flags, as the kernels.h comment counts them
static int fetchLoads(unsigned f) {
    int n = 3;
    if (f & WF_NOLOAD1) n--;
    if (f & WF_NOLOAD2) n--;
    if (f & WF_INV) n++;
    if (f & WF_CHERRY2) n += 3;
    return n;
}

// what the assembly loop has issued when stage i waits, oldest first; own: a load stage i itself consumes
struct Issue { bool load; bool own; };
static std::vector<Issue> issuedBeforeWait(const std::vector<unsigned>& f, int first, int i) {
    std::vector<Issue> q;
    auto fetch = [&](int j, bool own) { for (int k = 0; k < fetchLoads(f[(size_t)j]); k++) q.push_back(Issue{true, own}); };
    auto child = [&](int j, bool own) { if (j >= first && (f[(size_t)j] & WF_X)) for (int k = 0; k < 4; k++) q.push_back(Issue{true, own}); };
    auto store = [&](int j) { if (j >= first && (f[(size_t)j] & WF_STORE)) for (int k = 0; k < 4; k++) q.push_back(Issue{false, false}); };
    fetch(i, true); child(i - 1, false); store(i - 2); fetch(i + 1, false); child(i, true); store(i - 1); fetch(i + 2, false);
    return q;
}

struct Slice { std::vector<unsigned> flags; int first, count, nops; };

// a random slice of valid flags words in front of its no-ops, behind `first` words that belong to somebody else
static Slice randomSlice(std::mt19937& rng, bool asmLoop) {
    auto pick = [&](int n) { return (int)(rng() % (unsigned)n); };
    Slice s;
    s.first = pick(4); s.count = 1 + pick(12); s.nops = asmLoop ? 3 : 2;
    const bool writes = pick(2) == 0;                       // a program that rescales in write mode: no fused cherries, every fetch at its full size
    const unsigned skip = asmLoop && !writes && pick(2) ? (WF_NOLOAD1 | WF_NOLOAD2) : 0u;
    for (int k = 0; k < s.first; k++) s.flags.push_back(0xdeadbeefu);
    for (int k = 0; k < s.count; k++) {
        static const int K1[] = {WK_MEM, WK_TIPS, WK_H0, WK_H1, WK_H2, WK_TAB};
        static const int K2[] = {WK_MEM, WK_TIPS, WK_ACC, WK_TAB, WK_CHERRY};
        const int k1 = K1[pick(6)];
        int k2 = K2[pick(asmLoop && !writes ? 5 : 4)];
        if (k2 == WK_ACC && k == 0) k2 = WK_TIPS;
        const bool table = k1 == WK_TAB || k2 == WK_TAB;
        int smode = pick(writes && !table ? 3 : 2);          // WS_NONE, WS_READ, WS_WRITE
        if (k2 == WK_CHERRY) smode = WS_NONE;               // (WF_INV and WK_CHERRY exclude each other)
        unsigned f = walkFlags(k1, k2, pick(4), smode, pick(3) == 0);
        if (asmLoop && k1 == WK_TAB) f |= WF_X | WF_TAB1;   // the bits the engine adds
        if (asmLoop && k2 == WK_TAB) f |= WF_MEM2 | WF_TAB2;
        if (k1 != WK_TIPS) f |= skip & WF_NOLOAD1;
        if (k2 != WK_TIPS) f |= skip & WF_NOLOAD2;
        s.flags.push_back(f);
    }
    for (int k = 0; k < s.nops; k++) s.flags.push_back((unsigned)((WK_TIPS << 5) | (WK_TIPS << 8)) | skip);
    return s;
}

static void checkSlice(const Slice& s, bool asmLoop, bool strict, int padMode) {
    // exactly as long as the slice and its no-ops: a read past them is a heap overflow the sanitizer reports
    WalkOp* w = (WalkOp*)malloc(s.flags.size() * sizeof(WalkOp));
    memset(w, 0x5a, s.flags.size() * sizeof(WalkOp));
    for (size_t k = 0; k < s.flags.size(); k++) w[k].flags = s.flags[k];
    std::vector<WalkOp> before(w, w + s.flags.size());
    walkStageWaits(w, s.first, s.count, asmLoop, strict, padMode);
    std::vector<unsigned> f(s.flags.size());
    for (size_t k = 0; k < f.size(); k++) f[k] = w[k].flags;
    // nothing but the flags of first .. first + count - 1 changes
    for (size_t k = 0; k < f.size(); k++) {
        WalkOp a = before[k], b = w[k];
        const bool inside = (int)k >= s.first && (int)k < s.first + s.count;
        if (inside) a.flags = b.flags = 0;
        CHECK(memcmp(&a, &b, sizeof(WalkOp)) == 0, "descriptor %zu outside the slice's flags was written", k);
    }
    free(w);
    for (int i = s.first; i < s.first + s.count; i++) {
        const unsigned was = s.flags[(size_t)i], now = f[(size_t)i];
        g_checked++;
        if (!asmLoop) {
            // two deep: 8 N + 12, N = the next fetch (+ the previous store under the lax rule, never behind a write-mode micro-operation)
            CHECK((now & 0xff00ffffu) == was, "two-deep: stage %d: bits outside the wait field changed", i);
            int stores = 0;
            if (!strict && i > s.first && scaleMode(s.flags[(size_t)i - 1]) != (unsigned)WS_WRITE && (s.flags[(size_t)i - 1] & WF_STORE)) stores = 4;
            const unsigned nx = s.flags[(size_t)i + 1];
            int n = 1 + ((nx & WF_X) ? 4 : 0) + ((nx & WF_T1) ? 2 : 0) + ((nx & WF_T2) ? 2 : 0) + ((nx & WF_INV) ? 2 : 0) + stores;
            if (n > 12) n = 12;
            CHECK(((now >> 16) & 0xffu) == (unsigned)(8 * n + 12), "two-deep: stage %d: field %u, expected %d", i, (now >> 16) & 0xffu, 8 * n + 12);
            continue;
        }
        // padding: exactly behind write-mode rescaling (mode 1) or a store as well (mode 2) two to four stages back, in this slice
        bool pad = false;
        for (int b = 2; b <= 4 && i - b >= s.first; b++) {
            const unsigned p = s.flags[(size_t)(i - b)];
            if (padMode >= 1 && scaleMode(p) == (unsigned)WS_WRITE) pad = true;
            if (padMode >= 2 && (p & WF_STORE)) pad = true;
        }
        if (i < s.first + 2) CHECK(!pad, "test: a pad on one of the first two");
        CHECK((now & ~(0xfu << WF_WAIT_SHIFT)) == (was | (pad ? (unsigned)WF_INV : 0u)), "assembly loop: stage %d: WF_INV %s, or other bits changed", i, pad ? "missing" : "added");
        if (pad && !(was & WF_INV)) g_padded++;
        // the wait: the loads behind the stage's own, 1..16
        const std::vector<Issue> q = issuedBeforeWait(f, s.first, i);
        int lastOwn = -1, behind = 0;
        for (size_t k = 0; k < q.size(); k++) if (q[k].own) lastOwn = (int)k;
        for (size_t k = (size_t)(lastOwn + 1); k < q.size(); k++) if (q[k].load) behind++;
        const int waits = WAIT_N[(now >> WF_WAIT_SHIFT) & 15u];
        CHECK(waits <= behind, "assembly loop: stage %d waits for %d outstanding, only %d loads are behind its own", i, waits, behind);
        CHECK(waits == (behind < 1 ? 1 : behind > 16 ? 16 : behind), "assembly loop: stage %d waits for %d outstanding, %d loads are behind its own", i, waits, behind);
    }
}

int main() {
    for (int n = 1; n <= 16; n++) CHECK(WAIT_N[(walkWaitCode(n) >> WF_WAIT_SHIFT) & 15u] == n, "walkWaitCode(%d)", n);
    std::mt19937 rng(20261019u);
    for (int round = 0; round < 4000; round++)
        for (int asmLoop = 0; asmLoop < 2; asmLoop++) {
            const Slice s = randomSlice(rng, asmLoop != 0);
            for (int strict = 0; strict < 2; strict++)
                for (int padMode = 0; padMode <= 2; padMode++) checkSlice(s, asmLoop != 0, strict != 0, padMode);
        }
    CHECK(g_padded > 1000, "the padding rule was exercised only %ld times", g_padded);
    printf("walk_waits_check: OK (%ld stages, %ld padded)\n", g_checked, g_padded);
    return 0;
}
