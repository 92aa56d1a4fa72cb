// plan_harness.h — what the native planner checks (tests/native/plan_check*.cpp) share.  TEST INFRASTRUCTURE, not product.
//
// The two worlds and list-order evaluation (truthOp), the index-level interpreters of the walk kernel's register model — runPlan for a
// plan, runCompressed for a plan with class tables (planner.h RepeatPlan) —, checkUserLists, the Harness that drives a planner the way
// the engine does, a tree with BEAST's buffer-index protocol and the two topology moves, the alignments that repeat, chains that change
// the topology (scenarioTopology, topologyWithoutPlanCache), and a digest of every plan the interpreters execute (printDigest).  Included by exactly one source file per program: everything here has internal linkage.
#pragma once
#include <algorithm>
#include <cassert>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <random>
#include <vector>

#include "../../beast-mcmc_amd/csrc/planner.h"

using namespace mi355;

static int P = 7, C = 2;
static long foldedPlans = 0, foldedPays = 0, foldedMembers = 0, unfoldedReads = 0;
static const char* g_where = "";
static long g_list = 0;
#define CHECK(cond, m, k) do { if (!(cond)) { fprintf(stderr, "FAILED %s [%s, list %ld] micro-op %d: store %d k1 %d a1 %d k2 %d a2 %d mat %d %d scale %d mode %d hold %d\n", #cond, g_where, g_list, k, (m).storeBuf, (m).k1, (m).a1, (m).k2, (m).a2, (m).mat1, (m).mat2, (m).scaleIdx, (m).smode, (m).hold); exit(1); } } while (0)
#define REQUIRE(cond, ...) do { if (!(cond)) { fprintf(stderr, "FAILED %s (%s:%d) [%s, list %ld]: ", #cond, __FILE__, __LINE__, g_where, g_list); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); exit(1); } } while (0)

// ---- the plan digest -----------------------------------------------------------------------------------------------
// 64-bit FNV-1a over the raw bytes of every plan runPlan executes without a fold map — prog, segs, deps, launchOrder, snapPairs, runs,
// leaves (all-int structs: no padding) — and of every RepeatPlan runCompressed executes: its plan as above, then lower, then origin.
// Two builds of the planner that print the same digest line made the same plans, byte for byte, in the same order.
static unsigned long long g_digest = 14695981039346656037ull;
static long g_digestPlans = 0;
static inline void digestBytes(const void* p, size_t n) {
    const unsigned char* b = static_cast<const unsigned char*>(p);
    for (size_t i = 0; i < n; i++) { g_digest ^= b[i]; g_digest *= 1099511628211ull; }
}
template <class T> static inline void digestVector(const std::vector<T>& v) { if (!v.empty()) digestBytes(v.data(), v.size() * sizeof(T)); }
static inline void digestPlan(const Plan& p) {
    static_assert(sizeof(MicroOp) == 10 * sizeof(int) && sizeof(PlanSeg) == 8 * sizeof(int) && sizeof(PlanRun) == 2 * sizeof(int), "padding in a plan's structs");
    digestVector(p.prog); digestVector(p.segs); digestVector(p.deps); digestVector(p.launchOrder); digestVector(p.snapPairs); digestVector(p.runs);
    digestBytes(&p.leaves, sizeof p.leaves);
}
static inline void printDigest() { printf("plan digest: %016llx over %ld plans\n", g_digest, g_digestPlans); }

struct V4 { double v[4]; };
static inline V4 matvec(const double* m, const V4& x) {
    V4 y;
    for (int i = 0; i < 4; i++) y.v[i] = std::fma(m[4 * i + 3], x.v[3], std::fma(m[4 * i + 2], x.v[2], std::fma(m[4 * i + 1], x.v[1], m[4 * i] * x.v[0])));
    return y;
}
static inline V4 column(const double* m, int s) { V4 y; for (int i = 0; i < 4; i++) y.v[i] = s < 4 ? m[4 * i + s] : 1.0; return y; }

struct World {
    std::vector<std::vector<double>> partials;     // [buf] -> C*P*4 or empty
    std::vector<std::vector<uint8_t>> tips;        // [buf] -> P or empty
    std::vector<std::vector<double>> mats;         // [slot] -> C*16
    std::vector<std::vector<double>> scale;        // [idx] -> P raw factors (empty: never written)
};

static V4 childFactor(const World& w, int buf, bool tip, int mat, int c, int p) {
    const double* m = &w.mats[mat][(size_t)c * 16];
    if (tip) return column(m, w.tips[buf][p]);
    assert(!w.partials[buf].empty());
    V4 x; memcpy(x.v, &w.partials[buf][((size_t)c * P + p) * 4], 32);
    return matvec(m, x);
}

// list-order evaluation of one op (all patterns of [p0, p1))
static void truthOp(World& w, const std::vector<char>& compact, const int* op, int p0, int p1) {
    const int dest = op[0], wS = op[1], rS = op[2], c1 = op[3], m1 = op[4], c2 = op[5], m2 = op[6];
    std::vector<double> out = w.partials[dest];
    if (out.empty()) out.assign((size_t)C * P * 4, 0.0);
    for (int p = p0; p < p1; p++) {
        V4 r[8];
        for (int c = 0; c < C; c++) {
            const V4 a = childFactor(w, c1, compact[c1], m1, c, p), b = childFactor(w, c2, compact[c2], m2, c, p);
            for (int i = 0; i < 4; i++) r[c].v[i] = a.v[i] * b.v[i];
        }
        if (wS >= 0) {
            double m = 0.0;
            for (int c = 0; c < C; c++) for (int i = 0; i < 4; i++) m = std::fmax(m, r[c].v[i]);
            if (!(m > 0.0)) m = 1.0;
            if (w.scale[wS].empty()) w.scale[wS].assign(P, 0.0);
            w.scale[wS][p] = m;
            const double im = 1.0 / m;
            for (int c = 0; c < C; c++) for (int i = 0; i < 4; i++) r[c].v[i] *= im;
        } else if (rS >= 0) {
            const double im = 1.0 / w.scale[rS][p];
            for (int c = 0; c < C; c++) for (int i = 0; i < 4; i++) r[c].v[i] *= im;
        }
        for (int c = 0; c < C; c++) memcpy(&out[((size_t)c * P + p) * 4], r[c].v, 32);
    }
    w.partials[dest] = out;
}

static long g_ticketRuns = 0;          // programs executed on tickets (runPlan below)
// the walk kernel's register model, index level
// fold != nullptr: the engine's read-mode folding (planner.h FoldMap) — a micro-operation multiplies by the product of the reciprocals
// of the scale buffers it pays for (nothing where it pays for none) instead of by its own node's
static void runPlan(World& w, const Plan& plan, const std::vector<int>& partStart, const std::vector<int>& partEnd, const FoldMap* fold = nullptr) {
    if (!fold) { digestPlan(plan); g_digestPlans++; }
    // snapshot copies: one parallel launch (all sources are read before any destination is written)
    std::vector<std::vector<double>> src;
    for (size_t i = 0; i + 1 < plan.snapPairs.size(); i += 2) src.push_back(w.mats[plan.snapPairs[i]]);
    for (size_t i = 0; i + 1 < plan.snapPairs.size(); i += 2) w.mats[plan.snapPairs[i + 1]] = src[i / 2];
    // The kernels are software-pipelined two micro-operations deep: the partials a micro-operation reads as its FIRST child
    // (PK_MEM in k1) are requested at the start of the PREVIOUS micro-operation's stage, before that one stores its result
    // (kernels_walk4.hip WALK_STAGE, tools/gen_walk4_fast.py stage()).  A program must therefore never read in k1 what the
    // micro-operation right before it stores; and slices of one wave run side by side, so none may read what another stores.
    for (size_t a = 0; a < plan.segs.size(); a++) {
        const PlanSeg& sg = plan.segs[a];
        for (int k = sg.progStart + 1; k < sg.progStart + sg.progCount; k++) {
            const MicroOp& m = plan.prog[k];
            CHECK(!(m.k1 == PK_MEM && plan.prog[k - 1].storeBuf == m.a1), m, k);
        }
        for (size_t b = 0; b < plan.segs.size(); b++) {
            const PlanSeg& ob = plan.segs[b];
            if (a == b || ob.wave != sg.wave || ob.partition != sg.partition) continue;
            for (int k = sg.progStart; k < sg.progStart + sg.progCount; k++) {
                const MicroOp& m = plan.prog[k];
                for (int q = ob.progStart; q < ob.progStart + ob.progCount; q++) {
                    const int st = plan.prog[q].storeBuf;
                    if (st < 0) continue;
                    CHECK(!(m.k1 == PK_MEM && m.a1 == st), m, k);
                    CHECK(!(m.k2 == PK_MEM && m.a2 == st), m, k);
                }
            }
        }
    }
    // One launch may run every slice of the plan side by side, each workgroup first waiting for the slices in its dependency
    // list (planner.h PlanSeg): every stored result a slice reads must come from a slice it waits for, of an earlier wave, and
    // the launch order must put every slice behind the ones it waits for.
    {
        CHECK(plan.launchOrder.size() == plan.segs.size(), plan.prog[0], 0);
        std::vector<int> pos(plan.segs.size(), -1);
        for (size_t i = 0; i < plan.launchOrder.size(); i++) { CHECK(pos[plan.launchOrder[i]] < 0, plan.prog[0], (int)i); pos[plan.launchOrder[i]] = (int)i; }
        for (size_t a = 0; a < plan.segs.size(); a++) {
            const PlanSeg& sg = plan.segs[a];
            for (int d = sg.depStart; d < sg.depStart + sg.depCount; d++) {
                const int b = plan.deps[d];
                CHECK(plan.segs[b].wave < sg.wave && plan.segs[b].partition == sg.partition, plan.prog[sg.progStart], (int)a);
                CHECK(pos[b] < pos[a], plan.prog[sg.progStart], (int)a);
                CHECK(plan.segs[b].tail >= plan.segs[b].progCount + sg.tail, plan.prog[sg.progStart], (int)a);
            }
            for (size_t b = 0; b < plan.segs.size(); b++) {
                const PlanSeg& ob = plan.segs[b];
                if (a == b || ob.partition != sg.partition) continue;
                bool waits = false;
                for (int d = sg.depStart; d < sg.depStart + sg.depCount; d++) waits = waits || plan.deps[d] == (int)b;
                if (waits) continue;
                for (int k = sg.progStart; k < sg.progStart + sg.progCount; k++) {
                    const MicroOp& m = plan.prog[k];
                    for (int q = ob.progStart; q < ob.progStart + ob.progCount; q++) {
                        const int st = plan.prog[q].storeBuf;
                        if (st < 0) continue;
                        CHECK(!(m.k1 == PK_MEM && m.a1 == st), m, k);
                        CHECK(!(m.k2 == PK_MEM && m.a2 == st), m, k);
                    }
                }
            }
        }
    }
    auto runSlice = [&](int si) {
        const PlanSeg& sg = plan.segs[si];
        for (int p = partStart[sg.partition]; p < partEnd[sg.partition]; p++) {
            V4 ACC[8], H[3][8];
            for (int k = sg.progStart; k < sg.progStart + sg.progCount; k++) {
                const MicroOp& m = plan.prog[k];
                V4 r[8];
                for (int c = 0; c < C; c++) {
                    V4 f1, f2;
                    const double* M1 = &w.mats[m.mat1][(size_t)c * 16];
                    const double* M2 = &w.mats[m.mat2][(size_t)c * 16];
                    if (m.k1 == PK_TIPS) f1 = column(M1, w.tips[m.a1][p]);
                    else if (m.k1 == PK_MEM) { CHECK(!w.partials[m.a1].empty(), m, k); V4 x; memcpy(x.v, &w.partials[m.a1][((size_t)c * P + p) * 4], 32); f1 = matvec(M1, x); }
                    else { assert(m.k1 >= PK_H0 && m.k1 <= PK_H2); f1 = matvec(M1, H[m.k1 - PK_H0][c]); }
                    if (m.k2 == PK_TIPS) f2 = column(M2, w.tips[m.a2][p]);
                    else if (m.k2 == PK_MEM) { CHECK(!w.partials[m.a2].empty(), m, k); V4 x; memcpy(x.v, &w.partials[m.a2][((size_t)c * P + p) * 4], 32); f2 = matvec(M2, x); }
                    else { assert(m.k2 == PK_ACC); f2 = matvec(M2, ACC[c]); }
                    for (int i = 0; i < 4; i++) r[c].v[i] = f1.v[i] * f2.v[i];
                }
                if (m.smode == PS_WRITE) {
                    double mx = 0.0;
                    for (int c = 0; c < C; c++) for (int i = 0; i < 4; i++) mx = std::fmax(mx, r[c].v[i]);
                    if (!(mx > 0.0)) mx = 1.0;
                    if (w.scale[m.scaleIdx].empty()) w.scale[m.scaleIdx].assign(P, 0.0);
                    w.scale[m.scaleIdx][p] = mx;
                    const double im = 1.0 / mx;
                    for (int c = 0; c < C; c++) for (int i = 0; i < 4; i++) r[c].v[i] *= im;
                } else if (fold) {
                    double im = 1.0;
                    for (int q = fold->payStart[k]; q < fold->payStart[k + 1]; q++) { CHECK(!w.scale[fold->members[q]].empty(), m, k); im *= 1.0 / w.scale[fold->members[q]][p]; }
                    if (fold->payStart[k + 1] > fold->payStart[k]) for (int c = 0; c < C; c++) for (int i = 0; i < 4; i++) r[c].v[i] *= im;
                } else if (m.smode == PS_READ) {
                    CHECK(!w.scale[m.scaleIdx].empty(), m, k);
                    const double im = 1.0 / w.scale[m.scaleIdx][p];
                    for (int c = 0; c < C; c++) for (int i = 0; i < 4; i++) r[c].v[i] *= im;
                }
                if (m.storeBuf >= 0) {
                    if (w.partials[m.storeBuf].empty()) w.partials[m.storeBuf].assign((size_t)C * P * 4, 0.0);
                    for (int c = 0; c < C; c++) memcpy(&w.partials[m.storeBuf][((size_t)c * P + p) * 4], r[c].v, 32);
                }
                for (int c = 0; c < C; c++) { ACC[c] = r[c]; if (m.hold) H[m.hold - 1][c] = r[c]; }
            }
        }
    };
    // Two ways to run a one-launch program (kernels_walk4.hip).  FLAGS: every slice has its own workgroups, which wait for the slices
    // they read from — any order that puts a slice behind its dependencies, here the launch order.  TICKETS (plan.leaves > 0: the
    // slices form a forest): only the slices without dependencies start; whoever finishes slice s counts itself in at s.next and the
    // LAST to arrive there carries on with that slice.  Every other program with a forest is run that way here, the leaves in the
    // REVERSE of the launch order (the order must not matter), and every slice must have run exactly once at the end.
    static unsigned long ticketToggle = 0;
    if (plan.leaves > 0) {
        const int n = (int)plan.segs.size();
        int leaves = 0;
        for (int a = 0; a < n; a++) {
            const PlanSeg& sg = plan.segs[a];
            CHECK(sg.progCount > 0, plan.prog[0], a);
            if (sg.depCount == 0) leaves++;
            for (int d = sg.depStart; d < sg.depStart + sg.depCount; d++) CHECK(plan.segs[plan.deps[d]].next == a, plan.prog[sg.progStart], a);
            if (sg.next >= 0) {
                bool listed = false;
                const PlanSeg& nx = plan.segs[sg.next];
                for (int d = nx.depStart; d < nx.depStart + nx.depCount; d++) listed = listed || plan.deps[d] == a;
                CHECK(listed, plan.prog[sg.progStart], a);
            }
        }
        CHECK(leaves == plan.leaves, plan.prog[0], leaves);
    }
    if (plan.leaves > 0 && (ticketToggle++ & 1)) {
        const int n = (int)plan.segs.size();
        std::vector<int> arrived(n, 0), ran(n, 0);
        for (int i = n - 1; i >= 0; i--) {
            int s = plan.launchOrder[i];
            if (plan.segs[s].depCount != 0) continue;
            for (;;) {
                runSlice(s); ran[s]++;
                const int nxt = plan.segs[s].next;
                if (nxt < 0 || ++arrived[nxt] != plan.segs[nxt].depCount) break;
                s = nxt;
            }
        }
        for (int a = 0; a < n; a++) CHECK(ran[a] == 1, plan.prog[plan.segs[a].progStart], a);
        g_ticketRuns++;
    } else
        for (int si : plan.launchOrder) runSlice(si);
}

// The planner's user lists against its definitions: a definition's key stands in the list of every leaf and every scale buffer its steps
// name, and in no other (replay() edits the lists in place when a definition keeps its leaves: planner.cpp).
static void checkUserLists(const WalkPlanner& pl, int nBuf, int nScale, const char* where) {
    const int parts = pl.partitionCount();
    std::vector<std::vector<int>> wantTip((size_t)nBuf), wantScale((size_t)nScale);
    for (int k = 0; k < nBuf * parts; k++) {
        if (!pl.isVirtualKey(k)) continue;
        const VirtDef& v = pl.definition(k);
        for (int s = 0; s < v.nSteps; s++) {
            if (v.steps[s].tipA >= 0) wantTip[(size_t)v.steps[s].tipA].push_back(k);
            if (v.steps[s].tipB >= 0) wantTip[(size_t)v.steps[s].tipB].push_back(k);
            if (v.steps[s].scaleIdx >= 0) wantScale[(size_t)v.steps[s].scaleIdx].push_back(k);
        }
    }
    auto same = [](std::vector<int> a, std::vector<int> b) {
        std::sort(a.begin(), a.end()); a.erase(std::unique(a.begin(), a.end()), a.end());
        std::sort(b.begin(), b.end());
        return a == b;                               // (b unsorted-unique on purpose: a key listed twice is an error too)
    };
    for (int t = 0; t < nBuf; t++) if (!same(wantTip[(size_t)t], pl.tipUsers(t))) { fprintf(stderr, "USER LISTS: leaf %d [%s]\n", t, where); exit(1); }
    for (int x = 0; x < nScale; x++) if (!same(wantScale[(size_t)x], pl.scaleUsers(x))) { fprintf(stderr, "USER LISTS: scale buffer %d [%s]\n", x, where); exit(1); }
}

static long g_replayInPlace = 0;
struct Harness {
    ~Harness() { g_replayInPlace += pl.replayInPlace; }
    int T, nBuf, nMat, nScale;
    World truth, plan;
    WalkPlanner pl;
    std::vector<char> compact;
    std::vector<int> partStart{0}, partEnd;
    int parts = 1;
    std::mt19937 rng;
    long lists = 0, micro = 0, holds = 0, memReads = 0, stored = 0, materialised = 0, waves = 0, segsTotal = 0;
    long fastReplays = 0;
    int fixedChunk = -1;          // >= 0: every list is planned with this chunk size (the engine's choice depends on the instance only)
    bool mixStepLimit = false;    // some lists are planned under a step limit (scenarioMcmc)

    void init(int tips, int nBuffers, int nMatrices, int nScales, bool virt, unsigned seed) {
        T = tips; nBuf = nBuffers; nMat = nMatrices; nScale = nScales; rng.seed(seed);
        { static const int caps[6] = {6, 8, 12, 16, 24, 32}; static const int holdChoice[3] = {2, 3, 0}; pl.init(nBuf, T, nMat, nScale, caps[seed % 6], virt, holdChoice[(seed / 6) % 3]); }     // (0 hold slots: the 21..64-state walk, kernels_mfma.hip k_walkT64)
        // one-launch programs: the simulated schedule's machine count and the smaller slices above the first wave, varied
        { static const double mach[4] = {0.0, 1.0, 3.0, 10.4}; pl.launchMachines = mach[(seed / 2) % 4]; }
        { static const int top[3] = {0, 8, 16}; pl.chunkTopOps = top[(seed / 3) % 3]; }
        const int slots = pl.matrixSlots();
        for (World* w : {&truth, &plan}) {
            w->partials.assign(nBuf, {}); w->tips.assign(nBuf, {}); w->mats.assign(slots, std::vector<double>((size_t)C * 16, 0.0));
            w->scale.assign(nScale, {});
        }
        compact.assign(nBuf, 0);
        partEnd.assign(1, P);
    }
    void setTipStates(int tip) {
        materialiseKeys(pl.tipUsers(tip));
        std::vector<uint8_t> s(P);
        for (int p = 0; p < P; p++) s[p] = (uint8_t)(rng() % 5);
        truth.tips[tip] = s; plan.tips[tip] = s;
        compact[tip] = 1; pl.setCompactTip(tip, true); pl.setLeafPartials(tip, false);
    }
    void setTipPartials(int tip) {
        materialiseKeys(pl.tipUsers(tip));
        pl.clearVirtual(tip);
        std::vector<double> x((size_t)C * P * 4);
        std::uniform_real_distribution<double> u(0.05, 1.0);
        for (double& v : x) v = u(rng);
        truth.partials[tip] = x; plan.partials[tip] = x;
        compact[tip] = 0; pl.setCompactTip(tip, false); pl.setLeafPartials(tip, true);      // uploaded partials: a leaf definitions may read
    }
    void setMatrix(int slot) {
        std::uniform_real_distribution<double> u(0.01, 1.0);
        std::vector<double> m((size_t)C * 16);
        for (double& v : m) v = u(rng) * 1e-3;     // small entries: products shrink, rescaling matters
        truth.mats[slot] = m; plan.mats[slot] = m;
    }
    void materialise(const std::vector<int>& bufs) {       // buffers -> the keys of their (virtual) partitions
        std::vector<int> keys;
        for (int b : bufs) pl.keysOf(b, keys);
        materialiseKeys(keys);
    }
    void materialiseKeys(std::vector<int> keys) {
        if (keys.empty()) return;
        Plan mp;
        std::vector<int> which;
        for (int x : keys) if (pl.isVirtualKey(x)) which.push_back(x);
        pl.planMaterialize(keys, mp);
        runPlan(plan, mp, partStart, partEnd);
        for (int x : which) { compareRange(pl.bufferOf(x), partStart[pl.partitionOf(x)], partEnd[pl.partitionOf(x)], "materialised"); materialised++; }
    }
    void compareRange(int b, int p0, int p1, const char* what) {
        if (truth.partials[b].empty()) return;
        bool ok = plan.partials[b].size() == truth.partials[b].size();
        for (int c = 0; ok && c < C; c++)
            ok = memcmp(&plan.partials[b][((size_t)c * P + p0) * 4], &truth.partials[b][((size_t)c * P + p0) * 4], (size_t)(p1 - p0) * 32) == 0;
        if (!ok) { fprintf(stderr, "MISMATCH (%s) buffer %d patterns [%d, %d) after %ld lists [%s]\n", what, b, p0, p1, lists, g_where); exit(1); }
    }
    void compareAll() {
        for (int b = 0; b < nBuf; b++) {
            if (compact[b]) continue;
            for (int k = 0; k < parts; k++) if (!pl.isVirtualKey(pl.key(b, k))) compareRange(b, partStart[k], partEnd[k], "real");
        }
        for (int s = 0; s < nScale; s++) {
            if (truth.scale[s].empty()) continue;
            if (plan.scale[s].size() != truth.scale[s].size() || memcmp(plan.scale[s].data(), truth.scale[s].data(), (size_t)P * 8) != 0) {
                fprintf(stderr, "MISMATCH scale %d after %ld lists\n", s, lists); exit(1);
            }
        }
    }
    // one updatePartials call, the way the engine drives the planner
    void update(const std::vector<int>& ops, int tuple) {
        const int count = (int)(ops.size() / tuple);
        for (int k = 0; k < count; k++) {
            const int* op = &ops[(size_t)k * tuple];
            const int part = tuple > 7 ? op[7] : 0;
            truthOp(truth, compact, op, partStart[part], partEnd[part]);
        }
        // a gradient chain's post-order lists are planned with short definitions only (planner.h stepLimit): mixed in at random
        pl.stepLimit = mixStepLimit && (lists % 5 == 3 || lists % 7 == 5) ? 1 + (int)(lists % 2) : 0;
        int begin = 0;
        {   // the engine's fast path for a repeated closed list (engine_walk.cpp runOperationsWalk): no checks, no planning
            bool simple = false;
            if (fixedChunk >= 0 && pl.replayCached(ops.data(), count, tuple, parts, true, fixedChunk, &simple)) {
                assert(simple);
                checkFolded(*pl.planned);
                runPlan(plan, *pl.planned, partStart, partEnd);
                fastReplays++;
                begin = count;
            }
        }
        while (begin < count) {
            const int n = pl.hazardFreePrefix(ops.data(), begin, count, tuple, parts);
            assert(n >= 1);
            const int* sub = ops.data() + (size_t)begin * tuple;
            std::vector<int> need;                 // (keys)
            pl.mustMaterializeBefore(sub, n, tuple, need);
            materialiseNoCompare(need);
            Plan scratch;
            static const int chunkChoices[6] = {0, 0, 3, 8, 20, 64};
            const int rc = pl.plan(sub, n, tuple, parts, true, scratch, fixedChunk >= 0 ? fixedChunk : chunkChoices[rng() % 6]);
            const Plan& p = *pl.planned;           // `scratch`, or the planner's cached copy
            for (size_t q = 1; q < p.segs.size(); q++) assert(p.segs[q].wave >= p.segs[q - 1].wave);
            waves += pl.lastWaves; segsTotal += (long)p.segs.size();
            assert(rc == 0);
            // every MEM child must be real data, every destination must end up real or virtual
            if (begin == 0 && n == count) checkFolded(p);         // (the truth world holds the values after the WHOLE list)
            runPlan(plan, p, partStart, partEnd);
            micro += (long)p.prog.size(); holds += pl.lastHolds; memReads += pl.lastMemReads; stored += pl.lastStored;
            begin += n;
        }
        if (pl.stepLimit > 0)
            for (int k = 0; k < count; k++) {
                const int* op = &ops[(size_t)k * tuple];
                const int kk = pl.key(op[0], tuple > 7 ? op[7] : 0);
                if (pl.isVirtualKey(kk) && pl.definition(kk).nSteps > pl.stepLimit) { fprintf(stderr, "a definition of %d steps under a limit of %d [%s, list %ld]\n", pl.definition(kk).nSteps, pl.stepLimit, g_where, lists); exit(1); }
            }
        pl.stepLimit = 0;
        lists++; g_list = lists;
        compareAll();
        if (nBuf <= 1200) checkUserLists(pl, nBuf, nScale, g_where);
    }
    // The engine's read-mode folding of reciprocal scale factors (planner.h foldScaleFactors): the same program with the factors of
    // unstored results applied where the planner says must give every STORED result the value list-order evaluation gives it — to
    // rounding (the factors are the same numbers multiplied in another order); a factor applied twice or not at all would be off
    // by orders of magnitude.  Run on a copy of the planned world as it is before the program.
    void checkFolded(const Plan& p) {
        if (nBuf > 1200) return;                      // (the copy: not for the 5000-tip ladder)
        FoldMap fm;
        static const int caps[3] = {32, 4, 2};
        if (!foldScaleFactors(p, caps[lists % 3], fm)) return;
        bool anyRead = false;
        for (const MicroOp& m : p.prog) anyRead = anyRead || m.smode == PS_READ;
        if (!anyRead) return;
        // every factor is paid exactly once: the members over the whole program are the program's read-mode scale indices
        {
            std::vector<int> want, got(fm.members);
            for (const MicroOp& m : p.prog) if (m.smode == PS_READ) want.push_back(m.scaleIdx);
            std::sort(want.begin(), want.end()); std::sort(got.begin(), got.end());
            if (want != got) { fprintf(stderr, "FOLD: members differ from the program's read-mode factors [%s, list %ld]\n", g_where, lists); exit(1); }
        }
        World shadow = plan;
        runPlan(shadow, p, partStart, partEnd, &fm);
        for (const PlanSeg& sg : p.segs)
            for (int k = sg.progStart; k < sg.progStart + sg.progCount; k++) {
                const int b = p.prog[k].storeBuf;
                if (b < 0) continue;
                for (int c = 0; c < C; c++)
                    for (int q = partStart[sg.partition]; q < partEnd[sg.partition]; q++)
                        for (int i = 0; i < 4; i++) {
                            const double x = shadow.partials[b][((size_t)c * P + q) * 4 + i], t = truth.partials[b][((size_t)c * P + q) * 4 + i];
                            if (!(std::fabs(x - t) <= 1e-12 * std::fabs(t))) {
                                fprintf(stderr, "FOLD MISMATCH buffer %d pattern %d: %.17g against %.17g [%s, list %ld]\n", b, q, x, t, g_where, lists); exit(1);
                            }
                        }
            }
        foldedPlans++;
        for (size_t k = 0; k < p.prog.size(); k++) { if (fm.payStart[k + 1] > fm.payStart[k]) foldedPays++; if (p.prog[k].smode == PS_READ) unfoldedReads++; }
        foldedMembers += (long)fm.members.size();
    }
    // materialise without comparing: the truth world already holds the values AFTER the list (used for buffers whose
    // old definition is about to be invalidated by a scale rewrite — their truth value is the OLD one only if the list
    // does not rewrite them; they are checked by compareAll afterwards)
    void materialiseNoCompare(const std::vector<int>& xs) {
        if (xs.empty()) return;
        Plan mp;
        pl.planMaterialize(xs, mp);
        runPlan(plan, mp, partStart, partEnd);
    }
};

// ---- a tree and BEAST's buffer-index protocol -------------------------------------------------------------------
struct Tree {
    int T; std::vector<int> left, right, parent;   // internal nodes T..2T-2
    int root = -1;                                 // 2T-2 as random() builds it; a topology move can make another node the root
    void random(int tips, std::mt19937& rng, bool caterpillar) {
        T = tips; const int N = 2 * T - 1; root = N - 1;
        left.assign(N, -1); right.assign(N, -1); parent.assign(N, -1);
        std::vector<int> roots;
        for (int i = 0; i < T; i++) roots.push_back(i);
        for (int n = T; n < N; n++) {
            int a, b;
            if (caterpillar) { a = roots.size() - 1; b = 0; if (a == b) b = 1; }
            else { a = rng() % roots.size(); do { b = rng() % roots.size(); } while (b == a); }
            left[n] = roots[a]; right[n] = roots[b]; parent[roots[a]] = n; parent[roots[b]] = n;
            if (a < b) std::swap(a, b);
            roots.erase(roots.begin() + a); roots.erase(roots.begin() + b);
            roots.push_back(n);
        }
    }
    void postOrder(int root, std::vector<int>& out) const {      // iterative: the ladder tree is 4999 levels deep
        std::vector<std::pair<int, int>> st{{root, 0}};
        while (!st.empty()) {
            const int n = st.back().first, phase = st.back().second++;
            if (n < T) { st.pop_back(); continue; }
            if (phase == 0) st.push_back({left[n], 0});
            else if (phase == 1) st.push_back({right[n], 0});
            else { out.push_back(n); st.pop_back(); }
        }
    }
    std::vector<int> levelOrder() const {   // reverse level order: deepest internal nodes first
        const int N = 2 * T - 1;
        std::vector<int> depth(N, 0), order;
        for (int n = N - 2; n >= 0; n--) {}
        std::vector<int> stack{root};
        std::vector<std::pair<int, int>> byDepth;
        while (!stack.empty()) { int n = stack.back(); stack.pop_back(); if (n < T) continue; byDepth.push_back({depth[n], n});
            depth[left[n]] = depth[right[n]] = depth[n] + 1; stack.push_back(left[n]); stack.push_back(right[n]); }
        std::stable_sort(byDepth.begin(), byDepth.end(), [](auto& a, auto& b) { return a.first > b.first; });
        for (auto& d : byDepth) order.push_back(d.second);
        return order;
    }
    // ---- topology moves (node numbers follow BEAST: a pruned node's parent travels with it) ----
    int sibling(int n) const { const int p = parent[n]; return left[p] == n ? right[p] : left[p]; }
    void replaceChild(int p, int from, int to) { (left[p] == from ? left[p] : right[p]) = to; parent[to] = p; }
    bool below(int n, int top) const { for (int a = n; a >= 0; a = parent[a]) if (a == top) return true; return false; }
    // narrow exchange: i and its uncle swap places (i's parent is not the root).  parentChanged / childrenChanged: the nodes a
    // TreeChangedEvent names
    void narrowExchange(int i, std::vector<int>& parentChanged, std::vector<int>& childrenChanged) {
        const int p = parent[i], g = parent[p], u = sibling(p);
        replaceChild(p, i, u); replaceChild(g, u, i);
        parentChanged = {i, u}; childrenChanged = {p, g};
    }
    // prune and regraft: i's sibling takes the place of i's parent p (or becomes the root), p goes onto the branch above j (or
    // becomes the root when j is).  j is outside what is pruned — the subtree of i and p itself — and is not the sibling, above which
    // p already sits
    void pruneRegraft(int i, int j, std::vector<int>& parentChanged, std::vector<int>& childrenChanged) {
        const int p = parent[i], s = sibling(i), g = parent[p];
        assert(!below(j, i) && j != p && j != s);
        parentChanged = {s, p, j}; childrenChanged = {p};
        if (g >= 0) { replaceChild(g, p, s); childrenChanged.push_back(g); } else { root = s; parent[s] = -1; }
        const int jp = parent[j];
        (left[p] == s ? left[p] : right[p]) = j;
        if (jp >= 0) { replaceChild(jp, j, p); if (jp != g) childrenChanged.push_back(jp); } else { root = p; parent[p] = -1; }
        parent[j] = p;
    }
};

// partials buffers: tips 0..T-1, internal node n -> T + 2(n-T) + flip;  matrices: node n -> 2n + flip;  scale: node n-T -> 2(n-T)+flip
struct Protocol {
    const Tree& t; int T;
    std::vector<int> pFlip, mFlip, sFlip, pSaved, mSaved, sSaved;
    explicit Protocol(const Tree& tr) : t(tr), T(tr.T) { const int N = 2 * T - 1; pFlip.assign(N, 0); mFlip.assign(N, 0); sFlip.assign(N, 0); }
    int pBuf(int n) const { return n < T ? n : T + 2 * (n - T) + pFlip[n]; }
    int mBuf(int n) const { return 2 * n + mFlip[n]; }
    int sBuf(int n) const { return 2 * (n - T) + sFlip[n]; }
    void store() { pSaved = pFlip; mSaved = mFlip; sSaved = sFlip; }
    void restore() { pFlip = pSaved; mFlip = mSaved; sFlip = sSaved; }
    void emit(const std::vector<int>& nodes, int scaleMode /*0 none 1 write 2 read*/, std::vector<int>& ops) {
        for (int n : nodes) {
            if (scaleMode == 1) sFlip[n] ^= 1;
            ops.insert(ops.end(), {pBuf(n), scaleMode == 1 ? sBuf(n) : -1, scaleMode == 2 ? sBuf(n) : -1, pBuf(t.left[n]), mBuf(t.left[n]), pBuf(t.right[n]), mBuf(t.right[n])});
        }
    }
};

// ---- repeated sub-patterns (planner.h RepeatIndex) ---------------------------------------------------------------------
// tip states: five prototype columns, 2 % of the states redrawn (divergent: every state drawn), ~1 % missing under two codes
static inline std::vector<std::vector<uint8_t>> randomTips(int T, int patterns, bool divergent, std::mt19937& rng) {
    std::vector<std::vector<uint8_t>> tips((size_t)T, std::vector<uint8_t>((size_t)patterns));
    const int protos = 5;
    std::vector<std::vector<uint8_t>> proto((size_t)protos, std::vector<uint8_t>((size_t)T));
    for (auto& pr : proto) for (auto& s : pr) s = (uint8_t)(rng() % 4);
    for (int p = 0; p < patterns; p++) {
        const std::vector<uint8_t>& pr = proto[rng() % protos];
        for (int t = 0; t < T; t++) {
            uint8_t s = divergent ? (uint8_t)(rng() % 4) : (rng() % 50 == 0 ? (uint8_t)(rng() % 4) : pr[(size_t)t]);
            if (rng() % 100 == 0) s = (uint8_t)(4 + rng() % 2);          // ~1 % missing, under two codes
            tips[(size_t)t][(size_t)p] = s;
        }
    }
    return tips;
}
// alignments that repeat
static inline std::vector<std::vector<uint8_t>> repeatingTips(int T, int patterns, std::mt19937& rng) { return randomTips(T, patterns, false, rng); }

// the compressed plan on the walk kernel's register model: class-table programs first (one row per class, evaluated on the class's
// representative pattern), then the slices of the walk in launch order, a PK_TAB operand = the pattern's class row of that clade's table.
// fold: the UNCOMPRESSED plan's FoldMap, read through RepeatPlan::origin; nullptr: every read-mode micro-operation pays for itself
static inline void runCompressed(World& w, const RepeatPlan& rp, const FoldMap* fold, const RepeatIndex& idx, const std::vector<int>& partStart, const std::vector<int>& partEnd) {
    const Plan& plan = rp.plan;
    digestPlan(plan); digestVector(rp.lower); digestVector(rp.origin); g_digestPlans++;
    std::vector<std::vector<double>> src;
    for (size_t i = 0; i + 1 < plan.snapPairs.size(); i += 2) src.push_back(w.mats[plan.snapPairs[i]]);
    for (size_t i = 0; i + 1 < plan.snapPairs.size(); i += 2) w.mats[plan.snapPairs[i + 1]] = src[i / 2];
    std::map<int, std::vector<V4>> table;                 // clade -> [class][category]
    auto runSlice = [&](const PlanSeg& sg, bool lower) {
        const RepeatIndex::Clade* cl = lower ? &idx.clade(sg.partition) : nullptr;
        const int n0 = lower ? 0 : partStart[sg.partition], n1 = lower ? cl->D : partEnd[sg.partition];
        if (lower) table[sg.partition].assign((size_t)cl->D * C, V4());
        for (int q = n0; q < n1; q++) {
            const int p = lower ? cl->rep[(size_t)q] : q;
            V4 ACC[8], H[3][8];
            for (int k = sg.progStart; k < sg.progStart + sg.progCount; k++) {
                const MicroOp& m = plan.prog[(size_t)k];
                V4 r[8];
                auto operand = [&](int kind, int a, int mat, int c, bool first) {
                    const double* M = &w.mats[(size_t)mat][(size_t)c * 16];
                    if (kind == PK_TIPS) return column(M, w.tips[(size_t)a][(size_t)p]);
                    if (kind == PK_MEM) { CHECK(!lower && !w.partials[(size_t)a].empty(), m, k); V4 x; memcpy(x.v, &w.partials[(size_t)a][((size_t)c * P + p) * 4], 32); return matvec(M, x); }
                    if (kind == PK_TAB) { CHECK(!lower && table.count(a), m, k); return matvec(M, table[a][(size_t)idx.clade(a).cls[(size_t)p] * C + c]); }
                    if (first) { CHECK(isHoldKind(kind), m, k); return matvec(M, H[kind - PK_H0][c]); }
                    CHECK(kind == PK_ACC, m, k);
                    return matvec(M, ACC[c]);
                };
                for (int c = 0; c < C; c++) {
                    const V4 f1 = operand(m.k1, m.a1, m.mat1, c, true), f2 = operand(m.k2, m.a2, m.mat2, c, false);
                    for (int i = 0; i < 4; i++) r[c].v[i] = f1.v[i] * f2.v[i];
                }
                CHECK(m.smode != PS_WRITE, m, k);
                const int o = rp.origin[(size_t)k];
                if (fold) {
                    double im = 1.0;
                    for (int f = fold->payStart[(size_t)o]; f < fold->payStart[(size_t)o + 1]; f++) im *= 1.0 / w.scale[(size_t)fold->members[(size_t)f]][(size_t)p];
                    if (fold->payStart[(size_t)o + 1] > fold->payStart[(size_t)o]) { CHECK(!lower, m, k); for (int c = 0; c < C; c++) for (int i = 0; i < 4; i++) r[c].v[i] *= im; }
                } else if (m.smode == PS_READ) {
                    CHECK(!lower, m, k);
                    const double im = 1.0 / w.scale[(size_t)m.scaleIdx][(size_t)p];
                    for (int c = 0; c < C; c++) for (int i = 0; i < 4; i++) r[c].v[i] *= im;
                }
                if (m.storeBuf >= 0) {
                    CHECK(!lower, m, k);
                    if (w.partials[(size_t)m.storeBuf].empty()) w.partials[(size_t)m.storeBuf].assign((size_t)C * P * 4, 0.0);
                    for (int c = 0; c < C; c++) memcpy(&w.partials[(size_t)m.storeBuf][((size_t)c * P + p) * 4], r[c].v, 32);
                }
                if (lower && k == sg.progStart + sg.progCount - 1) { CHECK(m.hold == 0, m, k); for (int c = 0; c < C; c++) table[sg.partition][(size_t)q * C + c] = r[c]; }
                for (int c = 0; c < C; c++) { ACC[c] = r[c]; if (m.hold) H[m.hold - 1][c] = r[c]; }
            }
        }
    };
    for (const PlanSeg& sg : rp.lower) runSlice(sg, true);
    for (int si : plan.launchOrder) runSlice(plan.segs[(size_t)si], false);
}

// a run every micro-operation of which reads tips, ACC or hold slots and stores nothing: what the weighting counts as one gather
static inline bool plainRun(const Plan& plan, const PlanRun& run) {
    for (int i = run.start; i < run.start + run.count; i++) {
        const MicroOp& m = plan.prog[(size_t)i];
        if (m.storeBuf >= 0 || m.k1 == PK_MEM || m.k2 == PK_MEM) return false;
    }
    return run.count > 0;
}

// ---- chains that change the topology ---------------------------------------------------------------------------------------
// What a BEAST chain spends half of its tree proposals on: narrow exchange and prune-and-regraft (subtree slide, wide exchange and
// Wilson-Balding are one of the two as far as the buffer protocol goes), with height moves, rejections, rescaling cycles, closed full
// lists that come again, and random materialisations in between.  The truth world against the planned world, bitwise after every list.
// The dirty set is the caller stand-in's (tools/host/tree_likelihood.cpp runTraversal): a node named by a tree-changed event is dirty
// with both of its children, a dirty node that has a parent gets a new branch matrix in the other flip, and a node gets an operation
// when the subtree of one of its children was updated.
struct TopologyOptions {
    bool virt = true, caterpillar = false, mixStepLimit = false;
    int memStepCap = 0, memStepCapSeen = 0;
    int fixedChunk = -1;                   // >= 0: as the engine plans (Harness::fixedChunk: the fast replay of a closed list needs it)
    int initSeed = -1;                     // >= 0: Harness::init's seed (definition cap, hold slots, machines, top slices)
    bool repeats = false;                  // tips from repeatingTips; every cached read-mode plan also runs compressed (runCompressed) over ONE
    int classLimit = 0; size_t capacity = 0;   //   index kept through the chain, dropped at `capacity` as the engine drops it (prepareRepeats)
    bool weights = false, memDefTables = true; // WalkPlanner::repeatWeights / memDefTables
    void (*afterList)(Harness&) = nullptr; // a program's own assertions on the list the harness has just run
    bool noPlanCache = false;              // WalkPlanner::cacheEnabled off: every list planned from scratch (topologyWithoutPlanCache)
};
struct TopologyStats {
    long steps = 0, heightMoves = 0, narrow = 0, prune = 0, rejectedTopology = 0, rootToParent = 0, rootToSibling = 0, rootRestored = 0;
    long closedLists = 0, closedAgain = 0, writeCycles = 0, lists = 0, cacheHits = 0;
    long compressed = 0, subRuns = 0, resets = 0, cladesAcrossMoves = 0;      // (repeats) cladesAcrossMoves: clades the index took in behind accepted topology moves
    void add(const TopologyStats& o) {
        steps += o.steps; heightMoves += o.heightMoves; narrow += o.narrow; prune += o.prune; rejectedTopology += o.rejectedTopology;
        rootToParent += o.rootToParent; rootToSibling += o.rootToSibling; rootRestored += o.rootRestored; closedLists += o.closedLists; closedAgain += o.closedAgain;
        writeCycles += o.writeCycles; lists += o.lists; cacheHits += o.cacheHits; compressed += o.compressed; subRuns += o.subRuns; resets += o.resets; cladesAcrossMoves += o.cladesAcrossMoves;
    }
    void print(const char* program) const {
        printf("%s topology chains: %ld steps (%ld lists): %ld height moves, %ld narrow exchanges, %ld prune-and-regrafts, %ld topology moves rejected; root changes: %ld to the pruned node's parent, "
               "%ld to its sibling, %ld put back by a rejection; %ld closed full lists, %ld of them a second time, %ld write-mode cycles, %ld plan-cache hits; "
               "%ld plans compressed (%ld sub-runs), %ld clades indexed behind topology moves, %ld index resets\n",
               program, steps, lists, heightMoves, narrow, prune, rejectedTopology, rootToParent, rootToSibling, rootRestored, closedLists, closedAgain, writeCycles, cacheHits,
               compressed, subRuns, cladesAcrossMoves, resets);
    }
};

static inline TopologyStats scenarioTopology(int T, bool virt, unsigned seed, int steps, TopologyOptions o = TopologyOptions()) {
    std::mt19937 rng(seed);
    static char where[200];
    snprintf(where, sizeof where, "topology T=%d virt=%d cat=%d seed=%u memcaps %d/%d chunk %d repeats=%d", T, (int)virt, (int)o.caterpillar, seed, o.memStepCap, o.memStepCapSeen, o.fixedChunk, (int)o.repeats);
    g_where = where; g_list = 0;
    REQUIRE(T >= 5, "a topology chain needs five tips");
    TopologyStats st;
    Tree tree; tree.random(T, rng, o.caterpillar);
    const int N = 2 * T - 1;
    Harness h; h.init(T, T + 2 * (T - 1), 2 * N, 2 * (T - 1), virt, o.initSeed >= 0 ? (unsigned)o.initSeed : seed + 1);
    h.mixStepLimit = o.mixStepLimit; h.fixedChunk = o.fixedChunk;
    h.pl.memStepCap = o.memStepCap; h.pl.memStepCapSeen = o.memStepCapSeen; h.pl.repeatWeights = o.weights; h.pl.memDefTables = o.memDefTables;
    h.pl.cacheEnabled = !o.noPlanCache;
    RepeatIndex idx;
    if (o.repeats) {
        const auto tips = repeatingTips(T, P, rng);
        for (int t = 0; t < T; t++) {
            h.truth.tips[(size_t)t] = tips[(size_t)t]; h.plan.tips[(size_t)t] = tips[(size_t)t];
            h.compact[(size_t)t] = 1; h.pl.setCompactTip(t, true); h.pl.setLeafPartials(t, false);
        }
        idx.init(T, P, o.classLimit);
        if (o.capacity) idx.setCapacity(o.capacity);
        for (int t = 0; t < T; t++) idx.setTip(t, h.plan.tips[(size_t)t].data());
    } else
        for (int i = 0; i < T; i++) h.setTipStates(i);
    for (int s = 0; s < 2 * N; s++) h.setMatrix(s);
    Protocol pr(tree);
    bool topologyPending = false;                      // an accepted topology move since the index last saw a list
    // one list through the harness, the program's own checks, and — repeats — the compressed plan over the chain's index
    auto run = [&](const std::vector<int>& ops) {
        const long hits = h.pl.cacheHits + h.fastReplays;
        h.update(ops, 7);
        st.lists++; st.cacheHits += h.pl.cacheHits + h.fastReplays - hits;
        if (o.afterList) o.afterList(h);
        if (!o.repeats || h.pl.plannedTag == 0) return;
        const Plan& plan = *h.pl.planned;
        FoldMap fm;
        if (!foldScaleFactors(plan, st.lists % 2 ? 32 : 4, fm)) return;       // (a list that rescales in write mode is left alone)
        if (idx.overCapacity()) { idx.clear(); st.resets++; }
        const size_t before = idx.size();
        std::vector<RepeatRun> cand;
        findRepeatRuns(plan, &fm, idx, true, cand, nullptr, h.pl.memDefTables);
        if (topologyPending) { st.cladesAcrossMoves += (long)(idx.size() - before); topologyPending = false; }
        if (cand.empty()) return;
        RepeatPlan rp;
        emitRepeatPlan(plan, cand, rp);
        World a = h.plan, b = h.plan;                  // (the list has just run: its snapshot copies are idempotent)
        runPlan(a, plan, h.partStart, h.partEnd, &fm);
        runCompressed(b, rp, &fm, idx, h.partStart, h.partEnd);
        for (int buf = 0; buf < h.nBuf; buf++) {
            REQUIRE(a.partials[(size_t)buf].size() == b.partials[(size_t)buf].size(), "buffer %d", buf);
            if (!a.partials[(size_t)buf].empty()) REQUIRE(memcmp(a.partials[(size_t)buf].data(), b.partials[(size_t)buf].data(), a.partials[(size_t)buf].size() * 8) == 0, "buffer %d differs from the uncompressed plan", buf);
        }
        st.compressed++; st.subRuns += rp.subRuns;
    };
    // the stand-in's traversal over the CURRENT tree: new matrices for the dirty nodes, operations up to the root
    auto traverse = [&](std::vector<char> updateNode, int mode, bool level) {
        for (int n = 0; n < N; n++)
            if (updateNode[(size_t)n] && tree.parent[n] >= 0) { pr.mFlip[n] ^= 1; h.setMatrix(pr.mBuf(n)); }
        std::vector<int> post; tree.postOrder(tree.root, post);
        for (int n : post) if (updateNode[(size_t)tree.left[n]] || updateNode[(size_t)tree.right[n]]) updateNode[(size_t)n] = 2;      // (2: has an operation)
        std::vector<int> nodes;
        for (int n : (level ? tree.levelOrder() : post)) if (updateNode[(size_t)n] == 2) nodes.push_back(n);
        for (int n : nodes) pr.pFlip[n] ^= 1;
        std::vector<int> ops; pr.emit(nodes, mode, ops);
        return ops;
    };
    auto dirtyWithChildren = [&](std::vector<char>& updateNode, int n) {
        updateNode[(size_t)n] = 1;
        if (n >= T) { updateNode[(size_t)tree.left[n]] = 1; updateNode[(size_t)tree.right[n]] = 1; }
    };
    // as scenarioMcmc begins: no scaling, then write mode, then read mode
    for (int mode : {0, 1, 2}) run(traverse(std::vector<char>((size_t)N, 1), mode, mode != 0));
    for (int step = 0; step < steps; step++) {
        pr.store();
        const Tree saved = tree;
        std::vector<char> updateNode((size_t)N, 0);
        // both directions of root change are part of every scenario, accepted: p onto the branch above the root, and a child of the root pruned
        const bool forceUp = step == steps / 3, forceDown = step == (2 * steps) / 3;
        const unsigned kind = forceUp || forceDown ? 2u : rng() % 4;      // 0, 1: heights;  2: prune and regraft;  3: narrow exchange
        bool topology = false;
        if (kind == 3) {
            int i = -1;
            for (int tries = 0; tries < 100 && i < 0; tries++) { const int x = (int)(rng() % (unsigned)N); if (x != tree.root && tree.parent[x] != tree.root) i = x; }
            if (i >= 0) {
                std::vector<int> pc, cc; tree.narrowExchange(i, pc, cc);
                for (int n : pc) updateNode[(size_t)n] = 1;
                for (int n : cc) dirtyWithChildren(updateNode, n);
                st.narrow++; topology = true;
            }
        } else if (kind == 2) {
            int i = -1, j = -1;
            if (forceDown) { const int s = tree.left[tree.root] >= T ? tree.left[tree.root] : tree.right[tree.root]; i = tree.sibling(s); j = rng() % 2 ? tree.left[s] : tree.right[s]; }
            for (int tries = 0; tries < 200 && j < 0; tries++) {
                const int x = (int)(rng() % (unsigned)N), y = forceUp ? tree.root : (int)(rng() % (unsigned)N);
                if (x == tree.root || (forceUp && tree.parent[x] == tree.root)) continue;
                if (tree.below(y, x) || y == tree.parent[x] || y == tree.sibling(x)) continue;
                i = x; j = y;
            }
            REQUIRE(j >= 0 || !(forceUp || forceDown), "no prune-and-regraft found");
            if (j >= 0) {
                const int before = tree.root, p = tree.parent[i];
                std::vector<int> pc, cc; tree.pruneRegraft(i, j, pc, cc);
                for (int n : pc) updateNode[(size_t)n] = 1;
                for (int n : cc) dirtyWithChildren(updateNode, n);
                st.prune++; topology = true;
                if (tree.root != before) { if (tree.root == p) st.rootToParent++; else st.rootToSibling++; }
            }
        }
        if (!topology) {
            const int nChanges = 1 + (int)(rng() % 2);
            for (int q = 0; q < nChanges; q++) dirtyWithChildren(updateNode, (int)(rng() % (unsigned)N));
            st.heightMoves++;
        }
        const bool level = rng() % 2;
        const int mode = step % 9 == 4 ? 1 : 2;          // every ninth proposal is a rescaling evaluation: everything, in write mode
        if (mode == 1) { updateNode.assign((size_t)N, 1); st.writeCycles++; }
        run(traverse(updateNode, mode, level));
        const bool rejected = !(forceUp || forceDown) && rng() % 3 == 0;
        if (rejected) {
            if (tree.root != saved.root) st.rootRestored++;
            pr.restore(); tree = saved;
            if (topology) st.rejectedTopology++;
        } else if (topology) topologyPending = true;
        if (rng() % 4 == 0) { std::vector<int> xs; for (int q = 0; q < 3; q++) xs.push_back(T + (int)(rng() % (unsigned)(2 * (T - 1)))); h.materialise(xs); }
        if (step % 4 == 2) {                             // a model move: every node dirty, a closed list on the current topology
            pr.store();
            const std::vector<int> ops = traverse(std::vector<char>((size_t)N, 1), 2, level);
            run(ops); st.closedLists++;
            if (rng() % 2) {                             // ... and the same list again (new values in the same matrix slots)
                for (int n = 0; n < N; n++) if (tree.parent[n] >= 0 && rng() % 2) h.setMatrix(pr.mBuf(n));
                run(ops); st.closedAgain++;
                if (rng() % 2) run(ops);                 // (a third time: planned again at its second coming under memStepCapSeen, out of the cache now)
            }
        }
        st.steps++;
    }
    std::vector<int> every; for (int b = T; b < h.nBuf; b++) every.push_back(b);
    h.materialise(every);
    h.compareAll();
    REQUIRE(st.rootToParent > 0 && st.rootToSibling > 0, "root changes: %ld to the parent, %ld to the sibling", st.rootToParent, st.rootToSibling);
    REQUIRE(st.narrow > 0 && st.prune >= 2 && st.closedLists > 0, "%ld narrow exchanges, %ld prune-and-regrafts, %ld closed lists", st.narrow, st.prune, st.closedLists);
    if (o.repeats && o.capacity) REQUIRE(st.resets > 0, "the index never reached its capacity of %zu (%zu clades at the end)", o.capacity, idx.size());
    return st;
}

// The same chain with the plan cache and with WalkPlanner::cacheEnabled off (the engine's BEAGLE_MI355_NO_PLAN_CACHE=1): no plan is replayed,
// and yet every plan the interpreters execute is the same, byte for byte and in the same order (the digest), and a closed list is a kept
// plan either way — what the engine does to kept plans only (folded reciprocals, class tables) must not depend on the switch.
static inline void topologyWithoutPlanCache(int T, unsigned seed, int steps, TopologyOptions o) {
    REQUIRE(o.fixedChunk >= 0, "random chunk sizes are drawn per plan() call");
    const unsigned long long digest = g_digest; const long plans = g_digestPlans;
    unsigned long long got[2]; long count[2], hits[2];
    for (int off = 0; off < 2; off++) {
        g_digest = 14695981039346656037ull; g_digestPlans = 0;
        o.noPlanCache = off != 0;
        hits[off] = scenarioTopology(T, true, seed, steps, o).cacheHits;
        got[off] = g_digest; count[off] = g_digestPlans;
    }
    g_digest = digest; g_digestPlans = plans;
    REQUIRE(hits[0] > 0 && hits[1] == 0, "%ld plan-cache hits, %ld with the cache off", hits[0], hits[1]);
    REQUIRE(got[0] == got[1] && count[0] == count[1], "the plans differ without the plan cache: digest %016llx over %ld plans, %016llx over %ld with it", got[1], count[1], got[0], count[0]);
}
