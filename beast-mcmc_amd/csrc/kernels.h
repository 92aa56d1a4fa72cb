// kernels.h — device-side data structures and launcher prototypes of the MI355X engine.
// Everything here is gfx950-only HIP; there is no other backend.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

namespace mi355 {

// Environment switches.  The product library reads only the documented A/B switches (every one of them leaves the
// results unchanged and selects an older or a reference code path) with plain getenv.  Tuning knobs and timing experiments —
// slice lengths, scheduling orders, LDS padding, parts of a kernel left out (some of them give WRONG results by construction) —
// go through labEnv(), which only a LAB build (-DBEAGLE_MI355_LAB: `python beast-mcmc_amd/build.py --lab`, tools/build_variant.sh)
// connects to the environment; the library a maintainer ships cannot be talked into any of them.
#ifdef BEAGLE_MI355_LAB
inline const char* labEnv(const char* name) { return getenv(name); }
#else
inline const char* labEnv(const char*) { return nullptr; }
#endif

// One pruning operation as the level kernels see it (every state count but 4): pointers already resolved on the host
// from the reference's 7-int (or 9-int) tuple {dest, writeScale, readScale, child1, matrix1, child2, matrix2
// [, partition, cumulativeScale]} (src/dr/evomodel/treelikelihood/BeagleTreeLikelihood.java:1266-1299).
// Pointers read out of a descriptor are generic ("flat") to the compiler; flat loads count against the LDS counter as well
// as the vector-memory one and cannot use scalar-base addressing.  Every buffer the engine hands the kernels lives in
// HBM, so device code converts descriptor pointers with gptr() before dereferencing.
#if defined(__HIPCC__)
#define MI355_GLOBAL __attribute__((address_space(1)))
template <class T> __device__ __forceinline__ T MI355_GLOBAL* gptr(T* p) { return (T MI355_GLOBAL*)p; }
#endif

struct OpDesc {
    double*        dest;        // [C][P][S] partials, written on [pStart, pEnd)
    const void*    child1;      // double [C][P][S] partials, or uint8 [P] compact states (kind bit 0)
    const void*    child2;      // same (kind bit 1)
    double*        scaleWrite;  // per-pattern raw scale factors to WRITE (rescale now), or nullptr
    const double*  scaleRead;   // per-pattern raw scale factors to READ (divide by existing), or nullptr
    int            mat1, mat2;  // transition-matrix buffer indices of the two child branches
    int            kind;        // KIND_* bits
    int            pStart, pEnd;// pattern range of this op (whole buffer unless a ...ByPartition call)
    int            pad;
};
static_assert(sizeof(OpDesc) == 64, "OpDesc layout");
enum { KIND_STATES1 = 1, KIND_STATES2 = 2, KIND_CHERRY1 = 4, KIND_CHERRY2 = 8 };
// A child that is a "virtual cherry" (T32 instances with <= 20 states): its buffer is not stored, it IS
// node(tipA over matrix matA, tipB over matrix matB) [/ scale] and the parent's kernel rebuilds its MFMA operands from the
// two tips' states and LDS copies of the two matrices.  OpDesc.child1 / child2 then hold the INDEX of the descriptor in
// the array handed to launchPruneLevelTiled.
struct CherryDesc {
    const uint8_t* tipA;
    const uint8_t* tipB;
    const double*  scale;     // the cherry node's raw scale factors (read mode), or nullptr
    int            matA, matB;
};
static_assert(sizeof(CherryDesc) == 32, "CherryDesc layout");

// Opt a kernel into more than 64 KiB of dynamic LDS.  The attribute is per DEVICE: granted once per (kernel, device) —
// several instances on different GPUs of one process (BEAST's -beagle_instances) each get theirs.  false: the runtime refused.
bool grantDynamicLds(const void* kernel, size_t bytes);

// ---- the pattern walk (4 states, kernels_walk4.hip) ------------------------------------------------------------------
// One micro-operation of a walk program: node = (M1 . child1) * (M2 . child2) [* 1/scale].  A child is read from a
// partials buffer (WK_MEM), is a compact tip (WK_TIPS), or is a value the same thread computed earlier in the program:
// the previous micro-operation's result (WK_ACC, second operand only) or one of two hold slots (WK_H0/WK_H1, first
// operand only; `hold` = 1 + slot: the result of THIS micro-operation is also parked there).  The product commutes
// bitwise, so the planner is free to order the two children that way; a child in memory comes first.
enum { WK_MEM = 0, WK_TIPS = 1, WK_ACC = 2, WK_H0 = 3, WK_H1 = 4, WK_H2 = 5, WK_CHERRY = 6, WK_TAB = 7 };
// WK_TAB (first or second operand; 4 states): the child is a clade whose value an earlier launch evaluated once per distinct sub-pattern
// (planner.h RepeatIndex, engine_walk.cpp).  src1 / src2 = the clade's ROW VECTOR: per pattern, pair-interleaved like the tip states, the
// pattern's CLASS ID (uint16: a lane's pair is one aligned dword, first pattern in the low half; padding positions hold 0).  The table's
// rows lie in the table arena — laid out [C][P][4] like a partials buffer, or several of them back to back — from the table's first row
// on: the descriptor carries that address, arena + (arena index . C . P + first row) . 32, in scaleW (such a micro-operation never
// rescales in write mode) for its first table child (first or second operand); where BOTH children are tables, tab2 holds the second
// one's address as a signed distance from scaleW in rows (units of 32 bytes; 0 where only one child is a table).  The lane's two rows
// are read at base + 32 id + c P 32.  k_walk4 loads the ids where it consumes the operand: an index load, a wait, the row loads.  For the
// assembly loop the engine adds WF_X | WF_TAB1 (the row loads then count as a first child from memory in the stage waits) or WF_MEM2 |
// WF_TAB2 (the blocking second-child path); the loop requests the ids two stages ahead, right behind the micro-operation's fetch (WF_TABFAR),
// into the pipeline slot's tip-state register of that child, so that only the row loads are left where the operand is consumed
// (walkStageWaits, tableIds).
// WK_CHERRY (second operand only, k_walk4_fast only; round 6): the child is a node over two compact tips whose own micro-operation the
// engine has FUSED into this one (engine_walk.cpp ProgramResolver::microOp): src2 = the states of its first tip, scale = those of its second (the
// micro-operation multiplies by no reciprocals: WF_INV and WK_CHERRY exclude each other), the same entry of the matrix stream's cherry
// region = its two branch-matrix tables.  The kernel forms the child's value — column x column, what the fused micro-operation would have left
// in ACC, bit for bit — and goes on as for WK_ACC.  A third of a binary tree's internal nodes are such cherries.
// hold slots the planner may use: k_walk4 keeps all of them in LDS (4 KiB per slot and category: three fit up to 8
// categories), k_walk4_fast two in LDS and the third in registers
#if defined(__HIPCC__)
__host__ __device__
#endif
inline int walkHoldSlots(int C) { return C <= 8 ? 3 : 2; }
enum { WS_NONE = 0, WS_READ = 1, WS_WRITE = 2 };
// flags: what the kernel's fetch stage has to load for the micro-operation (WF_*), then the kinds
enum { WF_X = 1, WF_T1 = 2, WF_T2 = 4, WF_INV = 8, WF_STORE = 16, WF_CHERRY2 = 1 << 15 };
// (bit 14 = WS_WRITE of the scale mode: the assembly loop tests it directly)
// more bits for the assembly loop k_walk4_fast (tools/gen_walk4_fast.py): first child comes from a hold slot (and which),
// second child in memory, the result is parked in a hold slot; and in bits 16..23 — which belong to the kernel that runs the program:
// k_walk4 keeps its wait-table jump there (walkWaitJump) — "the fetch skips the first / second tip-state load" (WF_NOLOAD1 / 2: the
// child is no compact tip; set in programs that do not rescale in write mode) and the stage's wait as a 4-bit code (walkWaitCode)
enum : unsigned { WF_HREAD = 1u << 24, WF_HREAD1 = 1u << 25, WF_MEM2 = 1u << 26, WF_HWRITE = 1u << 27, WF_NOLOAD1 = 1u << 16, WF_NOLOAD2 = 1u << 17,
                  WF_WAIT_SHIFT = 18, WF_HREAD2 = 1u << 31, WF_TAB1 = 1u << 28, WF_TAB2 = 1u << 29,
                  // (walkStageWaits, tableIds) WF_TABFAR, the bit above the wait code: behind this stage's wait the loop requests the class ids
                  // of the table children of the micro-operation TWO ahead, which the stage has just fetched; WF_TABSYNC: nobody requested
                  // this micro-operation's ids — a slice's first two, which have no stage two in front of them: its table block loads them
                  WF_TABFAR = 1u << 22, WF_TABSYNC = 1u << 23 };
// k_walk4_fast's pipeline is three micro-operations deep: the wait of stage k is "at most N vector-memory instructions outstanding",
// N = what was issued behind the small loads of k and may stay in flight (walkStageWaits below).  A fetch is three loads, four
// for a micro-operation that multiplies by reciprocal scale factors (WF_INV), six with a fused cherry (WF_CHERRY2: its table half and
// two more tip-state pairs), so N is 6..12, + 4 behind a first child from memory, or 3..6 when the stage's own first child comes from
// memory; a tip-state load that is skipped (WF_NOLOAD1 / 2) takes one off.  Every count from 1 to 16 has its code (tools/gen_walk4_fast.py
// WAIT_N: 0..15 = 4, 3, 5, 2, 6, 7, 8, 9, 10, 11, 12, 1, 13, 14, 15, 16); more than 16 waits as for 16, less than 1 as for 1 (a smaller N
// only waits longer).
inline unsigned walkWaitCode(int n) {
    static const int codeOf[17] = {11, 11, 3, 1, 0, 2, 4, 5, 6, 7, 8, 9, 10, 12, 13, 14, 15};      // index: N (0 as 1)
    return (unsigned)codeOf[n < 0 ? 0 : n > 16 ? 16 : n] << WF_WAIT_SHIFT;
}
struct WalkOp {              // 64 bytes = one scalar-cache line; every field is an ADDRESS the kernel adds a 32-bit lane offset to
    const void*    src1;     // WK_MEM: first child's partials [C][P][4];  WK_TIPS: its uint8 states
    const void*    src2;     // WK_TIPS: second child's states;  WK_MEM (both children in memory): its partials
    double*        store;    // partials buffer the result is written to (WF_STORE)
    const double*  scale;    // WF_INV: the reciprocals this result is multiplied by — a scale buffer's reciprocal half or a folded vector
                             // (engine_walk.cpp); otherwise a readable all-ones array (the assembly loop loads and multiplies only under WF_INV,
                             // which also pads a fetch behind write-mode stores: walkStageWaits)
    // (the first 48 bytes are what the assembly loop loads per micro-operation: s_load_dwordx8 at 0, s_load_dwordx4 at 32)
    unsigned       flags;    // WF_* | k1 << 5 | k2 << 8 | hold << 11 | scaleMode << 13 | waitJump << 16 (walkWaitJump)
    int            tab2;     // WK_TAB on both children: the second table's first row, in rows behind scaleW (see WK_TAB); otherwise 0
    double*        scaleW;   // WS_WRITE: the scale buffer that receives the factors (plain layout) and, recipOff doubles on, their reciprocals
    const double*  m1;       // first / second child's branch matrix, category 0 ([C][4][4] doubles): read by
    const double*  m2;       // k_gatherMatrices, which lays them out as the stream the walk reads
};
static_assert(sizeof(WalkOp) == 64, "WalkOp layout");
// Position of pattern p in a pair-interleaved per-pattern array (walk instances: compact tip states, reciprocal scale
// factors).  Of every block of 128 patterns, lane 2 q + r of the walk owns patterns q + 32 r and 64 + q + 32 r (that
// assignment makes its result stores full cache lines: tools/gen_walk4_fast.py) — the two are neighbours here, pair after
// pair in lane order.  Such arrays are padded to a multiple of 128 entries.
#if defined(__HIPCC__)
__host__ __device__
#endif
inline size_t walkPairIndex(size_t p) { return (p & ~(size_t)127) + 4 * (p & 31) + 2 * ((p >> 5) & 1) + ((p >> 6) & 1); }
inline unsigned walkFlags(int k1, int k2, int hold, int smode, bool store) {
    unsigned f = (unsigned)((k1 << 5) | (k2 << 8) | (hold << 11) | (smode << 13));
    if (k1 == WK_MEM) f |= WF_X;
    if (k1 == WK_TIPS) f |= WF_T1;
    if (k2 == WK_TIPS) f |= WF_T2;
    if (smode == WS_READ) f |= WF_INV;
    if (store) f |= WF_STORE;
    if (k1 >= WK_H0 && k1 <= WK_H2) f |= WF_HREAD | (k1 == WK_H1 ? WF_HREAD1 : 0u) | (k1 == WK_H2 ? WF_HREAD2 : 0u);
    if (k2 == WK_MEM) f |= WF_MEM2;
    if (k2 == WK_CHERRY) f |= WF_CHERRY2;
    if (hold) f |= WF_HWRITE;
    return f;
}
// vector-memory instructions the kernel's fetch stage issues for a micro-operation / its store stage
// of k_walk4 (k_walk4_fast: 3, + 1 with WF_INV, + 4 with WF_X)
inline int walkFetchCount(unsigned f) { return ((f & WF_X) ? 4 : 0) + ((f & WF_T1) ? 2 : 0) + ((f & WF_T2) ? 2 : 0) + ((f & WF_INV) ? 2 : 0) + 1; }
inline int walkStoreCount(unsigned f) { return (f & WF_STORE) ? 4 : 0; }
// flags field "waitJump" of micro-operation k: 8 N + 12 with N = walkFetchCount(k+1) (walkStageWaits, kernels_walk4.hip)
inline unsigned walkWaitJump(int n) { return (unsigned)(8 * n + 12) << 16; }
// The wait of every stage of one slice, w[first .. first + count - 1] with every other flag bit final: "at most N vector-memory
// instructions outstanding".  Loads and stores share the counter.  Reads the flags of the no-ops behind the slice (three for the
// assembly loop, two otherwise), writes none of them.
// DEFAULT (strict): N = the LOADS issued behind this micro-operation's own.  Sufficient under the one ordering rule the ISA
// guides state for this counter — vector-memory LOADS return in the order they were issued: when at most N operations
// are outstanding and the N youngest loads are all younger than this stage's loads, an unfinished load of this stage
// would leave N + 1 unfinished, whatever the stores (of this or any earlier stage) do.
// BEAGLE_MI355_STRICT_WAITS=0 (strictWaits false): N also counts the stores issued in between, i.e. assumes that a younger store
// is never counted out before an older load.  That held in > 1e9 lane-trials (tests/test_gpu_vmcnt_order.py) — but it
// is an observation, not a documented guarantee, so it is not what ships by default.
// A smaller N than the true number only waits longer.
// asmLoop: k_walk4_fast runs the program (otherwise a two-deep pipeline: k_walk4, k_walkT32).  padMode (LAB builds:
// BEAGLE_MI355_WALK_PAD_FETCH): 0 never pad a fetch, 1 behind write-mode rescaling (the default), 2 also behind stored results.
// tableIds (the assembly loop as generated today; false: the loop that loaded a table child's row ids where it consumed them, behind a
// full wait): sets WF_TABSYNC on a slice's first two micro-operations where they have table children and WF_TABFAR on micro-operation i
// where i + 2 has table children and is not one of those; behind the wait of a stage with WF_TABFAR the loop issues one load per table
// child of i + 2 — the lane's two class ids, the first child's in front of the second's —, and the block that reads a FIRST table
// child's rows runs in the middle of the stage before its use, without a wait of its own: that stage's wait lets the id load land too.
inline void walkStageWaits(WalkOp* w, int first, int count, bool asmLoop, bool strictWaits, int padMode, bool tableIds = false) {
    if (asmLoop) {
        // The stage waits below count LOADS.  Stores share the counter: a stage that finds stores of the two micro-operations
        // before it still unacknowledged waits for as many of them as its N falls short of "loads + stores".  With four loads per
        // fetch that shortfall was covered by the loads of the fetch before (older than the stores, long landed); with three it
        // is not — a write-mode evaluation (every micro-operation stores its factors) lost 8 % to it.  So a micro-operation
        // whose fetch is in flight across such stores fetches four again: WF_INV on top, its scale address the all-ones array
        // (a multiplication by one where it multiplies).  Behind write-mode rescaling only: behind the (rare) stored results of a
        // read-mode program the padding costs what it saves (config A 503 / 503 / 507 us without, with, and with both; ALWAYS
        // 1 053 / 1 003 / 1 005: profiles/r05_experiments.txt).
        for (int i = first + count - 1; i >= first + 2; i--) {      // (backwards: the test reads unpadded flags only of earlier ones — WF_INV is not what it looks at)
            bool pad = false;
            for (int b = 2; b <= 4 && i - b >= first && !pad; b++) {
                const unsigned f = w[i - b].flags;
                pad = (padMode >= 1 && ((f >> 13) & 3u) == (unsigned)WS_WRITE) || (padMode >= 2 && (f & WF_STORE));
            }
            if (pad) w[i].flags |= WF_INV;
        }
    }
    for (int i = first; i < first + count; i++) {
        // k_walk4 (two deep): N = the fetch of the next micro-operation (+ the previous one's stores)
        // (a micro-operation that rescales in write mode also stores its factors, from one of the workgroup's waves only: behind
        // it the count is the strict one whatever the mode)
        const bool prevWrites = i > first && ((w[i - 1].flags >> 13) & 3u) == (unsigned)WS_WRITE;
        const int stores1 = (strictWaits || prevWrites) ? 0 : (i > first ? walkStoreCount(w[i - 1].flags) : 0);
        const int next2 = walkFetchCount(w[i + 1].flags) + stores1;
        if (!asmLoop) { w[i].flags |= walkWaitJump(next2 < 12 ? next2 : 12); continue; }
        // k_walk4_fast (three deep; a fetch is THREE small loads, four with the reciprocal scale factors: WF_INV).  Issue order around
        // stage i: ... fetch(i) | first child of i - 1 from memory (4) | store(i - 2) | fetch(i + 1) | first child of i from memory
        // (4) | store(i - 1) | fetch(i + 2) | WAIT.  A first child of i in memory has to have landed as well: then only what
        // follows it counts.  (Loads only — the strict rule — whatever BEAGLE_MI355_STRICT_WAITS says: with two fetch sizes the
        // code space has no room for the store counts of the lax rule, which bought 1 %.)
        auto fetchLoads = [&](int j) { const unsigned f = w[j].flags;             // (matrix table; tip states, twice; reciprocals; a fused cherry's table half and tips)
                                       return 1 + ((f & WF_NOLOAD1) ? 0 : 1) + ((f & WF_NOLOAD2) ? 0 : 1) + ((f & WF_INV) ? 1 : 0) + ((f & WF_CHERRY2) ? 3 : 0); };
        const int x1 = i > first && (w[i - 1].flags & WF_X) ? 4 : 0;
        int nWait = (w[i].flags & WF_X) ? fetchLoads(i + 2) : fetchLoads(i + 1) + fetchLoads(i + 2) + x1;
        if (tableIds) {
            // Issue order with the class ids: ... fetch(i) | WAIT(i - 2) | ids(i) | first child of i - 1 | fetch(i + 1) | WAIT(i - 1) | ids(i + 1) |
            // first child of i | fetch(i + 2) | WAIT.  The ids of i + 1 lie between fetch(i + 1) and what follows it: they count; and where
            // i + 1 reads a table FIRST child — in the middle of THIS stage — its ids have to have landed: only a second child's ids and
            // fetch(i + 2) are behind them (a first child of i from memory too, but then the stage waits for that anyway).
            auto prefetched = [&](int j) { return j - first >= 2 && j < first + count; };
            const unsigned fn = w[i + 1].flags;
            const int ids2 = (fn & WF_TAB2) ? 1 : 0;
            if (i - first < 2 && (w[i].flags & (WF_TAB1 | WF_TAB2))) w[i].flags |= WF_TABSYNC;
            if (prefetched(i + 2) && (w[i + 2].flags & (WF_TAB1 | WF_TAB2))) w[i].flags |= WF_TABFAR;
            if (prefetched(i + 1) && !(w[i].flags & WF_X)) nWait = (fn & WF_TAB1) ? ids2 + fetchLoads(i + 2) : nWait + ids2;
        }
        w[i].flags |= walkWaitCode(nWait);
    }
}
// A program slice and the pattern range that executes it (one per partition of a partitioned instance).  The kernel is
// software-pipelined two micro-operations deep: progCount must be EVEN and two more readable descriptors must follow
// (k_walk4, k_walkT32); the assembly loop k_walk4_fast is three deep and leaves behind any stage: any progCount, three more descriptors.
// tStart: where the segment's patterns begin in the PAIR-INTERLEAVED arrays — those are laid out partition by partition, every
// partition padded to whole blocks of 128 (engine_instance.cpp setPairLayout), so that a lane's pair is one aligned load wherever a
// partition starts; partials and plain per-pattern arrays keep the caller's pattern numbering.
// depStart / depCount (one fused launch of all slices, k_walk4_fast only): the slices — rows of this array — whose stored results
// this one reads, as a range of the launch's dependency list; its workgroups wait for their flags first.
// next (a launch on tickets, k_walk4_fast only): the row of the ONE slice that reads this slice's stored result, -1: none.  Only the
// rows without dependencies get workgroups then; a workgroup that finishes row s counts itself in at tickets[next][x], and the one
// that makes the count depCount(next) carries on with row `next` itself (planner.h PlanSeg::next).
struct WalkSeg { int progStart, progCount, pStart, pEnd, tStart, depStart, depCount, next; };
// one launch: every 128-pattern group of every segment walks its program; maxRange = max (pEnd - pStart).  A lane owns two
// patterns, 64 apart; its tip states and reciprocal scale factors are stored pair-interleaved (walkPairIndex).
// dStream = the matrix stream of the WHOLE device program (launchGatherMatrices), nOps * C * 16 {M1, M2} pairs.
// tables: the program has class-table operands (kernels.h WK_TAB): the kernel k_walk4Tab, up to eight categories
void launchWalk4(hipStream_t stream, const WalkOp* dProg, const WalkSeg* dSegs, int nSegs, int maxRange, const void* dStream,
                 int P, int C, long recipOff, bool tables = false);
// cherryMats != nullptr (programs of k_walk4_fast with fused cherries): behind the stream's nOps * C entries a CHERRY region of as many, the
// tables of cherryMats[2 k], [2 k + 1] (a fused cherry's branch matrices, category 0) at entry k where they are not null
void launchGatherMatrices(hipStream_t stream, const WalkOp* dProg, int nOps, int C, void* dStream, const double* const* cherryMats = nullptr);
// ... and the plan's matrix snapshots (src, dst index pairs) in the same launch; m1 / m2 of freshly snapshotted matrices must point at the sources
// ... and queued host copies (copies / copyBlocks: kernels_walk4.hip k_gatherAndSnapshot); dProg / dSrcDst may then be the host ring's mapping
struct HostCopyList;
void launchGatherAndSnapshot(hipStream_t stream, const WalkOp* dProg, int nOps, int C, void* dStream, double* matrices, const int* dSrcDst, int nPairs, int elems,
                             const HostCopyList* copies = nullptr, int copyBlocks = 0, const double* const* cherryMats = nullptr);
// The same walk by the assembly loop (tools/gen_walk4_fast.py).  Requirement: EVERY descriptor carries readable addresses in
// src1, src2 and scale even where unused (the small loads are unconditional): all-missing tip states / all-one scale factors.
// deps / flags / epoch / flagStride: all slices of a program in ONE launch (slice y is dispatched before y + 1): a workgroup first
// waits until flags[d * flagStride + x] == epoch for every slice d of its dependency list, and sets flags[y * flagStride + x] =
// epoch when its results are out.  flags == nullptr: no waiting, no signalling (one launch per wave of independent slices).
// what the walk's root slice needs to finish the evaluation itself (kernels_walk4.hip, root_site4.h; rootSeg < 0: nothing)
struct RootFusedParts;
struct RootFused {
    const double* catWeights; const double* freqs; const double* cum; const double* patternWeights;
    double* siteLogL; double* blockSums; unsigned* counter; double* out; unsigned long long* flag; unsigned long long seq;
    int cumIsRaw; int rootSeg; int groups; int pad;
    const RootFusedParts* parts;     // DEVICE memory, or nullptr: the roots of a partitioned instance's partitions (below)
};
// ... and the same for the roots of up to ROOT_MAX_PARTS partitions (calculateRootLogLikelihoodsByPartition behind updatePartialsByPartition:
// every partition's top slice finishes its own partition; RootFused carries what the partitions share — pattern weights, site values,
// blockSums, counter, out[partition], flag, seq —, rootSeg = -1 and a pointer to this table in device memory: by value it kept more
// scalars alive across the assembly loop than the kernel has).  A pattern group's sum goes to blockSums[blockOff + group],
// the last of ALL groups adds every partition's up in index order (root_site4.h rootPublishGroupParts; k_rootSite4WParts: the same bits).
struct RootFusedPart { const double* catWeights; const double* freqs; const double* cum; int cumIsRaw, rootSeg, blockOff, groups; };
struct RootFusedParts { RootFusedPart p[8]; int n, totalGroups; };
// spinLimit: how long a workgroup polls those flags (ticks of the 100 MHz wall clock) before it computes what it waits for itself
// (kernels_walk4.hip: forward progress whatever the dispatch order); *selfServed counts the workgroups that did.
void launchWalk4Fast(hipStream_t stream, const WalkOp* dProg, const WalkSeg* dSegs, int nSegs, int maxRange, const void* dStream, int P, int C,
                     long recipOff, const int* dDeps = nullptr, unsigned* flags = nullptr, unsigned epoch = 0, int flagStride = 0,
                     const RootFused* root = nullptr, unsigned long long spinLimit = 0, unsigned* selfServed = nullptr,
                     unsigned* tickets = nullptr, int nLeaves = 0, bool xcdAware = false, unsigned cherryOff = 0);
// (cherryOff: byte offset of the stream's cherry region — nOps * C * 320 of the WHOLE device program — where it has fused cherries)
// (tickets != nullptr: rows 0 .. nLeaves - 1 of dSegs are the slices without dependencies — the launch's grid —, the rest follow;
// tickets[row * flagStride + x] are zero before the launch and zero again behind it; deps / flags / epoch / spinLimit unused;
// xcdAware: a launch the chip holds all at once lays its rows out so that all pattern groups of a row run on one XCD — kernels_walk4.hip)
#ifdef BEAGLE_MI355_LAB
void setWalkTrace(unsigned long long* devicePointer);          // (kernels_walk4.hip g_walkTrace; nullptr: off)
#endif
// 4-state walk instances: the root integration as a launch of its own, bit-compatible with the walk's root epilogue (root_site4.h)
void launchRootLogLikelihood4W(hipStream_t stream, const double* root, const double* catWeights, const double* freqs,
                               const double* cum, int cumIsRaw, const double* patternWeights, double* siteLogL,
                               double* blockSums, double* out, int P, int C, int pStart, int pEnd,
                               unsigned long long* flag, unsigned long long seq, unsigned* counter);

// matrices[dst[k]] = matrices[src[k]] for k < n (each C*S*S doubles): private snapshots of branch matrices
void launchSnapshotMatrices(hipStream_t stream, double* matrices, const int* dSrcDst, int n, int elems);

// ---- launchers (all asynchronous on `stream`) -------------------------------------------------

// Host -> device copies of small arrays by a kernel (engine_instance.cpp flushUploads): entry k moves `bytes` from `src` — host
// memory the device maps — to `dst`; its workgroups are firstBlock .. firstBlock + ceil(bytes / 4096) - 1.
constexpr int HOST_COPY_MAX = 12;
struct HostCopyList { struct Entry { void* dst; const void* src; unsigned bytes, firstBlock; } e[HOST_COPY_MAX]; int n; };
void launchHostCopies(hipStream_t stream, const HostCopyList& list, int blocks);
#ifdef __HIPCC__
// one workgroup of 256 threads moves 4 KiB of entry k (block = its index among the list's blocks): k_hostCopies, and the kernels the
// queued copies ride along with (k_transition4Fused, k_gatherAndSnapshot)
__device__ __forceinline__ void hostCopyBlock(const HostCopyList& L, unsigned block) {
    int k = 0;
    while (k + 1 < L.n && block >= L.e[k + 1].firstBlock) k++;
    const size_t base = (size_t)(block - L.e[k].firstBlock) * 4096;
    if (base >= L.e[k].bytes) return;                 // (an entry superseded by a later one for the same destination: bytes = 0)
    const char* s = (const char*)L.e[k].src + base;
    char* d = (char*)L.e[k].dst + base;
    const unsigned left = L.e[k].bytes - (unsigned)base, n = left < 4096u ? left : 4096u;
    const unsigned t = threadIdx.x;
    if ((((size_t)s | (size_t)d) & 15) == 0) {
        if (t * 16 + 16 <= n) *reinterpret_cast<uint4*>(d + t * 16) = *reinterpret_cast<const uint4*>(s + t * 16);
        for (unsigned i = (n & ~15u) + t; i < n; i += 256) d[i] = s[i];
    } else if ((((size_t)s | (size_t)d) & 3) == 0) {
        for (unsigned i = t * 4; i + 4 <= n; i += 1024) *reinterpret_cast<unsigned*>(d + i) = *reinterpret_cast<const unsigned*>(s + i);
        for (unsigned i = (n & ~3u) + t; i < n; i += 256) d[i] = s[i];
    } else
        for (unsigned i = t; i < n; i += 256) d[i] = s[i];
}
#endif
// dst[0..n) = src[0..n) — dst in host memory the device maps —, then *flag = seq (release, system scope): a result handed to a
// polling host thread
void launchPublish(hipStream_t stream, const double* src, int n, double* dst, unsigned long long* flag, unsigned long long seq);

// P(t) = U diag(exp(lambda * t * r_c)) U^-1, negatives clamped to 0, for `count` branches.
// dIdx/dLen/dEig/dRate: device arrays of length `count`: destination matrix index, edge length,
// eigen-system index and category-rate-set index per branch.
// complexEigen: eigen systems are [U | U^-1 | Re lambda (S) | Im lambda (S)] in real block form (transition_body.h iexpEntry)
void launchTransitionMatrices(hipStream_t stream, double* matrices, const double* eigen, const double* rates,
                              const int* dIdx, const double* dLen, const int* dEig, const int* dRate,
                              int count, int S, int C, bool complexEigen = false);

// 4 states, ONE eigen system and ONE rate set for all `count` branches (beagleUpdateTransitionMatrices), and everything the call
// needs still in the host's staging ring: eigSrc / ratesSrc / idx / len may be HOST addresses the device maps (each workgroup
// stages the eigen system and the rates in LDS with one read over the link, a thread reads its own branch length and matrix
// index), and the queued host->device copies of `pending` (kernels.h HostCopyList: the persistent copies of the same eigen
// system and rates, whatever else was queued) ride in the same launch as extra workgroups — one launch where there were a
// copy kernel and a transition kernel.  Same arithmetic and summation order as launchTransitionMatrices.
void launchTransitionMatrices4Fused(hipStream_t stream, double* matrices, const double* eigSrc, const double* ratesSrc, const int* idx,
                                    const double* len, int count, int C, bool complexEigen, const HostCopyList& pending, int copyBlocks);

// C_c = A_c * B_c per category, `count` triples (device index arrays).
void launchConvolveMatrices(hipStream_t stream, double* matrices, const int* dFirst, const int* dSecond,
                            const int* dResult, int count, int S, int C);
// C_c = A_c + B_c per category (a result may be one of its own operands: entry by entry)
void launchAddMatrices(hipStream_t stream, double* matrices, const int* dFirst, const int* dSecond, const int* dResult, int count, int S, int C);

// ---- substitution-parameter differential matrices (kernels_differential.hip; beagleMi355UpdateDifferentialMatrices) ---------
// V = U^-1 dQ U for `pairCount` (eigen system, differential) pairs, entries with |V_ij| < 1e-10 set to 0: dPairs holds {eigen index,
// differential index} per pair, dQ the call's differentials [.][S][S], V receives [pairCount][S][S].  S <= 64.
void launchDifferentialRotate(hipStream_t stream, double* V, const double* eigen, const double* dQ, const int* dPairs, int pairCount,
                              int S, bool complexEigen);
// slot dIdx[u], category c = U (V[dPair[u]] o Phi(dLen[u] * rate(c))) U^-1 for `count` branches (device arrays of that length: slot,
// length, eigen index, rate set, pair).  One thread per (branch, category) up to 8 states, one workgroup from 9 to 64.
void launchDifferentialExact(hipStream_t stream, double* matrices, const double* eigen, const double* rates, const double* V,
                             const int* dIdx, const double* dLen, const int* dEig, const int* dRate, const int* dPair,
                             int count, int S, int C, bool complexEigen);
// slot dIdx[u], category c = dLen[u] * rate(c) * dQ[dDiff[u]]
void launchDifferentialFirstOrder(hipStream_t stream, double* matrices, const double* rates, const double* dQ, const int* dIdx,
                                  const double* dLen, const int* dRate, const int* dDiff, int count, int S, int C);

// ---- eigen systems of time-reversible models (kernels_eigen.hip; beagleMi355SetReversibleModels) ------------------------------
constexpr int EIGEN_SWEEP_CAP = 30;          // Jacobi sweeps after which a model counts as failed (its eigenvalues become NaN)
// `count` models, model k from models[k] = {relative rates [S (S - 1) / 2], upper triangle in row order | frequencies [S]} into eigen
// slot slots[k] (U | U^-1 | lambda, [S] more zeros on a complex instance); sweeps[k] = the sweeps it took, negated when it hit the cap.
// 2 <= S <= 64.  false: the kernel's LDS was not granted (nothing is launched).
bool launchEigenReversible(hipStream_t stream, double* eigen, const double* models, const int* slots, int* sweeps, int count, int S,
                           bool complexEigen);

// ---- transition matrices from generators (kernels_generator.hip; beagleMi355UpdateTransitionMatricesFromGenerators) ----
constexpr int GENERATOR_TERMS = 21;            // B^0 .. B^20 per generator: the power table is [generator][21][S][S] doubles
constexpr int GENERATOR_MAX_SQUARINGS = 40;    // a matrix that would need more is written as NaN and counted
// tables[g] = {I, B, B^2 .. B^20}, B = Q[g] / mu[g] + I, for `count` generators (Q [count][S][S], mu [count], device arrays).  One
// thread per generator up to 8 states, one workgroup from 9 to 64.  false: no kernel for this S.
bool launchGeneratorPowers(hipStream_t stream, double* tables, const double* Q, const double* mu, int count, int S);
// slot dIdx[u], category c = exp(Q[dGen[u]] dLen[u] rate(c)) from the tables (header arithmetic) for `count` entries (device arrays of
// that length: slot, length, generator of the tables, rate set).  stats: {largest s, matrices refused} device words.  One thread per
// (entry, category) up to 8 states, one workgroup from 9 to 64 (squarings on the matrix cores from 16).
bool launchGeneratorMatrices(hipStream_t stream, double* matrices, const double* rates, const double* tables, const double* mu,
                             const int* dIdx, const double* dLen, const int* dGen, const int* dRate, unsigned* stats, int count, int S, int C);

// ---- branch matrices of epoch models (kernels_epoch.hip; beagleMi355UpdateTransitionMatricesWithEpochs) ----
// slot dSlot[u], category c = the left fold of the transition matrices of segments dOff[u] .. dOff[u + 1] - 1 (eigen system dSegEig[j],
// length dSegLen[j], rate set dRate[u]) for `count` entries; all device arrays.  One thread per (entry, category) up to 8 states, one
// workgroup from 9 to 64 (products on the matrix cores from 16).  false: no kernel for this S, or the kernel's LDS was not granted.
bool launchEpochMatrices(hipStream_t stream, double* matrices, const double* eigen, const double* rates, const int* dSlot, const int* dRate,
                         const int* dOff, const int* dSegEig, const double* dSegLen, int count, int S, int C, bool complexEigen);

// One dependency level of pruning operations: `nOps` independent ops, descriptors on the device.
// maxRange = max over ops of (pEnd - pStart).
void launchPruneLevel(hipStream_t stream, const OpDesc* dOps, int nOps, const double* matrices,
                      int P, int S, int C, int maxRange);

// The same for up to ROOT_MAX_PARTS pattern ranges in ONE pair of launches (calculateRootLogLikelihoodsByPartition): range k
// has its own root buffer, weights, frequencies and cumulative buffer; out[k] = its sum; `flag` as above, after the last.
constexpr int ROOT_MAX_PARTS = 8;
struct RootPart { const double* root; const double* catWeights; const double* freqs; const double* cum; int cumIsRaw, pStart, pEnd, blockOff; };
struct RootParts { RootPart p[ROOT_MAX_PARTS]; int n; };
void launchRootLogLikelihoodParts(hipStream_t stream, const RootParts& parts, const double* patternWeights, double* siteLogL, double* blockSums,
                                  double* out, int P, int S, int C, unsigned long long* flag, unsigned long long seq, unsigned* counter = nullptr);
// (counter: a zeroed device word, zero again behind the launch — the last workgroup of the site kernel forms the sums; nullptr: a second launch does)
// 4-state walk instances: a wave per 128 patterns with the assembly loop's lane map, the groups' sums as the walk's own root slices leave
// them (kernels_walk4.hip, RootFusedParts) — the same bits whether a partition's root is integrated there or here.  Uses RootPart::root,
// catWeights, freqs, cum, cumIsRaw, pStart, pEnd; blockOff counts 128-pattern groups.
void launchRootLogLikelihoodParts4W(hipStream_t stream, const RootParts& parts, const double* patternWeights, double* siteLogL, double* blockSums,
                                    double* out, int P, int C, unsigned long long* flag, unsigned long long seq, unsigned* counter);

// site[p] = log(sum_c w_c sum_i pi_i root[c][p][i]) + cum[p];  blockSums[b] = sum_p weight[p]*site[p] over block b
// then out[0] = sum_b blockSums[b] in a fixed order (deterministic).  cum may be nullptr; cumIsRaw says the
// buffer holds raw factors (log is taken on the fly).  Restricted to [pStart, pEnd).
void launchRootLogLikelihood(hipStream_t stream, const double* root, const double* catWeights, const double* freqs,
                             const double* cum, int cumIsRaw, const double* patternWeights, double* siteLogL,
                             double* blockSums, double* out, int P, int S, int C, int pStart, int pEnd,
                             unsigned long long* flag = nullptr, unsigned long long seq = 0, unsigned* counter = nullptr);
// (counter: a zeroed device word — the workgroup that finishes last forms the sum itself, one launch instead of two)

// cum[p] += sign * sum_k (raw_k ? log(src_k[p]) : src_k[p]) on [pStart, pEnd); srcs/raws are device arrays.
void launchAccumulateScale(hipStream_t stream, double* cum, const double* const* dSrcs, const int* dRaw,
                           int count, double sign, int pStart, int pEnd);

// The same from what a write-mode walk left behind per SLICE (walk instances, round 6): slice row r holds, per pattern at its position q in
// the pair-interleaved layout (pairPos[p]; nullptr: walkPairIndex(p)), the product of the factors the slice wrote as mantissa[r * stride + q]
// x 2^exponent[r * stride + q];  cum[p] += sign * sum over rows[0 .. n) of (log(mantissa) + exponent ln 2), in that order.
void launchAccumulateSlices(hipStream_t stream, double* cum, const double* mant, const int* expo, const int* dRows, int n, size_t stride,
                            const unsigned* dPairPos, double sign, int pStart, int pEnd);
void launchFill(hipStream_t stream, double* dst, double value, int pStart, int pEnd);
// dst[j][i] = prod_m srcs[m][i] over m in [start[j], start[j + 1]), i < len; worst[j] (zeroed by the caller) = bit pattern of job j's
// largest product, +infinity for anything not finite (kernels.hip k_foldReciprocals)
// invert: the sources are factors (<= 1), the range check is on 1 / product (the T32 walk, which divides by what it reads)
void launchFoldReciprocals(hipStream_t stream, const double* const* dSrcs, const int* dStart, double* const* dDst, int nJobs, int len, unsigned long long* dWorst,
                           bool invert = false, bool pairs = true);        // (pairs: two elements per thread where `len` is even — the same bits)
// out[p] = raw ? log(in[p]) : in[p]
void launchLogScale(hipStream_t stream, const double* in, double* out, int raw, int P);
// Read-back: out[c][p][i] (API layout) = partials * scale, from either device layout.  `scale` may be
// nullptr; scaleIsRaw: the buffer holds raw factors (else logs: the factor is exp).  One pass, then a single D2H.
// walk instances, after the pattern partitions changed: pair[pos[p]] = plain[p] for a tip's states (the rest "missing"), and
// the reciprocal half of a raw scale buffer rebuilt from its factors
void launchRelayoutStates(hipStream_t stream, const uint8_t* oldPlain, uint8_t* newPlain, uint8_t* newPair, const unsigned* dPairPos, int P);
// ... for a list of tips at once: newPair[0 .. pairLen) = missing, then the scatter (two launches whatever the number of tips)
struct RelayoutJob { const uint8_t* oldPlain; uint8_t* newPlain; uint8_t* newPair; };
void launchRelayoutStatesBatch(hipStream_t stream, const RelayoutJob* dJobs, int nJobs, const unsigned* dPairPos, int P, int pairLen, int missing);
void launchRecipFromFactors(hipStream_t stream, const double* factors, double* recip, const unsigned* dPairPos, int P);
void launchExportPartials(hipStream_t stream, const double* partials, const double* scale, int scaleIsRaw, double* out,
                          int P, int S, int C, bool tiled);
// dst[c][p][i] = src[p][i] for every category (setTipPartials replication)
void launchReplicateCategories(hipStream_t stream, const double* src, double* dst, int P, int S, int C);

// ---- pre-order partials and edge derivatives (kernels_preorder.hip) -----------------------------
// One level of pre-order ops.  The OpDesc fields are reused: dest = pre(child), child1 = pre(parent) (always partials),
// mat1 = the child's branch matrix (used transposed), child2 / mat2 = the sibling's post-order partials (or compact
// states, KIND_STATES2) and branch matrix.  Works on either partials layout.
// recipOff != 0: a rescaling op also stores the reciprocal of its factor at scaleWrite[recipOff + walkPairIndex(p)] (walk instances)
void launchPrePartials(hipStream_t stream, const OpDesc* dOps, int nOps, const double* matrices, int P, int S, int C, bool tiled,
                       int maxRange, long recipOff);
struct EdgeDesc {
    const void*   post;          // post-order partials of the node below the edge (double*) or its compact states (uint8*)
    const double* pre;           // pre-order partials of the same node
    const double* tmp;           // launchEdgeReduce only: pre[j] * (D . post)[j], produced by a pass of the pruning kernel
    int           dmat;          // differential matrix index (C*S*S doubles)
    int           postIsStates;
    int           slot;          // output row: perPattern[slot][P], blockSums[slot][blocks][2]
    int           pad;
};
// 16..64 states, T32 layout (kernels_mfma.hip k_edgeTiled): pre and post read once, the product with D on the matrix cores; same
// outputs as launchEdgeDifferentials (blockSums rows of edgeBlocks(P) entries).  EdgeDesc::tmp unused.
bool launchEdgeTiled(hipStream_t stream, const EdgeDesc* dEdges, int nEdges, const double* matrices, const double* catWeights,
                     const double* patternWeights, double* perPattern, double* blockSums, int P, int S, int C);
// 4 states, plain layout (kernels_preorder4.hip): a NODE of the pre-order pass — both children's pre-order partials from one
// read of pre(parent), post(a), post(b), and both edges' derivative sums on the way.  preA / preB may be NULL (not stored);
// slotA / slotB < 0: no derivative asked for that edge; dA / dB: the edges' differential matrices.
struct PreNodeJob {
    const double* preParent;
    const void*   postA;         // double [C][P][4], or uint8 states (statesA)
    const void*   postB;
    double*       preA;
    double*       preB;
    int           matA, matB, dA, dB;
    int           slotA, slotB, statesA, statesB;
    double        pad;
};
static_assert(sizeof(PreNodeJob) == 80, "PreNodeJob layout");
void launchPreNodes4(hipStream_t stream, const PreNodeJob* dJobs, int nJobs, const double* matrices, const double* catWeights,
                     const double* patternWeights, double* blockSums, int P, int C);
// 4 states: the edge derivative SUMS of a whole pre-order list in one launch, no pre-order partial written (kernels_preorder4.hip
// k_preWalk4).  One descriptor per node of the list, in depth-first order; the node's own pre-order partial is in the thread's
// registers (it was produced by the previous descriptor) or in one of the LDS hold slots.
struct PreWalkOp {
    const void*    postA;        // double [C][P][4]; any valid partials buffer when the child is a compact tip
    const void*    postB;
    const uint8_t* tipA;         // uint8 states [P]; any valid states array when the child has partials
    const uint8_t* tipB;
    double*        storeA;       // continuation PW_CONT_STORE: where the child's pre-order partial is written (it heads another segment)
    double*        storeB;
    const double*  recipA;       // 1 / (scale factor of post(a)), pair-interleaved (a walk instance's reciprocal array); all ones when
    const double*  recipB;       // the child is a tip or its partials carry no factor
    int            matA, matB;   // the children's branch matrices
    int            dA, dB;       // the edges' entries in the launch's product array (launchEdgeProducts): the slot, normally
    int            slotA, slotB; // where the edges' sums go (the launch's last slot = nobody asked)
    unsigned       flags;        // PW_* below
    int            pad;
};
static_assert(sizeof(PreWalkOp) == 96, "PreWalkOp layout");
constexpr unsigned PW_TIP_A = 1u, PW_TIP_B = 2u;          // the child is a compact tip
constexpr int PW_SRC_SHIFT = 4, PW_CONT_A_SHIFT = 8, PW_CONT_B_SHIFT = 12;   // 4 bits each
// source of the node's pre-order partial: 0 = the registers, 1 + k = hold slot k
// what becomes of a child's pre-order partial: 0 = nothing below it, 1 = the registers (the next descriptor is that child),
// 2 + k = hold slot k (its descriptor comes after the other child's subtree), PW_CONT_STORE = memory (storeA / storeB)
constexpr unsigned PW_CONT_STORE = 15u;
constexpr int PW_MAX_HOLD = 13;
// A post-order operand that is NOT stored (a gradient chain keeps its tip-tip nodes, and a tip-tip node under one more tip, as
// definitions: engine_preorder.cpp) is re-evaluated from the tips where the walk needs it, by descriptors of a second kind placed
// right in front of the node's own: PW_POSTOP: (M_A x_A) * (M_B tip_B) * recipA -> post slot `dst` (LDS, PW_POST_SLOTS per thread),
// x_A a tip (tipA) or post slot `slotA` (PW_SLOT_A: the inner tip-tip node of the longer kind); matA / matB: the definition's
// private matrix snapshots; recipA: the reciprocal of the node's own scale factor.  Such a descriptor asks for the same loads as
// a node over two tips, writes no sum and leaves the walk's own state alone.  A node descriptor takes an unstored child from its
// slot: PW_SLOT_A / PW_SLOT_B (+ PW_TIP_* so that nothing but a dummy state byte is loaded for it).
constexpr unsigned PW_POSTOP = 1u << 16, PW_SLOT_A = 1u << 17, PW_SLOT_B = 1u << 18;
constexpr int PW_SLOTA_SHIFT = 19, PW_SLOTB_SHIFT = 21, PW_DST_SHIFT = 23;      // 2 bits each
// The shortest unstored operand — a node over two compact tips — is evaluated INSIDE the descriptor of its parent (round 5, second
// form: a descriptor of its own costs a whole stage whatever it computes): PW_CHERRY_A / _B.  For such a child postX points at the
// definition's two branch matrices interleaved lane by lane ({M1[l], M2[l]}, 256 bytes per category: launchCherryPairs), tipX and
// storeX (a node over two tips never heads a segment: nothing is stored for it) at the two tips' states, recipX at the reciprocal of
// the node's OWN scale factor; three loads (one 16-byte, two single bytes) where a stored child asks for two.
constexpr unsigned PW_CHERRY_A = 1u << 25, PW_CHERRY_B = 1u << 26;
// bits 28..31: the vector-memory loads the descriptor asks for (8..12: four matrices, two reciprocal factors, one / two / three per
// child) — what the wait of the descriptor BEFORE it leaves outstanding
constexpr int PW_LOADS_SHIFT = 28;
inline unsigned preWalkLoads(unsigned flags) {
    auto child = [&](unsigned tip, unsigned cherry) { return (flags & cherry) ? 3u : (flags & tip) ? 1u : 2u; };
    return 6u + child(PW_TIP_A, PW_CHERRY_A) + child(PW_TIP_B, PW_CHERRY_B);
}
constexpr int PW_POST_SLOTS = 3;
// A walk is cut into SEGMENTS that run side by side (one more grid dimension): the first one starts at the list's root and
// stores the pre-order partials of the nodes that head the others; those run in a second launch.  progCount even, two more
// no-op descriptors behind every segment.
struct PreWalkSeg { int progStart, progCount; const double* rootPre; };
static_assert(sizeof(PreWalkSeg) == 16, "PreWalkSeg layout");
// sums [nSlots + 1][waves] with waves = preWalkWaves(P, C); dProg[0] is the list's root (what the likelihood is formed from),
// listRootPre its pre-order partial
int  preWalkWaves(int P, int C);
// products: [nSlots + 1][C][16], entry e = (branch matrix of edge e) . (its differential matrix), the spare last one zeros
// (launchEdgeProducts from pairs {matrix, differential matrix}, -1 -1 for zeros); PreWalkOp::dA / dB index it
void launchEdgeProducts(hipStream_t stream, const double* matrices, const int* dPairs, double* products, int C, int n);
// out[k][c][l] = { M[pairs[2 k]][c][l], M[pairs[2 k + 1]][c][l] }, l = 0..15: what a PW_CHERRY child's postX points at
void launchCherryPairs(hipStream_t stream, const double* matrices, const int* dPairs, double* out, int C, int n);
bool launchPreWalk4(hipStream_t stream, const PreWalkOp* dProg, const PreWalkSeg* dSegs, int nSegs, const double* listRootPre,
                    const double* matrices, const double* products, const double* catWeights, const double* patternWeights, double* sums, int P, int C,
                    int holdSlots, bool postSlots = false);
void launchPreWalkFinal(hipStream_t stream, const double* sums, int nSlots, int P, int C, double* out);
// the edge derivatives alone, same shape (32-byte vector accesses); outputs as launchEdgeDifferentials
void launchEdgeDifferentials4(hipStream_t stream, const EdgeDesc* dEdges, int nEdges, const double* matrices, const double* catWeights,
                              const double* patternWeights, double* perPattern, double* blockSums, int P, int C);
int  edgeBlocks(int P);          // workgroups per edge = entries per edge in blockSums (x2 doubles)
// per edge: blockSums[slot][b] = {sum_p w_p num/den, sum_p w_p (num/den)^2} over workgroup b; perPattern (nullable) [slot][P];
// finish with launchEdgeFinal
void launchEdgeDifferentials(hipStream_t stream, const EdgeDesc* dEdges, int nEdges, const double* matrices, const double* catWeights,
                             const double* patternWeights, double* perPattern, double* blockSums,
                             int P, int S, int C, bool tiled);
// same outputs from tmp = pre * (D . post) (see EdgeDesc): num = sum_c w_c sum_j tmp, den = sum_c w_c sum_j pre * post
void launchEdgeReduce(hipStream_t stream, const EdgeDesc* dEdges, int nEdges, const double* catWeights, const double* patternWeights,
                      double* perPattern, double* blockSums, int P, int S, int C, bool tiled);
// outSums[2r], outSums[2r+1] = fixed-order sums of row r's block sums, r < nRows
void launchEdgeFinal(hipStream_t stream, const double* blockSums, int nRows, int P, double* outSums);
// out[S*S] = sum over edges and patterns of the weighted pre x post cross products (see kernels_preorder.hip); partial: [edgeBlocks(P)][S*S]
void launchCrossProducts(hipStream_t stream, const EdgeDesc* dEdges, int nEdges, const double* dEdgeLengths, const double* catWeights,
                         const double* catRates, const double* patternWeights, double* partial, double* out, int P, int S, int C, bool tiled);
// ---- node-height derivatives (kernels_nodeheight.hip; beagleMi355NodeHeightDerivatives) -----------------------------------
// One internal node i with children j, k: pre(i), post(j), post(k) read once, nothing written but the block sums.  Per pattern, with
// x the children's partials (a compact state: its unit vector, all ones when missing), a = P x, b = Q a, c = Q b per child, q = pre(i),
// u = Q_i^T q, v = Q_i^T u and <.> = sum_c w_c sum_s:
//   D = <a_j a_k q>;  g_j = <b_j a_k q> / D, g_k likewise, g_i = <a_j a_k u> / D;  h_jj = <c_j a_k q> / D - g_j^2, h_kk likewise,
//   h_jk = <b_j b_k q> / D - g_j g_k, h_ii = <a_j a_k v> / D - g_i^2, h_ij = <b_j a_k u> / D - g_i g_j, h_ik likewise
//   first  = r_j g_j + r_k g_k - r_i g_i
//   second = r_j^2 h_jj + r_k^2 h_kk + 2 r_j r_k h_jk + r_i^2 h_ii - 2 r_i r_j h_ij - 2 r_i r_k h_ik          (no i terms at the root: dI < 0)
// blockSums[slot][edgeBlocks(P)][2] = {sum_p weight_p first, sum_p weight_p second} per 64 patterns; finish with launchEdgeFinal.
struct NodeHeightJob {
    const double* pre;           // pre-order partials of node i
    const void*   postJ;         // post-order partials of child j (double*) or its compact states (uint8*, statesJ)
    const void*   postK;
    int           matJ, dJ;      // child j's branch matrix and differential matrix (indices into `matrices`, C*S*S doubles each)
    int           matK, dK;
    int           dI;            // node i's differential matrix, < 0 at the root
    int           statesJ, statesK;
    int           slot;
    double        rJ, rK, rI;    // branch rates
};
static_assert(sizeof(NodeHeightJob) == 80, "NodeHeightJob layout");
// 4 states, plain layout: a pattern per lane, 32-byte vector loads, the five matrices of a job wave-uniform; second = false leaves
// every second-order term out (the second block sum is 0)
void launchNodeHeight4(hipStream_t stream, const NodeHeightJob* dJobs, int nJobs, const double* matrices, const double* catWeights,
                       const double* patternWeights, double* blockSums, int P, int C, bool second);
// 2..64 states, either layout.  products: scratch of nodeHeightProductDoubles(nJobs, S, C) doubles the launcher fills first with
// Q_j P_j, Q_j Q_j P_j (and k's) and Q_i Q_i per job, so that every vector the sums need is ONE matrix applied to a partial the
// thread holds (b_j = (Q_j P_j) x_j ...).  false: LDS refused.
size_t nodeHeightProductDoubles(int nJobs, int S, int C);
bool launchNodeHeight(hipStream_t stream, const NodeHeightJob* dJobs, int nJobs, const double* matrices, double* products,
                      const double* catWeights, const double* patternWeights, double* blockSums, int P, int S, int C, bool tiled, bool second);
void launchTransposeMatrices(hipStream_t stream, double* matrices, const int* dSrcDst, int count, int S, int C);
void launchFillFrequencies(hipStream_t stream, double* dest, const double* freqs, int P, int S, int C, bool tiled);

int  pruneBlocksForRange(int S, int range);

// ---- T32 layout (20-/61-state MFMA path, kernels_mfma.hip): partials[c][tile][state][32 patterns] --------------
// One dependency level on the fp64 matrix cores; anyScaleWrite adds the second (max + divide) pass.
// 17..20 states: the walk's programs on the T32 layout (kernels_mfma.hip k_walkT32): same descriptors and segments as the 4-state
// walk (src = plain tip states / T32 partials, scale = the RAW factors, no write mode); dStream from launchGatherFragments over
// the same device program (walkT32StreamBytes)
size_t walkT32StreamBytes(int nEntries, int C, int S);
void launchGatherFragments(hipStream_t stream, const WalkOp* dProg, int nEntries, int C, int S, void* dStream);
// writeMode (a program with write-mode rescaling in it — k_walkT32W1: a workgroup is all categories of one tile, hold slots in registers;
// at most WALK_T32_WRITE_MAX_CATEGORIES of them and two hold slots: false otherwise)
constexpr int WALK_T32_WRITE_MAX_CATEGORIES = 4, WALK_T32_WRITE_MAX_HOLD = 2;
bool launchWalkT32(hipStream_t stream, const WalkOp* dProg, const WalkSeg* dSegs, int nSegs, int maxRange, const void* dStream, int P, int S, int C, int holdSlots,
                   bool writeMode = false);
// 21..64 states: the column tables of a list's virtual cherries (kernels_mfma.hip k_cherryTables), handed to launchPruneLevelTiled
size_t cherryTableBytes(int nCherries, int S, int C);
void launchCherryTables(hipStream_t stream, const CherryDesc* dCherries, int n, const double* matrices, int S, int C, double* out);
void launchPruneLevelTiled(hipStream_t stream, const OpDesc* dOps, int nOps, const double* matrices, int P, int S, int C,
                           bool anyScaleWrite, const CherryDesc* dCherries = nullptr, const double* dCherryTables = nullptr);
// A level of pre-order operations on the T32 layout in ONE pass each (kernels_mfma.hip k_preOpTiled; OpDesc fields as
// launchPrePartials; no write-mode rescaling: such operations take the two passes of the pruning kernel).  false: LDS refused.
bool launchPreOpsTiled(hipStream_t stream, const OpDesc* dOps, int nOps, const double* matrices, int P, int S, int C);
// per-pattern site log-likelihoods + per-block weighted sums (finish with launchRootFinal)
int  rootSiteTiledBlocks(int patterns);      // entries launchRootSiteTiled writes to blockSums for that many patterns
void launchRootSiteTiled(hipStream_t stream, const double* root, const double* catWeights, const double* freqs,
                         const double* cum, int cumIsRaw, const double* patternWeights, double* siteLogL,
                         double* blockSums, int P, int S, int C, int pStart, int pEnd);
// ---- ancestral states (kernels_ancestral.hip; beagleMi355SampleAncestralStates) -----------------------------------------
// One row of the pre-order node list, resolved on the host: the node's partials (plain [C][P][S] or T32) OR its compact tip states
// (uint8 [P], value >= S = unknown), its branch matrix [C][S][S] (nullptr at the root) and the row of its parent (-1 at the root).
struct AncestralRow {
    const double*  partials;
    const uint8_t* states;
    const double*  matrix;
    int            parent;
    int            pad;
};
// states[row][p] (uint8) and cats[p] (may be nullptr) for the instance's P patterns, ONE launch; the random numbers are keyed on
// the global pattern pOffset + p of an alignment of globalP patterns (a shard of the sharded handle draws what one instance would).
// *fpError |= 1 when some draw's total weight was not finite and > 0 (the state is then 0).
void launchSampleAncestral(hipStream_t stream, const AncestralRow* dRows, int nRows, const double* catWeights, const double* freqs,
                           int P, int S, int C, bool tiled, int globalP, int pOffset, unsigned long long seed, bool map,
                           uint8_t* states, int* cats, unsigned* fpError);
// ---- stochastic Dollo node-pattern likelihood (kernels_nodepattern.hip; beagleMi355NodePatternLikelihoods) ---------------
// One row of the post-order node list, resolved on the host: the node's partials (plain [C][P][S] or T32) OR its compact tip states
// (uint8 [P]), its own scale buffer (nullptr: none; raw: factors, not their logarithms), log of its birth weight, its children's
// rows (-1, -1: a tip) and the scratch slots of the row and of its children — a slot is handed out again once its row's parent has
// read it.
struct NodePatternRow {
    const double*  partials;
    const uint8_t* states;
    const double*  scale;
    double         logWeight;
    int            child1, child2;
    int            scaleRaw;
    int            slot, slot1, slot2;
};
int  nodePatternBlocks(int P);               // workgroups over P patterns (entries of blockSums)
// Patterns [p0, p0 + count) of the instance's P, p0 a multiple of 256: logPattern [P] and blockSums [nodePatternBlocks(P)] at their
// global places; lambda (doubles) and below (ints) are [slots][stride] scratch and terms (nullptr: not wanted) the [nRows][stride]
// stage, column p - p0.  blockSums[b] = sum of patternWeights[p] * logPattern[p] over the block's patterns by a fixed tree.
void launchNodePattern(hipStream_t stream, const NodePatternRow* dRows, int nRows, const double* catWeights, const double* freqs,
                       const double* patternWeights, int P, int S, int C, bool tiled, int deathState, int p0, int count, int stride,
                       double* lambda, int* below, double* terms, double* logPattern, double* blockSums);
// ---- marginal node state posteriors (kernels_nodeposterior.hip; beagleMi355NodePosteriors) --------------------------------
// One row of the node list, resolved on the host: the node's post-order partials (plain [C][P][S] or T32) OR its compact tip states
// (uint8 [P]; statesPost != 0), its pre-order partials, and the row of the launch's outputs it fills.
struct NodePosteriorRow {
    const void*   post;
    const double* pre;
    int           statesPost;
    int           slot;
};
static_assert(sizeof(NodePosteriorRow) == 24, "NodePosteriorRow layout");
constexpr int NODE_POSTERIOR_MAX_ROWS = 65535;       // rows of one launch (the grid's second dimension)
// Per row, pattern p and state s: m[s] = sum_c (pre_c[p][s] * post_c[p][s]) * w_c (c ascending from 0.0), Z = sum_s m[s] (s ascending
// from 0.0), posterior = m[s] / Z — NaN, and *fpError = 1, where Z is 0 or not finite.  Outputs of the launch's rows, each nullptr
// when not wanted: posteriors [nRows][P][S], mapStates (uint8) and mapProbabilities [nRows][P] (the first s with the strictly largest
// posterior), blockSums [edgeBlocks(P)][nRows][S] = sum of patternWeights[p] * posterior over the block's 64 patterns by a fixed
// tree (v[i] += v[i + off], off = 32, 16 .. 1); finish those with launchBlockTotals(blockSums, edgeBlocks(P), 1, nRows * S, 0, out).
// false: the state count needs more LDS than a workgroup can have.
bool launchNodePosteriors(hipStream_t stream, const NodePosteriorRow* dRows, int nRows, const double* catWeights,
                          const double* patternWeights, int P, int S, int C, bool tiled, double* posteriors, uint8_t* mapStates,
                          double* mapProbabilities, double* blockSums, unsigned* fpError);
// categories [P][C] of ONE row: n_c = (sum_s pre_c[p][s] * post_c[p][s]) * w_c (s ascending from 0.0), D = sum_c n_c (c ascending
// from 0.0), n_c / D — NaN, and *fpError = 1, where D is 0 or not finite
void launchNodePosteriorCategories(hipStream_t stream, const NodePosteriorRow* dRow, const double* catWeights, int P, int S, int C,
                                   bool tiled, double* categories, unsigned* fpError);
// ---- placement scores (kernels_placement.hip; beagleMi355PlacementScores) --------------------------------------------------
// One candidate attachment, resolved on the host: the parent's pre-order partials; the sibling's post-order partials OR compact
// states (sibStates != 0) with its branch matrix [C][S][S] (both nullptr: no sibling factor); the child's post-order partials OR compact
// states (childStates != 0); the matrices parent -> attachment point (nullptr: identity) and attachment point -> child; which pendant
// table of the call (launchPendantTables) is its own; the row of the launch's table it fills.
struct PlacementCandidate {
    const double* pre;
    const void*   sib;
    const double* mSib;
    const void*   child;
    const double* mUp;
    const double* mLow;
    int           pendant;
    int           sibStates;
    int           childStates;
    int           slot;
};
static_assert(sizeof(PlacementCandidate) == 64, "PlacementCandidate layout");
constexpr int PLACEMENT_MAX_CANDIDATES = 65535;      // candidates of one launch (the grid's second dimension)
constexpr int PLACEMENT_SEGMENT = 8192;              // (pattern, code) entries one accumulator of the score product runs over
// out [nSlots][C][S][X]: G[m][c][a][x] = sum_b M_{slots[m]},c[a][b] * codeTable[x][b], b ascending from 0.0
void launchPendantTables(hipStream_t stream, const double* matrices, const int* dSlots, int nSlots, const double* codeTable, int S, int C,
                         int X, double* out);
// Per candidate k, pattern p, category c and state a (every sum ascending from 0.0):
//   u(a) = pre(a) * sum_b Msib[a][b] sib(b)   (pre(a) without a sibling; compact states: 1.0 at the state, all ones when it is >= S)
//   t(a) = sum_a' u(a') Mup[a'][a]            (u(a) without an upper matrix)
//   e(a) = t(a) * sum_b Mlow[a][b] child(b)
//   D   += w_c * sum_a e(a),   N[x] += w_c * sum_a e(a) G_c[a][x]
// table [slot][P][X] = log(N[x] / D) — NaN, and *fpError = 1, where D is 0 or not finite; -inf where N[x] is 0.
// false: too many candidates, or the state count needs more LDS than a workgroup can have.
bool launchPlacementTable(hipStream_t stream, const PlacementCandidate* dCands, int nCands, const double* catWeights, const double* pendant,
                          int P, int S, int C, int X, bool tiled, double* table, unsigned* fpError);
int  placementPatternBlock(int S, int X);            // patterns a workgroup of launchPlacementTable takes (0: none fit)
// counts [nQueries][P][X] += 1 per site with sitePatterns[site] >= 0 and a code < X (integer atomics); the caller zeroes counts
void launchPlacementCounts(hipStream_t stream, const int* sitePatterns, const uint8_t* codes, int nQueries, int siteCount, int P, int X,
                           int* counts);
// scores [nQueries][nCands] = sum over j = p X + x of counts[q][j] * table[k][j], terms with a count of 0 left out: per segment of
// PLACEMENT_SEGMENT entries ascending from 0.0 into partial [placementSegments][nQueries][nCands], then the segments ascending from 0.0
int  placementSegments(int P, int X);
void launchPlacementScores(hipStream_t stream, const int* counts, const double* table, int nQueries, int nCands, int P, int X, double* partial,
                           double* scores);
// ---- regraft scores (kernels_regraft.hip; beagleMi355RegraftScores) -------------------------------------------------------
// The candidates are PlacementCandidate rows (pendant: which pendant vector of the call, launchRegraftPendants); what is attached is a
// pruned subtree's post-order partials, so there is no code table: one number per (candidate, pattern).
constexpr int REGRAFT_MAX_CANDIDATES = 65535;        // candidates of one launch (the grid's second dimension)
constexpr int REGRAFT_SEGMENT = 64;                 // patterns one accumulator of the weighted pattern sum runs over
// doubles of one pendant vector q [C][P][S] in the instance's partials layout (T32: whole tiles of 32 patterns)
inline size_t regraftPendantDoubles(int P, int S, int C, bool tiled) { return (size_t)C * S * (tiled ? (size_t)((P + 31) >> 5) * 32 : (size_t)P); }
// out [nSlots] vectors of regraftPendantDoubles: q[m][c][p][a] = sum_b M_{slots[m]},c[a][b] * subtree_c,p(b), b ascending from 0.0, in
// the layout of the instance's partials, so that the main stage streams it as a fourth partials buffer.  subtree: partials, or
// (subtreeStates) compact states — 1.0 at the state, all ones when it is >= S.
void launchRegraftPendants(hipStream_t stream, const double* matrices, const int* dSlots, int nSlots, const void* subtree, bool subtreeStates,
                           int P, int S, int C, bool tiled, double* out);
// Per candidate k, pattern p and category c, with u, t, e as for launchPlacementTable and q the candidate's pendant vector (every sum
// ascending from 0.0):   D += w_c * sum_a e(a),   N += w_c * sum_a e(a) q_c(a);
// ratios [slot][P] = log(N / D) + logscale[p] — NaN where D is 0 or not finite (and *fpError = 1 unless patternWeights[p] is 0: no score
// uses it); -inf where N is 0.  scale (nullptr: no term): P log factors, or (scaleRaw) P factors whose logarithm is taken.
// false: too many candidates, or the state count needs more LDS than a workgroup can have.
bool launchRegraftRatios(hipStream_t stream, const PlacementCandidate* dCands, int nCands, const double* catWeights, const double* pendants,
                         const double* scale, bool scaleRaw, const double* patternWeights, int P, int S, int C, bool tiled, double* ratios,
                         unsigned* fpError);
int  regraftPatternBlock(int S);                     // patterns a workgroup of launchRegraftRatios takes (0: none fit)
// scores [nCands] = sum_p patternWeights[p] * ratios[k][p], patterns of weight 0 left out: per segment of REGRAFT_SEGMENT patterns
// ascending from 0.0 into partial [regraftSegments][nCands], then the segments ascending from 0.0 (two launches)
inline int regraftSegments(int P) { return (P + REGRAFT_SEGMENT - 1) / REGRAFT_SEGMENT; }
void launchRegraftScores(hipStream_t stream, const double* ratios, const double* patternWeights, int nCands, int P, double* partial,
                         double* scores);
// ---- sequence simulation (kernels_simulate.hip; beagleMi355SimulateSequences) -------------------------------------------
// One row of the pre-order node list, resolved on the host: its branch matrix [C][S][S] (nullptr at the root), the scratch row
// ("slot") its states go to and the slot of its parent (-1 at the root); parentIsPrev: the parent is the row right before it, whose
// states the site kernel still holds in a register.
struct SimRow {
    const double* matrix;
    int parentSlot, slot, parentIsPrev, pad;
};
constexpr int SIM_SITES_PER_THREAD = 4;      // consecutive sites a thread carries: independent chains, one packed store per row
// The cumulative tables of a call: doubles [(nRows - 1)][C][S] rows of S | the state frequencies' row of S | the category weights'
// row of C, ints (meta) one per row.  A row holds the running maximum of the cumulative sums cum_i (sums in index order), so that
// "the first i with u < cum_i" is "the number of entries that are not above u" whatever the signs of the terms; meta = the largest
// index of a positive term.  A row whose total is not finite and > 0 is all NaN with meta -1: nothing is above u, and the draw
// that falls through to meta finds the error there.
inline size_t simTableRows(int nRows, int S, int C) { return (size_t)(nRows - 1) * C * S + 2; }
inline size_t simTableDoubles(int nRows, int S, int C) { return (size_t)(nRows - 1) * C * S * S + S + C; }
void launchSimTables(hipStream_t stream, const SimRow* dRows, int nRows, const double* catWeights, const double* freqs, int S, int C,
                     double* table, int* meta);
// states[slot][stride] (uint8; stride a multiple of 4) and cats[stride] for sites siteOffset .. siteOffset + nSites - 1 of an
// alignment of siteCount sites, ONE launch.  haveRoot: slot rows[0].slot already holds the root's states; haveCats: cats is given.
// *fpError |= 1 when a vector that was drawn from had a total that is not finite and > 0 (the state is then 0).
void launchSimSites(hipStream_t stream, const SimRow* dRows, int nRows, const double* table, const int* meta, int S, int C,
                    int nSites, size_t stride, unsigned long long siteCount, unsigned long long siteOffset, unsigned long long seed,
                    bool haveRoot, bool haveCats, uint8_t* states, int* cats, unsigned* fpError);
// ---- Markov jumps (kernels_markovjumps.hip; beagleMi355SampleMarkovJumps) ------------------------------------------------
constexpr int MAX_JUMP_REGISTERS = 8;
// One row of the node list: the branch's time and rate, its matrices [C][S][S] (nullptr at the root) and its parent row
struct JumpRow {
    double         time;
    double         rate;
    const double*  matrix;
    int            parent;
    int            pad;
};
// register flags: bit 0 = reward register (rateReg = diag(R)), bit 1 = divide by branchRate * categoryRate.
// rr, tmp, M: [K][S][S] scratch; M[k] = U^-1 rateReg_k U from the (real) eigen system at `eigen` (U | U^-1 | lambda).
void launchJumpRegisters(hipStream_t stream, const double* eigen, const double* registers, const int* regFlags, int K, int S,
                         double* rr, double* tmp, double* M);
// cond[k][r][c][S][S] = (U ((A o M_k) U^-1)) / P_r[c] (then / (rate_r * rate_c) for a scaled register) for rows 1 .. nRows-1
void launchJumpMatrices(hipStream_t stream, const JumpRow* dRows, int nRows, const double* eigen, const double* rates,
                        const double* M, const int* regFlags, int K, int S, int C, double* cond);
int  jumpSiteBlocks(int P);                  // workgroups of launchJumpSites (rows of blockPartials)
// rows [r0, r1) of every pattern: jumps [K][r1-r0][P] (may be nullptr), running pattern totals [K][P] (read unless r0 == 0),
// blockPartials [jumpSiteBlocks(P)][K][nRows]; *fpError |= 2 when some value is not finite
void launchJumpSites(hipStream_t stream, const JumpRow* dRows, int nRows, int r0, int r1, const uint8_t* states, const int* cats,
                     const double* cond, int K, int S, int C, int P, double* jumps, double* patternTotals, double* blockPartials,
                     unsigned* fpError);
// out[k][r] = sum of blockPartials[.][k][r] over `blocks` workgroups in ascending order; rows below firstRow: 0 (every sampler's
// per-workgroup sums: Markov jumps, uniformized jumps, robust counts, unconditioned counts)
void launchBlockTotals(hipStream_t stream, const double* blockPartials, int blocks, int K, int nRows, int firstRow, double* out);
// ---- codon robust counts (kernels_robustcounts.hip; beagleMi355RobustCounts, beagleMi355SimulateUnconditionedCounts) --------
constexpr int ROBUST_STATES = 64;              // the 4 x 4 x 4 product chain
constexpr int ROBUST_MAX_JUMPS = 100000;       // changes after which an unconditioned history is given up (header)
// One row of the node list: tau = branch rate x time, the parent row (-1 at the root), whether the site totals include it
struct RobustRow {
    double tau;
    int    parent;
    int    include;
};
// rr, tmp, M: [K][64][64] scratch; M[k] = U^-1 ((Q o R_k, R's diagonal as 0) U) from the SUPPLIED Q and `eigen` (U | U^-1 | lambda)
void launchRobustRegisters(hipStream_t stream, const double* eigen, const double* Q, const double* registers, int K, double* rr,
                           double* tmp, double* M);
// cond[k][r][64][64] = (U ((A o M_k) U^-1)) / |U (diag(e^(lambda tau)) U^-1)| for rows 1 .. nRows-1 (row 0 is left alone)
void launchRobustTables(hipStream_t stream, const RobustRow* dRows, int nRows, const double* eigen, const double* M, int K,
                        double* cond);
// rows [r0, r1) of every site, the codon of (row, site) = s0 * 16 + s1 * 4 + s2: counts [K][r1-r0][P] (may be nullptr), running
// site totals [K][P] over the included rows (read unless r0 == 0), blockPartials [jumpSiteBlocks(P)][K][nRows] (every row);
// *fpError |= 2 when a gathered value is not finite
void launchRobustSites(hipStream_t stream, const RobustRow* dRows, int nRows, int r0, int r1, const uint8_t* s0, const uint8_t* s1,
                       const uint8_t* s2, const double* cond, int K, int P, double* counts, double* siteTotals,
                       double* blockPartials, unsigned* fpError);
int  unconditionedBlocks(int siteCount);      // workgroups per length row of launchUnconditioned
// one unconditional Gillespie history per (length row in [l0, l1), site): values [K][l1-l0][siteCount] (may be nullptr),
// blockPartials [unconditionedBlocks][K][lengthCount]; *fpError |= 1 for a draw that failed, |= 4 for a history cut at ROBUST_MAX_JUMPS
void launchUnconditioned(hipStream_t stream, const double* Q, const double* freqs, const double* lengths, int lengthCount, int l0,
                         int l1, int siteCount, const double* registers, int K, int S, unsigned long long seed, double* values,
                         double* blockPartials, unsigned* fpError);
// ---- uniformized Markov jumps (kernels_uniformized.hip; beagleMi355SampleMarkovJumpsUniformized) --------------------------
// One row of the node list: the branch's time and rate, the parent's and the node's heights, its matrices [C][S][S] (nullptr at
// the root) and its parent row
struct UniformRow {
    double         time;
    double         rate;
    double         hParent;
    double         hChild;
    const double*  matrix;
    int            parent;
    int            pad;
};
constexpr int UNIFORM_MAX_TRIES = 1000;        // SubordinatedProcess.drawNumberOfChanges' maxTries
constexpr int UNIFORM_MAX_SIMULANTS = 1024;
struct UniformSiteArgs {
    const UniformRow* rows;
    const uint8_t* states;               // the draw's states [nRows][P] and categories [P]
    const int* cats;
    const double* rates;                 // category rates [C]
    const double* table;                 // R^n [N][S][S] (R^0 = I)
    const double* registers;             // [K][S][S]
    const int* regFlags;                 // [K]: bit 0 reward, bit 1 scale by time
    double* stage;                       // values [K][stageRows][P] of the launched rows
    double* blockPartials;               // [jumpSiteBlocks(P)][K][nRows]
    int* eventCounts;                    // [nRows][P] real changes of simulant 0 (nullptr: not counted); offsets when writing
    const long long* patternOffsets;     // [P] first event of each pattern (writing)
    double* eventHeights;                // [events] (writing)
    uint8_t* eventStates;                // [events][2] (writing)
    unsigned* fpError;                   // |= 2 on a failed draw or a value that is not finite
    unsigned long long* fallbacks;       // += histories that took the fallback
    unsigned long long seed;
    double mu;
    int nRows, K, S, P, N, simulants, stageRows, globalP, pOffset;
};
// table[n] = table[n-1] table[1] for n = 2 .. N-1
void launchUniformPowers(hipStream_t stream, double* table, int S, int N);
// rows [r0, r1) of every pattern: values, row sums, counts (write = false), or the events (write = true)
void launchUniformSites(hipStream_t stream, const UniformSiteArgs& a, int r0, int r1, bool write);
// patternTotals [K][P] (+)= stage rows [r0, r1) in row order
void launchUniformPatternTotals(hipStream_t stream, const double* stage, int stageRows, int r0, int r1, int K, int P, double* patternTotals);
// counts [nRows][P] -> offsets within each pattern (in place); patternOffsets [P + 1]: exclusive scan of the pattern sums, then the total
void launchEventOffsets(hipStream_t stream, int* counts, int nRows, int P, long long* patternOffsets);
// ---- complete substitution histories (kernels_history.hip; beagleMi355SimulateCompleteHistories) ---------------------------
constexpr int HISTORY_MAX_STATES = 64;
constexpr int HISTORY_MAX_JUMPS = 100000;      // changes after which a history is given up (header)
constexpr int HISTORY_WAVE = 64;               // sites of one workgroup (one wave); a chunk of sites is a multiple of 4 of them
constexpr int HISTORY_TOTAL_BLOCK = 256;       // sites of one block of the row totals' fixed order
// One row of the node list: the branch's operational time, the parent's and the node's heights, its generator, the scratch rows
// its states and its parent's states are kept in
struct HistoryRow {
    double length;
    double hParent;
    double hChild;
    int    q;
    int    slot;
    int    parentSlot;
    int    parentIsPrev;
};
// Jump tables: one line per (generator, state), then the frequencies' line and the category weights' line.  A line holds the
// running maximum of the cumulative sums in index order (the state's own entry taken as 0), `total` its last cumulative sum,
// `last` the largest index of a positive term (-1: the total is not finite and > 0), `rate` = -Q[i][i] (generator lines only).
inline size_t historyLines(int qCount, int S) { return (size_t)qCount * S + 2; }
inline size_t historyTableDoubles(int qCount, int S, int C) { return (size_t)qCount * S * S + S + C; }
void launchHistoryTables(hipStream_t stream, const double* Q, int qCount, const double* catWeights, const double* freqs, int S, int C,
                         double* table, double* total, double* rate, int* last);
struct HistoryArgs {
    const HistoryRow* rows;
    const double* table;                 // the jump tables and their per-line words
    const double* total;
    const double* rate;
    const int* last;
    const double* catRates;              // [C]
    const double* registers;             // [K][S][S]
    uint8_t* states;                     // [slots][stride]: scratch rows of the chunk
    int* cats;                           // [stride]
    double* stage;                       // values [K][nRows][stride] (nullptr: not wanted)
    double* siteTotals;                  // [K][stride]
    double* wavePartials;                // [stride / 64][K][nRows] (nullptr: no row totals)
    int* eventCounts;                    // [nRows][nSites] (nullptr: not counted)
    const long long* siteOffsets;        // writing: [nSites + 1] first event of each site within the chunk
    double* eventHeights;                // writing: the instance's event list
    uint8_t* eventStates;
    unsigned* fpError;                   // |= 1 for a draw that failed, |= 4 for a history cut at HISTORY_MAX_JUMPS
    unsigned long long seed, siteCount, siteOffset;
    long long eventBase;                 // writing: the chunk's first event in the instance's list
    size_t stride;
    int nRows, K, S, C, nSites, qCount, rewardMask, haveRoot, haveCats;
};
// sites siteOffset .. siteOffset + nSites - 1 of a call over siteCount sites, ONE launch: every history, its end state, every
// register's value, the site totals, the per-wave row sums and the event counts (write = false), or the histories again with their
// events written (write = true)
void launchHistoryWalk(hipStream_t stream, const HistoryArgs& a, bool write);
// rowTotals [K][nRows] (+)= the chunk's blocks of four waves in ascending order (first: from 0.0); row 0: 0
void launchHistoryRowTotals(hipStream_t stream, const double* wavePartials, int waves, int K, int nRows, bool first, double* rowTotals);
// out[0] = sum of n block sums in a fixed order
void launchRootFinal(hipStream_t stream, const double* blockSums, int n, double* out, unsigned long long* flag = nullptr,
                     unsigned long long seq = 0);

// ---- BASTA structured coalescent (kernels_basta.hip): a partial is S doubles, an operation is 8 ints
// {dest, in1, matrix1, in2, matrix2, acc1, acc2, interval number} (include/beagle_mi355.h)
// the whole list in ONE launch: a wave per starting operation (leaves), link = per operation {the operation that reads its result
// or -1, how many inputs of THAT operation the list produces}, tickets = one zeroed word per operation
void launchBastaChains(hipStream_t stream, const int* ops, const int* link, const int* leaves, int nLeaves, unsigned* tickets,
                       const double* matrices, double* partials, const double* sizes, double* coalescent, int S);
// operations [first, first + count) of one interval, each on its own
void launchBastaInterval(hipStream_t stream, const int* ops, int first, int count, const double* matrices, double* partials,
                         const double* sizes, double* coalescent, int S);
// per interval e, f, g, h and its term of the log-density (a wave each, operations in list order), then out[0] = the terms' sum in a fixed order
void launchBastaReduce(hipStream_t stream, const int* ops, const int* intervals, int nIntervals, const double* lengths,
                       const double* partials, const double* sizes, const double* coalescent, double* e, double* f, double* g,
                       double* h, double* intervalLogL, double* out, int S);
// ---- ... its lineage demes (kernels_basta_states.hip; beagleBastaSampleStates).  The draw runs from the roots outwards in CHAINS: a
// chain starts at one input of a coalescence (or at the one input of a root that is no coalescence), draws that input's state from the
// state of the operation's `dest`, and follows the one-input operations that produced the input, one draw each, until it reaches a
// vector the list does not produce or the `dest` of the next coalescence — whose two chains are one level further down.
// The host lays every chain's draws out in the order the wave makes them, so that the wave chases no pointers and can ask for the
// next step while it draws the current one:
// steps: [step] = {input vector, matrix, acc vector of a coalescence's input or -1, interval}, a chain's steps one after another;
// chains: [chain] = {first step, steps, the vector whose state the chain starts from, BASTA_CHAIN_* bits}.
constexpr int BASTA_CHAIN_ROOT = 1;      // that vector is a root: its state is drawn here (by both chains of a root coalescence alike) ...
constexpr int BASTA_CHAIN_STORES_ROOT = 2;   // ... and stored by this one
struct BastaStatesArgs {
    const int4* steps; const int4* chains;
    const double* matrices; const double* partials; const double* freqs;
    uint8_t* states;                     // [vector][stride]: replicate r0 + l of the chunk at column l
    unsigned long long* occupancy;       // [interval][S] or null
    unsigned long long* changes;         // [S][S] or null
    unsigned* error;                     // set when a draw met a total that is not finite and positive
    unsigned long long seed;
    int S, stride, r0, count;            // the chunk: replicates r0 .. r0 + count - 1, count <= stride
    int map, asWritten;
};
// the chains [first, first + n) — one level — for every replicate of the chunk: a wave per (chain, 64 replicates)
void launchBastaStates(hipStream_t stream, const BastaStatesArgs& a, int first, int n);
// out[l][v] = states[v][l] for l < count, v < vectors
void launchBastaStatesTranspose(hipStream_t stream, const uint8_t* states, int vectors, int stride, int count, uint8_t* out);
// ---- ... and its gradient (kernels_basta_gradient.hip; beagleBastaGradient, the rule is in include/beagle_mi355.h): the adjoint of
// every vector, from the roots outwards over the same chains.  Besides steps and chains the wave needs, per step, the interval number
// where e and g of the step's interval live (stepNumbers), and per chain what the coalescence at its top adds:
// chainAux: [chain] = {acc vector of the coalescence's OTHER input or -1, the coalescence's interval number, side (0: in1), 0}.
constexpr int BASTA_GRADIENT_MAX_STATES = 256;
struct BastaGradientArgs {
    const int4* steps; const int4* chains; const int4* chainAux; const int* stepNumbers;
    const int* ops; const int* intervals;
    const double* matrices; const double* partials; const double* sizes; const double* coalescent;
    const double* e; const double* f; const double* g; const double* h;
    const double* lengths;               // [interval]
    const double* distances;             // [interval] or null: no migration-rate gradient
    double* adjoints;                    // [vector][S], zeroed by the caller
    double* w;                           // [vector][S]: at a coalescence's dest, (adjoint - <adjoint, vector> + 1) / J
    double* parts;                       // [interval][S * S + S]: an interval's share of W, then of G_theta
    double* out;                         // [S * S + S]
    int S;
};
// the chains [first, first + n) — one level: a wave per chain, lane = state
void launchBastaGradientSweep(hipStream_t stream, const BastaGradientArgs& a, int first, int n);
// parts: per interval the sums over its operations in list order (a workgroup each); out: the intervals added in index order
void launchBastaGradientReduce(hipStream_t stream, const BastaGradientArgs& a, int nIntervals);

// ---- tip error models (kernels_tipemission.hip): a tip whose partials are a lookup E[code][state], K codes
// matrices[dst][c][i][k] = sum_j matrices[src][c][i][j] E[k][j] (j ascending, no fused multiply-add), zero for k >= K: one job per
// (branch matrix, folded tip) of an operation list, all of them in one launch
struct TipFoldJob { int src, dst, K, pad; const double* emission; };
void launchFoldTipEmission(hipStream_t stream, double* matrices, const TipFoldJob* dJobs, int nJobs, int S, int C);
// dest[c][p][i] = E[codes[p]][i], ones for a code >= K, in the API layout or the T32 layout (its padded patterns zero)
void launchExpandTipEmission(hipStream_t stream, double* dest, const uint8_t* codes, const double* emission, int K, int P, int S, int C,
                             bool tiled);

}  // namespace mi355
