// engine_walk.cpp — 4 states: a planned program (planner.h) resolved to device addresses and run as pattern-walk launches
// (kernels_walk4.hip); materialisation of virtual buffers; updatePartials' steady-state fast path.  See engine_internal.h.
#include "engine_internal.h"
#include <atomic>
#include <unordered_map>

using mi355::OpDesc;

namespace mi355 {
namespace eng {

// ---- folded reciprocal vectors (Instance::folds) ------------------------------------------------------------------------
constexpr int FOLD_MAX_MEMBERS = 32;        // factors per fold: a longer run of unstored nodes is folded in pieces
// largest product of reciprocals a fold may hold (each is >= 1).  An unstored intermediate travels through registers and hold slots
// UNSCALED by the members gathered so far, i.e. as small as 1 / product of its per-node-scaled size: with 1e100 its entries stay
// normal numbers down to 1e-208 of the node's largest entry (per-node read mode keeps them down to 1e-308); beyond, the plan falls
// back to per-node factors (Resolved::noFoldTag)
constexpr double FOLD_SAFE_MAX = 1e100;

// a kept program is no longer good for reuse (its vectors keep their capacity)
static inline void invalidate(Instance::Resolved& r) { r.tag = 0; r.dProgValid = false; r.folds.clear(); r.foldEpoch = -1; }

// forget every fold (their vectors are kept for reuse) and every resolved program that may point at one
static void dropFolds(Instance* in, bool keepVectors) {
    for (Instance::FoldVec& f : in->folds) if (keepVectors && f.recip) in->foldFree.push_back(f.recip);
    if (!keepVectors) in->foldFree.clear();                // (another layout: the old vectors stay with the instance until it is destroyed)
    in->folds.clear(); in->foldIndex.clear();
    for (Instance::Resolved& r : in->resolved) invalidate(r);
}
void forgetFolds(Instance* in) { dropFolds(in, false); scalesWritten(in); }

// the fold of exactly these scale buffers, in this order (index into Instance::folds; < 0: out of memory)
static int foldFor(Instance* in, const std::vector<int>& members) {
    size_t h = 1469598103934665603ull;
    for (int m : members) { h ^= (size_t)(unsigned)m; h *= 1099511628211ull; }
    auto it = std::lower_bound(in->foldIndex.begin(), in->foldIndex.end(), std::make_pair(h, -1));
    for (auto q = it; q != in->foldIndex.end() && q->first == h; ++q)
        if (in->folds[(size_t)q->second].members == members) return q->second;
    Instance::FoldVec f;
    f.members = members;
    if (!in->foldFree.empty()) { f.recip = in->foldFree.back(); in->foldFree.pop_back(); }
    else {
        if (devAlloc(in, (void**)&f.recip, in->scaleStride * sizeof(double))) return -1;
        // (the T32 walk reads whole tiles: what lies past the last pattern must be a number it can divide by)
        if (in->walkT) mi355::launchFill(live(in), f.recip, 1.0, 0, (int)in->scaleStride);
    }
    in->folds.push_back(f);
    const int id = (int)in->folds.size() - 1;
    in->foldIndex.insert(it, std::make_pair(h, id));
    return id;
}

// (re)build the folds of `ids` that are older than the last scale-buffer write; *anyBad: one of `ids` leaves the safe range.
// One launch for all of them, then ONE read-back of the range check — which stalls the stream once per write-mode evaluation
// (DYNAMIC rescaling: every 100th), not per evaluation.
static int refreshFolds(Instance* in, const std::vector<int>& ids, bool* anyBad) {
    std::vector<int> stale;
    for (int id : ids) {
        Instance::FoldVec& f = in->folds[(size_t)id];
        if (f.builtEpoch != in->scaleWriteEpoch) { f.builtEpoch = in->scaleWriteEpoch; stale.push_back(id); }
    }
    if (!stale.empty()) {
        std::vector<const double*> srcs; std::vector<int> start; std::vector<double*> dst;
        for (int id : stale) {
            const Instance::FoldVec& f = in->folds[(size_t)id];
            start.push_back((int)srcs.size());
            for (int m : f.members) srcs.push_back(in->scale[m] + (in->walkT ? 0 : in->scaleStride));    // (reciprocal halves; T32: the factors)
            dst.push_back(f.recip);
        }
        start.push_back((int)srcs.size());
        { int rc = growDevice(in, in->foldWorst, stale.size() * sizeof(unsigned long long),
                              std::max<size_t>(stale.size() + stale.size() / 2, 256) * sizeof(unsigned long long), Grow::KeepOld); if (rc) return rc; }
        HIP_TRY(hipMemsetAsync(in->foldWorst.p, 0, stale.size() * sizeof(unsigned long long), live(in)));
        const int chunk = 2048;                             // (jobs per launch: their pointer lists go through the staging ring)
        for (size_t b = 0; b < stale.size(); b += chunk) {
            const size_t e = std::min(stale.size(), b + chunk);
            std::vector<int> st(start.begin() + b, start.begin() + e + 1);
            const int base = st[0];
            for (int& v : st) v -= base;
            void *dSrcs = nullptr, *dStart = nullptr, *dDst = nullptr;
            int rc = uploadTransient(in, srcs.data() + base, (size_t)st.back() * sizeof(double*), &dSrcs); if (rc) return rc;
            rc = uploadTransient(in, st.data(), st.size() * sizeof(int), &dStart); if (rc) return rc;
            rc = uploadTransient(in, dst.data() + b, (e - b) * sizeof(double*), &dDst); if (rc) return rc;
            mi355::launchFoldReciprocals(live(in), (const double* const*)dSrcs, (const int*)dStart, (double* const*)dDst, (int)(e - b),
                                         in->walkT ? in->P : (int)in->pairLen, in->foldWorst.as<unsigned long long>() + b, in->walkT);
        }
        HIP_TRY(hipGetLastError());
        std::vector<unsigned long long> worst(stale.size());
        int rc = download(in, worst.data(), in->foldWorst.p, worst.size() * sizeof(unsigned long long)); if (rc) return rc;
        for (size_t k = 0; k < stale.size(); k++) {
            double v; memcpy(&v, &worst[k], sizeof(v));
            in->folds[(size_t)stale[k]].bad = !(v <= FOLD_SAFE_MAX);
        }
        in->statFoldBuilds += (long)stale.size();
    }
    *anyBad = false;
    for (int id : ids) if (in->folds[(size_t)id].bad) *anyBad = true;
    return 0;
}

// ---- repeated sub-patterns (Instance::repeatIndex; planner.h RepeatIndex) -------------------------------------------------
// drop every class table (and, `index`, every class index): tip states changed, or the arena is full of clades no list names any more.
// Every kept program may point at a table: all are resolved again.
static void dropRepeatTables(Instance* in, bool index) {
    // (the pool's blocks are kept and handed out again: whatever overwrites them is a copy on the instance's stream, behind every launch
    // that reads the old contents.  Kept programs and slots that wait for an index name clades by their old ids: all are resolved again)
    if (!in->repeatTables.empty() || (index && in->repeatIndex.size())) {
        in->repeatTables.clear();
        in->resolveEpoch++;
        for (Instance::Resolved& r : in->resolved) r.repeatsMissing = false;
    }
    for (Instance::RepeatBlock& b : in->repeatPool) b.used = 0;
    in->repeatRows.reset();
    if (index) { in->repeatIndex.clear(); in->repeatQueue.clear(); }
}
void repeatsForget(Instance* in) { in->repeatSlicingOff = false; if (in->repeatsOn && (in->repeatIndex.size() || !in->repeatTables.empty())) dropRepeatTables(in, true); }

// the row vector of a class table: the pattern's class id (uint16) at its pair position (kernels.h WK_TAB), padded to 256 bytes
static inline size_t repeatRowBytes(const Instance* in) { return (in->pairLen * sizeof(uint16_t) + 255) & ~(size_t)255; }
// the class table of `clade` (its index is built): rows of the arena, the row vector and the representatives' tip states on the device.
// nullptr: no room (*full), or out of memory
static Instance::RepeatTable* repeatTableFor(Instance* in, int clade, bool* full) {
    auto it = in->repeatTables.find(clade);
    if (it != in->repeatTables.end()) return &it->second;
    const mi355::RepeatIndex::Clade& c = in->repeatIndex.clade(clade);
    const int P = in->P, Dpad = (c.D + 127) & ~127;
    if (Dpad > P || !in->repeatArena) return nullptr;
    if (c.D > 65535) return nullptr;                  // (a class id is 16 bits in the row vector, as it is in the index)
    if (in->repeatTableCap && in->repeatTables.size() >= in->repeatTableCap) { *full = true; return nullptr; }
    Instance::RepeatTable t;
    const mi355::RepeatRows before = in->repeatRows;
    if (!in->repeatRows.place(c.D, t.arena, t.row)) { *full = true; return nullptr; }
    t.D = c.D; t.tips = c.tips; t.tipStride = (size_t)Dpad;
    const size_t rowBytes = repeatRowBytes(in);
    t.bytes = rowBytes + t.tips.size() * t.tipStride + 256;
    t.bytes = (t.bytes + 255) & ~(size_t)255;
    // device room from the pool, host room in the pinned staging buffer (wrapping it waits for the copies still reading it: the first
    // evaluation of a large instance at most)
    const size_t expect = std::max<size_t>(8, in->repeatTableCap / 3);
    Instance::RepeatBlock* blk = nullptr;
    for (Instance::RepeatBlock& b : in->repeatPool) if (b.size - b.used >= t.bytes) { blk = &b; break; }
    if (!blk) {
        Instance::RepeatBlock b;
        b.size = std::max(t.bytes, std::min<size_t>((size_t)16 << 20, expect * t.bytes));
        if (devAlloc(in, (void**)&b.dev, b.size)) { in->repeatRows = before; return nullptr; }
        in->repeatPool.push_back(b);
        blk = &in->repeatPool.back();
    }
    if (in->repeatStageSize < t.bytes) {
        (void)hipStreamSynchronize(live(in));
        if (in->repeatStage) hipHostFree(in->repeatStage);
        in->repeatStage = nullptr; in->repeatStageSize = 0; in->repeatStageUsed = 0;
        const size_t want = std::max(t.bytes, std::min<size_t>((size_t)32 << 20, (expect + expect / 4) * t.bytes));
        if (hipHostMalloc((void**)&in->repeatStage, want, hipHostMallocDefault) != hipSuccess) { in->repeatStage = nullptr; in->repeatRows = before; return nullptr; }
        in->repeatStageSize = want;
    }
    if (in->repeatStageSize - in->repeatStageUsed < t.bytes) { (void)hipStreamSynchronize(live(in)); in->repeatStageUsed = 0; }
    unsigned char* const h = reinterpret_cast<unsigned char*>(in->repeatStage + in->repeatStageUsed);
    memset(h, 4, t.bytes);                            // (padding of the tip rows: "missing")
    // (the table's first row is not in the entries: a consumer's descriptor carries its address, ProgramResolver::microOp)
    uint16_t* rows = reinterpret_cast<uint16_t*>(h);
    memset(rows, 0, rowBytes);
    for (int p = 0; p < P; p++) rows[in->pairPos[(size_t)p]] = c.cls[(size_t)p];
    for (size_t k = 0; k < t.tips.size(); k++) {
        const std::vector<uint8_t>& st = in->hostTips[(size_t)t.tips[k]];
        unsigned char* dst = h + rowBytes + k * t.tipStride;
        for (int d = 0; d < c.D; d++) dst[mi355::walkPairIndex((size_t)d)] = st[(size_t)c.rep[(size_t)d]];
    }
    t.dev = blk->dev + blk->used;
    if (hipMemcpyAsync(t.dev, h, t.bytes, hipMemcpyHostToDevice, live(in)) != hipSuccess) { in->repeatRows = before; return nullptr; }
    blk->used += t.bytes; in->repeatStageUsed += t.bytes;
    return &in->repeatTables.emplace(clade, std::move(t)).first->second;
}
static inline const uint8_t* repeatTipRows(const Instance* in, const Instance::RepeatTable& t, int tip) {
    const size_t rowBytes = repeatRowBytes(in);
    for (size_t k = 0; k < t.tips.size(); k++) if (t.tips[k] == tip) return (const uint8_t*)t.dev + rowBytes + k * t.tipStride;
    return nullptr;
}

// Which definitions of a cached read-mode plan are evaluated once per class (slot->repeats; slot->compressed says whether any).  The
// first plan of an instance builds its indices here — the first read-mode evaluation pays for them once —; later a clade the index
// does not know (a topology move made it) is evaluated as before and queued: repeatsIdle builds it where the host waits for a result.
static int prepareRepeats(Instance* in, const mi355::Plan& plan, const mi355::FoldMap* fold, Instance::Resolved* slot) {
    struct Spent { Instance* in; std::chrono::steady_clock::time_point t0;
                   ~Spent() { in->statRepeatBuildUs += (long)std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count(); } } spent{in, std::chrono::steady_clock::now()};
    slot->compressed = false; slot->repeatsMissing = false; slot->lowerRange = 0;
    Instance::WalkTraffic& t = slot->traffic;
    t.tableRows = t.tableReads = t.repeatClades = t.twoTables = t.unstoredConsumers = t.subRuns = t.subRunOps = 0;
    // the index forgets nothing clade by clade: at its capacity everything goes (tables and kept programs with it) and this list's clades
    // are indexed afresh, here — once in thousands of topology moves
    if (in->repeatIndex.overCapacity()) { dropRepeatTables(in, true); in->statRepeatResets++; }
    std::vector<mi355::RepeatRun> cand, take;
    std::vector<int> missing;
    const bool buildNow = in->repeatTables.empty() && in->repeatQueue.empty();
    mi355::findRepeatRuns(plan, fold, in->repeatIndex, buildNow, cand, &missing, in->planner.memDefTables);
    if (!missing.empty()) {
        slot->repeatsMissing = true;
        for (int c : missing) if (std::find(in->repeatQueue.begin(), in->repeatQueue.end(), c) == in->repeatQueue.end()) in->repeatQueue.push_back(c);
    }
    if (cand.empty()) return 0;
    in->repeatTableCap = std::max<size_t>(64, 3 * cand.size());
    if (!in->repeatArena) {
        // (row offsets are 32-bit: the arenas together stay below 4 GiB)
        // twice the rows this plan's tables take (the lists of a chain share their clades; a topology move adds a few), two arenas at least
        const size_t one = (size_t)in->C * in->P * 32;
        size_t need = 0;
        for (const mi355::RepeatRun& r : cand) need += (size_t)((in->repeatIndex.clade(r.clade).D + 127) & ~127);
        const size_t perArena = std::max<size_t>(128, (size_t)in->P & ~(size_t)127);
        int arenas = (int)std::min<size_t>(64, std::max<size_t>(2, (2 * need + perArena - 1) / perArena));
        while (arenas > 1 && (size_t)arenas * one >= ((size_t)1 << 32)) arenas--;
        if (one >= ((size_t)1 << 32)) return 0;
        int rc = devAlloc(in, (void**)&in->repeatArena, (size_t)arenas * one + 512); if (rc) return rc;
        in->repeatArenas = arenas; in->repeatRows.init(arenas, in->P);
    }
    for (int attempt = 0; attempt < 2; attempt++) {
        bool full = false;
        take.clear();
        for (const mi355::RepeatRun& r : cand) {
            if (!repeatTableFor(in, r.clade, &full)) { if (full) break; continue; }
            take.push_back(r);
        }
        if (!full) break;
        // clades of lists long gone fill the arena: start over, the live ones come back as they are asked for (a plan that does not fit
        // even then keeps the tables that do)
        if (attempt == 0) dropRepeatTables(in, false);
    }
    if (take.empty()) return 0;
    mi355::emitRepeatPlan(plan, take, slot->repeats);
    slot->compressed = true;
    t.tableReads = slot->repeats.tableReads; t.repeatClades = (long)slot->repeats.lower.size();
    t.twoTables = slot->repeats.twoTables; t.unstoredConsumers = slot->repeats.unstoredConsumers;
    t.subRuns = slot->repeats.subRuns; t.subRunOps = slot->repeats.subRunOps;
    for (const mi355::PlanSeg& sg : slot->repeats.lower) {
        const Instance::RepeatTable& tab = in->repeatTables[sg.partition];
        t.tableRows += (long)tab.D * sg.progCount;
        slot->lowerRange = std::max(slot->lowerRange, tab.D);
    }
    return 0;
}

// the host is about to wait for a result: a step of the queued index work (one clade node: a pass over the patterns)
void repeatsIdle(Instance* in) {
    if (in->repeatQueue.empty()) return;
    const auto t0 = std::chrono::steady_clock::now();
    int budget = 1;
    const int c = in->repeatQueue.back();
    in->repeatIndex.build(c, &budget);
    if (in->repeatIndex.clade(c).built) in->repeatQueue.pop_back();
    if (in->repeatQueue.empty())
        for (Instance::Resolved& r : in->resolved) if (r.repeatsMissing) { r.tag = 0; r.dProgValid = false; r.repeatsMissing = false; }
    in->statRepeatBuildUs += (long)std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
}

// ---- a plan resolved to a device program (Instance::Resolved) -------------------------------------------------------------------
static int ablateMode() {                              // (LAB builds only — TIMING EXPERIMENTS, wrong results: 1 no stores, 2 no partials loads, 4 no scale traffic, 8 no tip traffic)
    static const int ablate = labEnv("BEAGLE_MI355_ABLATE") ? atoi(labEnv("BEAGLE_MI355_ABLATE")) : 0;
    return ablate;
}
// the plan the device program is made from: the planner's, or the one with its repeated clades taken from class tables (prepareRepeats).
// Its slices come first in Resolved::segs, the class-table programs behind them.
static inline const mi355::Plan& planInUse(const Instance::Resolved& r, const mi355::Plan& plan) { return r.compressed ? r.repeats.plan : plan; }
static inline size_t lowerSlices(const Instance::Resolved& r) { return r.compressed ? r.repeats.lower.size() : 0; }

// Resolution: plan -> r.w / segs / deps / cm, how the program is launched and the traffic it stands for.  Everything that happens once per
// program and not once per run is here: scale and partials buffers come into being (ensureScale, ensurePartials, scaleIsRaw), folds are
// looked up (foldFor), class tables made (prepareRepeats), the slice-sum vectors grown.  Touches no counter of the instance: an error
// leaves them as they were and r invalid.
struct ProgramResolver {
    Instance* const in; const mi355::Plan& plan; Instance::Resolved& r; const long planTag;
    const int ablate = ablateMode();
    const mi355::Plan* use = nullptr;                  // planInUse, once it is decided
    size_t nUp = 0, nLow = 0;                          // its slices, the class-table programs behind them
    mi355::FoldMap foldMap; bool fold = false;
    bool asmLoop = false, ticket = false, sums = false, fuseOk = false;
    unsigned skipLoads = 0;
    std::vector<int> posOf, cur;                       // slice of the planner's plan -> device slice (-1: not emitted yet); a fold's member list
    struct FusedAt { size_t at; int matA, matB; };
    std::vector<FusedAt> fusedAt;
    mi355::WalkOp nop;                                 // loads nothing, stores nothing
    size_t matStride = 0, tipOff = 0;
    // one slice while its micro-operations are emitted
    struct Slice {
        size_t si; bool low;                           // position in the device program; a class-table program (behind the slices of the walk proper)
        const mi355::PlanSeg* ps; const Instance::RepeatTable* tab;
        int lastStore = -1, lastHold = 0, cherry = -1; // what the micro-operation emitted last stores / parks (1 + slot); a cherry waiting to be fused into the next one
    };

    int org(int i) const { return r.compressed ? r.repeats.origin[(size_t)i] : i; }      // the planner's micro-operation (foldMap's index)
    bool paysFactors(int j) const {
        return fold ? foldMap.payStart[(size_t)org(j) + 1] > foldMap.payStart[(size_t)org(j)] : use->prog[(size_t)j].smode == mi355::PS_READ;
    }
    int gatherFrom(int mat) const { const int s = in->snapSourceOf[(size_t)mat]; return s < 0 ? mat : s; }
    // where a compact tip's states are read: the instance's array, or for a class-table program the representatives' rows
    const uint8_t* tipSrc(const Slice& s, int buf) const { return s.low ? repeatTipRows(in, *s.tab, buf) : in->tipStates[buf] ? in->tipStates[buf] + tipOff : nullptr; }

    int run();
    void decideLaunch();
    int chooseProgram();
    int slice(size_t oi);
    int microOp(Slice& s, int i);
    void sliceEpilogue(const Slice& s);
    void finish();
};

// Launch order, and tickets or flags.  4 states, assembly loop: ALL slices in one launch, dispatched critical path first, every workgroup
// waiting for the slices whose stored results it reads (planner.h PlanSeg; kernels_walk4.hip) — instead of one launch per wave of slices
void ProgramResolver::decideLaunch() {
    asmLoop = in->fastWalk && !in->walkT;          // k_walk4_fast runs this program (otherwise k_walk4 / k_walkT32)
    r.oneLaunch = in->fuseWaves && asmLoop && plan.launchOrder.size() == plan.segs.size();
    // ... on tickets when its slices form a forest: the slices without dependencies first (they are the launch's grid), in launch order
    ticket = r.oneLaunch && in->useTickets && plan.leaves > 0;
    // (a slice without micro-operations leaves the kernel before it counts itself in at its next slice, which would then never run and
    // whose ticket words would stay non-zero for the next launch: such a program runs on flags)
    for (size_t i = 0; i < plan.segs.size() && ticket; i++) if (plan.segs[i].progCount <= 0) ticket = false;
    r.order.clear();
    if (r.oneLaunch) {
        r.order = plan.launchOrder;
        if (ticket) std::stable_partition(r.order.begin(), r.order.end(), [&](int s) { return plan.segs[(size_t)s].depCount == 0; });
    }
    r.leaves = ticket ? plan.leaves : 0;
}

// Folds, class tables, slice sums: which plan the program is made from and what its micro-operations may use
int ProgramResolver::chooseProgram() {
    // read-mode programs of cached (full-evaluation) plans fold the reciprocals of unstored nodes (Instance::folds, planner.h FoldMap)
    fold = r.kept && r.noFoldTag != planTag && in->foldScales && (in->walk || in->walkT) && mi355::foldScaleFactors(plan, FOLD_MAX_MEMBERS, foldMap);
    // fused cherries (kernels.h WK_CHERRY): the assembly loop only, and no program that rescales in write mode anywhere (the cherry
    // halves of the kernel's table buffers share their LDS with the maximum buffers of write-mode rescaling)
    bool anyWrite = false;
    for (const mi355::MicroOp& q : plan.prog) if (q.smode == mi355::PS_WRITE) { anyWrite = true; break; }
    const bool noWrites = asmLoop && in->walk && !anyWrite;
    use = &plan;
    if (r.kept && in->repeatsOn && in->walk && !in->walkT && in->partitionCount == 1 && !anyWrite && in->planner.stepLimit == 0 && !plan.runs.empty() &&
        (in->fastWalk || in->C <= 8)) {                // (k_walk4's table variant: up to eight categories, kernels_walk4.hip)
        int rc = prepareRepeats(in, plan, fold ? &foldMap : nullptr, &r); if (rc) return rc;
        if (r.compressed) use = &r.repeats.plan;
        // a list cut for compression (planner.h repeatWeights) of which less than half was compressed — not for want of an index that is
        // still being built —: the lists behind it are cut as they were before (engine_internal.h repeatSlicingOff)
        if (in->planner.lastWeighed > 0 && in->planner.plannedTag == planTag && !r.repeatsMissing) {
            long inRuns = 0, taken = 0;
            for (const mi355::PlanRun& run : plan.runs) inRuns += run.count;
            if (r.compressed) for (const mi355::PlanSeg& sg : r.repeats.lower) taken += sg.progCount;
            if (2 * taken < inRuns) in->repeatSlicingOff = true;
        }
    }
    nUp = use->segs.size(); nLow = lowerSlices(r);
    // write-mode programs: every slice leaves the product of its factors behind (Instance::lastSums); the vectors are named by the last no-op
    // behind the slice's program.  They are the instance's, so growing them invalidates what other kept programs point at.
    sums = anyWrite && in->walk && !in->walkT && in->sliceSums && in->partitionCount == 1;
    if (sums && in->sliceRows < plan.segs.size()) {
        // (both go whatever they hold: sliceRows is 0 after a change of the pair layout, and a failure below leaves it 0 — the next call starts over)
        HIP_TRY(hipStreamSynchronize(live(in)));
        releaseDevice(in, in->sliceMant); releaseDevice(in, in->sliceExp); in->sliceRows = 0;
        const size_t rows = plan.segs.size() + plan.segs.size() / 2 + 8, cells = rows * in->pairLen;
        int rc = growDevice(in, in->sliceMant, cells * sizeof(double), cells * sizeof(double), Grow::SyncIfHeld); if (rc) return rc;
        rc = growDevice(in, in->sliceExp, cells * sizeof(int), cells * sizeof(int), Grow::SyncIfHeld); if (rc) return rc;
        in->sliceRows = rows;
        in->resolveEpoch++;
        in->lastSums.valid = false;
    }
    fuseOk = noWrites && in->fuseCherries;
    // ... and in such programs the loop's fetch skips the tip-state load of a child that is no compact tip (kernels.h WF_NOLOAD1 / 2): a
    // vector-memory instruction less on the CU's address unit for half the children of a tree.  Programs that rescale in write mode keep
    // every fetch at its full size: their stage waits count on it (kernels.h walkStageWaits).
    skipLoads = noWrites && in->skipTipLoads ? (mi355::WF_NOLOAD1 | mi355::WF_NOLOAD2) : 0u;
    return 0;
}

// Device program: per slice its micro-operations, a no-op when their number is odd, and two more no-ops the kernel's descriptor
// prefetch may read (kernels.h WalkSeg)
int ProgramResolver::run() {
    if (in->folds.size() > 4096) dropFolds(in, true);           // (tree shapes come and go; the vectors are reused)
    invalidate(r);                                              // (an error halfway never leaves a reusable half-program)
    r.traffic = Instance::WalkTraffic(); r.compressed = false;
    r.sumRows.clear(); r.wroteScale.clear();
    decideLaunch();
    { int rc = chooseProgram(); if (rc) return rc; }
    r.w.clear();
    r.w.reserve(use->prog.size() + 6 * (nUp + nLow));
    r.segs.assign(nUp + nLow, mi355::WalkSeg());
    r.deps.clear();
    posOf.assign(plan.segs.size(), -1);
    r.maxRange = 0;
    r.finalStore.assign(r.oneLaunch ? nUp : 0, -1); r.finalPart.assign(r.oneLaunch ? nUp : 0, 0);
    matStride = (size_t)in->C * in->S * in->S;
    tipOff = in->walkT ? 0 : in->statePairOff;          // the T32 walk reads the plain state arrays and the RAW scale factors
    // matrices whose snapshot is taken by THIS plan are gathered from the snapshot's source (same values; lets the snapshot copies and
    // the gather run in one launch: kernels_walk4.hip k_gatherAndSnapshot)
    // (a flat table over the matrix slots, entries put back behind the loop: a program on a new tree takes ~1 800 snapshots, and a hash
    // map of them cost 200 of the 270 us this resolution took)
    std::vector<int>& snapSrc = in->snapSourceOf;
    // (an instance with tip emissions: its lists name shadow slots, which lie behind every other slot — engine_tipemission.cpp)
    const size_t snapSlots = in->emis ? (size_t)in->emis->shadowBase + (size_t)in->matrixCount : (size_t)in->planner.matrixSlots();
    if (snapSrc.size() < snapSlots) snapSrc.assign(snapSlots, -1);
    for (size_t q = 0; q + 1 < plan.snapPairs.size(); q += 2) snapSrc[(size_t)plan.snapPairs[q + 1]] = plan.snapPairs[q];
    struct SnapReset { std::vector<int>& t; const std::vector<int>& pairs; ~SnapReset() { for (size_t q = 0; q + 1 < pairs.size(); q += 2) t[(size_t)pairs[q + 1]] = -1; } } snapReset{snapSrc, plan.snapPairs};
    { int rc = ensureWalkDummies(in); if (rc) return rc; }
    memset(&nop, 0, sizeof(nop));
    nop.m1 = in->matrices; nop.m2 = in->matrices;
    nop.src1 = in->dummyTips; nop.src2 = in->dummyTips; nop.scale = in->onesScale;
    nop.flags = (unsigned)((mi355::WK_TIPS << 5) | (mi355::WK_TIPS << 8)) | skipLoads;
    for (size_t oi = 0; oi < nUp + nLow; oi++) { int rc = slice(oi); if (rc) return rc; }
    finish();
    return 0;
}

int ProgramResolver::slice(size_t oi) {
    Slice s;
    s.si = oi; s.low = oi >= nUp;
    const size_t planSlice = s.low ? 0 : r.oneLaunch ? (size_t)r.order[oi] : oi;      // (of the plan in use; a class-table program is none of them)
    s.ps = s.low ? &r.repeats.lower[oi - nUp] : &use->segs[planSlice];
    s.tab = s.low ? &in->repeatTables.find(s.ps->partition)->second : nullptr;      // (PlanSeg::partition of a lower slice: its clade)
    if (!s.low) posOf[planSlice] = (int)oi;
    mi355::WalkSeg& sg = r.segs[oi];
    sg.depStart = (int)r.deps.size();
    if (r.oneLaunch && !s.low) for (int d = s.ps->depStart; d < s.ps->depStart + s.ps->depCount; d++) {
        if (posOf[plan.deps[d]] < 0) return BEAGLE_ERROR_GENERAL;      // (a slice behind one that waits for it: the planner's order forbids it)
        r.deps.push_back(posOf[plan.deps[d]]);
    }
    sg.depCount = (int)r.deps.size() - sg.depStart;
    sg.progStart = (int)r.w.size();
    for (int i = s.ps->progStart; i < s.ps->progStart + s.ps->progCount; i++) { int rc = microOp(s, i); if (rc) return rc; }
    sliceEpilogue(s);
    return 0;
}

// One micro-operation of the plan in use: its operands, what it multiplies by (scale buffer or fold), its store, a cherry fused into it, its flags
int ProgramResolver::microOp(Slice& s, int i) {
    const mi355::Plan& U = *use;
    const mi355::PlanSeg& ps = *s.ps;
    const int progStart = r.segs[s.si].progStart;
    std::vector<mi355::WalkOp>& w = r.w;
    Instance::WalkTraffic& t = r.traffic;
    mi355::MicroOp m = U.prog[i];
    // A cherry that is consumed at once is fused into its consumer (kernels.h WK_CHERRY): tip x tip, not stored, not parked, pays no
    // factors; the next micro-operation of the slice takes it as its second operand (ACC), multiplies by no reciprocals itself (the
    // descriptor's scale field carries the cherry's second tip) and would not come to sit right behind the micro-operation that
    // stores or parks its first child (the loop requests a first child from memory or from an LDS hold slot in the MIDDLE of the
    // stage before — in front of that stage's store and hold-slot write: with the cherry's own stage between them that was safe).
    if (fuseOk && i + 1 < ps.progStart + ps.progCount && m.k1 == mi355::PK_TIPS && m.k2 == mi355::PK_TIPS && m.storeBuf < 0 && m.hold == 0 &&
        !paysFactors(i) && in->tipStates[m.a1] && in->tipStates[m.a2]) {
        const mi355::MicroOp& nx = U.prog[(size_t)i + 1];
        if (nx.k2 == mi355::PK_ACC && !paysFactors(i + 1) && !(nx.k1 == mi355::PK_MEM && s.lastStore == nx.a1) &&
            !(mi355::isHoldKind(nx.k1) && s.lastHold == nx.k1 - mi355::PK_H0 + 1)) { s.cherry = i; return 0; }
    }
    // The kernels request a first child's partials one stage early — before the previous micro-operation's store
    // is issued (kernels_walk4.hip WALK_STAGE).  The planner never emits that sequence (tests/native/plan_check.cpp
    // checks every program for it); should one arrive anyway, a no-op in between restores the distance.
    if ((int)w.size() > progStart && m.k1 == mi355::PK_MEM && s.lastStore == m.a1) {
        if (m.k2 == mi355::PK_ACC) { m.k2 = mi355::PK_MEM; m.a2 = m.a1; }      // the no-op overwrites ACC; the value is in memory as well
        w.push_back(nop);
    }
    // (k_walk4 reads a first child from a class table one stage early, like a hold slot: not in front of a program's first stage)
    if (!asmLoop && (int)w.size() == progStart && m.k1 == mi355::PK_TAB) w.push_back(nop);
    mi355::WalkOp d;
    memset(&d, 0, sizeof(d));
    d.src1 = in->dummyTips; d.src2 = in->dummyTips; d.scale = in->onesScale;     // unused operands stay readable (kernels.h launchWalk4Fast)
    // (the counters are of full-width vectors: a class-table program's reads and stores are tableRows)
    if (m.k1 == mi355::PK_MEM) { d.src1 = in->partials[m.a1]; if (!d.src1 || isCompactTip(in, m.a1)) return BEAGLE_ERROR_OUT_OF_RANGE; t.memReads++; }
    else if (m.k1 == mi355::PK_TIPS) { d.src1 = tipSrc(s, m.a1); if (!d.src1) return BEAGLE_ERROR_OUT_OF_RANGE; if (!s.low) t.tipReads++; }
    if (m.k2 == mi355::PK_MEM) { d.src2 = in->partials[m.a2]; if (!d.src2 || isCompactTip(in, m.a2)) return BEAGLE_ERROR_OUT_OF_RANGE; t.memReads++; }
    else if (m.k2 == mi355::PK_TIPS) { d.src2 = tipSrc(s, m.a2); if (!d.src2) return BEAGLE_ERROR_OUT_OF_RANGE; if (!s.low) t.tipReads++; }
    // a child from a class table (kernels.h WK_TAB): its row vector, and where a write-mode operation has its scale buffer the address
    // of the table's first row — the first table child's; a second one's as a distance from it, in rows
    if (m.k1 == mi355::PK_TAB || m.k2 == mi355::PK_TAB) {
        long firstRow = -1;
        for (int which = 0; which < 2; which++) {
            if ((which ? m.k2 : m.k1) != mi355::PK_TAB) continue;
            const auto tb = in->repeatTables.find(which ? m.a2 : m.a1);
            if (tb == in->repeatTables.end()) return BEAGLE_ERROR_GENERAL;
            (which ? d.src2 : d.src1) = tb->second.dev;
            const long row = (long)tb->second.arena * in->C * in->P + tb->second.row;
            t.tabMaxClasses = std::max(t.tabMaxClasses, (long)tb->second.D);
            if (firstRow < 0) { firstRow = row; d.scaleW = in->repeatArena + (size_t)row * 4; }
            else d.tab2 = (int)(row - firstRow);
        }
    }
    if (m.smode != mi355::PS_NONE) {
        int rc = ensureScale(in, m.scaleIdx); if (rc) return rc;
        if (m.smode == mi355::PS_WRITE) {
            if (in->walkT && !in->walkTWrite) return BEAGLE_ERROR_GENERAL;
            in->scaleIsRaw[m.scaleIdx] = 1; t.scaleWrites++; d.scaleW = in->scale[m.scaleIdx];
            if (sums) { r.wroteScale.push_back(m.scaleIdx); if (r.sumRows.empty() || r.sumRows.back() != (int)s.si) r.sumRows.push_back((int)s.si); }
        } else {
            if (!in->scaleIsRaw[m.scaleIdx]) return BEAGLE_ERROR_OUT_OF_RANGE;   // never written by a rescaling op
            if (!fold) {
                t.scaleReads++;
                d.scale = in->scale[m.scaleIdx] + (in->walkT ? 0 : in->scaleStride);  // read mode multiplies by the reciprocal
            }
        }
    }
    int smodeNow = m.smode;
    if (fold) {                            // multiply by what the planner says this result pays for — nothing, one buffer's reciprocals, a fold
        const int b0 = foldMap.payStart[(size_t)org(i)], b1 = foldMap.payStart[(size_t)org(i) + 1];
        smodeNow = b1 > b0 ? mi355::PS_READ : mi355::PS_NONE;
        if (b1 - b0 == 1) d.scale = in->scale[foldMap.members[(size_t)b0]] + (in->walkT ? 0 : in->scaleStride);
        else if (b1 > b0) {
            cur.assign(foldMap.members.begin() + b0, foldMap.members.begin() + b1);
            const int f = foldFor(in, cur);
            if (f < 0) return BEAGLE_ERROR_OUT_OF_MEMORY;
            r.folds.push_back(f);
            d.scale = in->folds[(size_t)f].recip;
        }
        if (b1 > b0) t.scaleReads++;
    }
    if (m.storeBuf >= 0) {
        int rc = ensurePartials(in, m.storeBuf); if (rc) return rc;
        d.store = in->partials[m.storeBuf];
        t.stored++;
    }
    const bool tableStore = s.low && i == ps.progStart + ps.progCount - 1;      // a class-table program's result: rows of the arena
    if (tableStore) d.store = in->repeatArena + (size_t)s.tab->arena * in->C * in->P * 4;
    d.m1 = in->matrices + (size_t)gatherFrom(m.mat1) * matStride; d.m2 = in->matrices + (size_t)gatherFrom(m.mat2) * matStride;
    int k2 = m.k2;
    if (s.cherry >= 0) {
        const mi355::MicroOp& c = U.prog[(size_t)s.cherry];
        d.src2 = tipSrc(s, c.a1); d.scale = (const double*)tipSrc(s, c.a2);
        if (!d.src2 || !d.scale) return BEAGLE_ERROR_OUT_OF_RANGE;
        k2 = mi355::WK_CHERRY;
        fusedAt.push_back(FusedAt{w.size(), gatherFrom(c.mat1), gatherFrom(c.mat2)});
        if (!s.low) t.tipReads += 2;
        s.cherry = -1;
    }
    d.flags = mi355::walkFlags(m.k1, k2, m.hold, smodeNow, m.storeBuf >= 0 || tableStore);
    if (asmLoop && m.k1 == mi355::PK_TAB) {
        d.flags |= mi355::WF_X | mi355::WF_TAB1;
        t.tabFirst++;
        if ((int)w.size() > progStart) {
            const unsigned pf = w.back().flags;
            if ((pf & mi355::WF_X) && !(pf & mi355::WF_TAB1)) t.tabFirstBehindMem++;
            if (pf & mi355::WF_CHERRY2) t.tabFirstBehindCherry++;
        }
    }
    if (asmLoop && k2 == mi355::PK_TAB) d.flags |= mi355::WF_MEM2 | mi355::WF_TAB2;
    if (m.k1 != mi355::PK_TIPS) d.flags |= skipLoads & mi355::WF_NOLOAD1;
    if (k2 != mi355::PK_TIPS) d.flags |= skipLoads & mi355::WF_NOLOAD2;
    if (ablate) {
        if (ablate & 1) d.flags &= ~(unsigned)mi355::WF_STORE;
        if (ablate & 2) d.flags &= ~(unsigned)mi355::WF_X;
        if (ablate & 4) d.scale = in->onesScale;
        if (ablate & 8) { if (m.k1 == mi355::PK_TIPS) d.src1 = in->dummyTips; if (m.k2 == mi355::PK_TIPS) d.src2 = in->dummyTips; }
    }
    w.push_back(d);
    s.lastStore = m.storeBuf; s.lastHold = m.hold;
    return 0;
}

// Behind a slice's micro-operations: the no-ops its kernel's pipeline needs, where its product of factors goes, the stage waits, its
// pattern range and what a held launch has to know of it
void ProgramResolver::sliceEpilogue(const Slice& s) {
    std::vector<mi355::WalkOp>& w = r.w;
    mi355::WalkSeg& sg = r.segs[s.si];
    // (the kernels' software pipelines: the assembly loop is three micro-operations deep and leaves behind any stage — any
    // length, three more readable descriptors —; the C++ kernel and the T32 walk are two deep: an even length, two more)
    if (!asmLoop && !(in->walkT && in->S > 20) && ((int)w.size() - sg.progStart) % 2) w.push_back(nop);      // (k_walkT64 prefetches nothing across stages)
    sg.progCount = (int)w.size() - sg.progStart;
    for (int q = 0; q < (asmLoop ? 3 : 2); q++) w.push_back(nop);
    if (sums && !r.sumRows.empty() && r.sumRows.back() == (int)s.si) {      // (this slice writes factors: where its product of them goes)
        w.back().scaleW = in->sliceMant.as<double>() + s.si * in->pairLen;
        w.back().store = (double*)(in->sliceExp.as<int>() + s.si * in->pairLen);
    }
    static const int padMode = labEnv("BEAGLE_MI355_WALK_PAD_FETCH") ? atoi(labEnv("BEAGLE_MI355_WALK_PAD_FETCH")) : 1;     // (LAB builds: 0 never, 1 the default, 2 both)
    mi355::walkStageWaits(w.data(), sg.progStart, sg.progCount, asmLoop, in->strictWaits, padMode, /* tableIds */ asmLoop);
    if (s.low) { sg.pStart = s.tab->row; sg.pEnd = s.tab->row + s.tab->D; sg.tStart = 0; sg.next = -1; return; }
    const mi355::PlanSeg& ps = *s.ps;
    sg.pStart = in->partStart[ps.partition]; sg.pEnd = in->partEnd[ps.partition]; sg.tStart = in->padStart[ps.partition];
    r.maxRange = std::max(r.maxRange, sg.pEnd - sg.pStart);
    if (r.oneLaunch) {
        if (ps.progCount > 0) r.finalStore[s.si] = use->prog[(size_t)ps.progStart + ps.progCount - 1].storeBuf;
        r.finalPart[s.si] = ps.partition;
    }
}

// What takes the whole program: the ticket chain, the sinks, the cherry matrices; then r is valid
void ProgramResolver::finish() {
    for (size_t oi = 0; oi < nUp; oi++) {          // (kernels.h WalkSeg::next: rows of THIS array)
        const mi355::PlanSeg& ps = use->segs[r.oneLaunch ? (size_t)r.order[oi] : oi];
        r.segs[oi].next = ticket && ps.next >= 0 ? posOf[(size_t)ps.next] : -1;
    }
    r.sinks = 0; r.sinkRows.clear();
    if (r.oneLaunch) {
        std::vector<char> feeds(r.segs.size(), 0);
        for (int d : r.deps) feeds[(size_t)d] = 1;
        for (size_t i = 0; i < nUp; i++) if (!feeds[i] && r.segs[i].progCount > 0) r.sinkRows.push_back((int)i);
        r.sinks = (int)r.sinkRows.size();
    }
    r.cm.clear();
    if (!fusedAt.empty()) {
        r.cm.assign(2 * r.w.size(), nullptr);
        for (const FusedAt& f : fusedAt) { r.cm[2 * f.at] = in->matrices + (size_t)f.matA * matStride; r.cm[2 * f.at + 1] = in->matrices + (size_t)f.matB * matStride; }
    }
    r.traffic.fused = (long)fusedAt.size();
    for (const mi355::PlanSeg& sg : use->segs) r.traffic.microOps += sg.progCount;
    if (r.kept) r.tag = planTag;
    r.epoch = in->resolveEpoch;
}

static int resolveProgram(Instance* in, const mi355::Plan& plan, long planTag, Instance::Resolved& r) {
    ProgramResolver pr{in, plan, r, planTag};
    return pr.run();
}

// ---- running a resolved program ---------------------------------------------------------------------------------------------------
// the one place where a program's traffic reaches the instance's counters
static void accountTraffic(Instance* in, const Instance::Resolved& r) {
    const Instance::WalkTraffic& t = r.traffic;
    in->statMemReads += t.memReads; in->statTipReads += t.tipReads; in->statScaleReads += t.scaleReads;
    in->statScaleWrites += t.scaleWrites; in->statStored += t.stored; in->statFused += t.fused; in->statMicroOps += t.microOps;
    in->statTableRows += t.tableRows; in->statTableReads += t.tableReads; in->statRepeatClades += t.repeatClades;
    in->statTwoTables += t.twoTables; in->statUnstoredConsumers += t.unstoredConsumers;
    in->statSubRuns += t.subRuns; in->statSubRunOps += t.subRunOps;
    in->statTabFirst += t.tabFirst; in->statTabFirstBehindMem += t.tabFirstBehindMem; in->statTabFirstBehindCherry += t.tabFirstBehindCherry;
    in->statTabMaxClasses = std::max(in->statTabMaxClasses, t.tabMaxClasses);
}

// the slices' products of factors this run leaves behind, and which scale buffers they cover (engine_abi.cpp accumulate)
static void recordSliceSums(Instance* in, const Instance::Resolved& r) {
    if (r.sumRows.empty()) return;
    if (in->scaleGen.size() < (size_t)in->scaleCount) { in->scaleGen.assign((size_t)in->scaleCount, 0); in->scaleSeen.assign((size_t)in->scaleCount, 0); }
    const long gen = ++in->sliceGen;
    for (int idx : r.wroteScale) in->scaleGen[(size_t)idx] = gen;
    in->lastSums.valid = true; in->lastSums.epoch = in->scaleWriteEpoch; in->lastSums.gen = gen; in->lastSums.rows = r.sumRows; in->lastSums.nWritten = (int)r.wroteScale.size();
}

// the folds a kept program reads are those of the scale buffers as they are now; *bad: one of them leaves the safe range
static int refreshProgramFolds(Instance* in, Instance::Resolved& r, bool* bad) {
    *bad = false;
    if (r.folds.empty()) return 0;
    if (r.foldEpoch != in->scaleWriteEpoch) {
        int rc = refreshFolds(in, r.folds, bad); if (rc) return rc;
        r.foldEpoch = in->scaleWriteEpoch;
        if (*bad) return 0;
    }
    in->statFoldedVectors = (long)r.folds.size();
    return 0;
}

// The packed program: [micro-ops (64 B each) | segments (32 B each) | dependency lists | snapshot pairs | the matrices of fused cherries,
// two pointers per micro-operation, where the program has any] — ONE host-to-device copy.  `dev`: where it is on the device; `staged`: the
// program as this call staged it, seen through the ring's device mapping (nullptr: it was resident, or went by another route).
struct PackedProgram {
    struct Part { size_t off; const void* src; size_t bytes; } part[5];        // micro-ops, segments, dependencies, snapshot pairs, cherry matrices
    size_t total = 0;
    int nOps = 0, nPairs = 0;
    char* dev = nullptr; const char* staged = nullptr;
    PackedProgram(const Instance::Resolved& r, const mi355::Plan& plan) : nOps((int)r.w.size()), nPairs((int)(plan.snapPairs.size() / 2)) {
        const size_t opBytes = r.w.size() * sizeof(mi355::WalkOp), segBytes = r.segs.size() * sizeof(mi355::WalkSeg), depBytes = r.deps.size() * sizeof(int);
        const size_t pairBytes = plan.snapPairs.size() * sizeof(int), pairOff = opBytes + segBytes + ((depBytes + 31) & ~(size_t)31);
        part[0] = Part{0, r.w.data(), opBytes};
        part[1] = Part{opBytes, r.segs.data(), segBytes};
        part[2] = Part{opBytes + segBytes, r.deps.data(), depBytes};
        part[3] = Part{pairOff, plan.snapPairs.data(), pairBytes};
        part[4] = Part{pairOff + ((pairBytes + 15) & ~(size_t)15), r.cm.data(), r.cm.size() * sizeof(const double*)};
        total = part[4].off + part[4].bytes;
    }
    const mi355::WalkOp* ops(const char* base) const { return (const mi355::WalkOp*)base; }
    const mi355::WalkSeg* segs(const char* base) const { return (const mi355::WalkSeg*)(base + part[1].off); }
    const int* deps(const char* base) const { return (const int*)(base + part[2].off); }
    const int* pairs(const char* base) const { return (const int*)(base + part[3].off); }
    const double* const* cherryMats(const char* base) const { return part[4].bytes ? (const double* const*)(base + part[4].off) : nullptr; }
};
// the matrix stream of a program: both branch matrices of every micro-operation, in program order; 4 states: 2 x 5 columns x 4 per
// category, and behind them, where the program has fused cherries, the cherry region of the same size (kernels_walk4.hip)
static inline unsigned cherryRegionOff(const Instance* in, const Instance::Resolved& r) {
    return r.cm.empty() ? 0u : (unsigned)(r.w.size() * (size_t)in->C * 40 * sizeof(double));
}
static inline size_t matStreamBytes(const Instance* in, const Instance::Resolved& r) {
    if (in->walkT) return mi355::walkT32StreamBytes((int)r.w.size(), in->C, in->S) + 8192;          // (the kernel's second fragment load reads up to 1.8 KB past an entry)
    return r.w.size() * (size_t)in->C * 40 * sizeof(double) * (r.cm.empty() ? 1 : 2) + 1024;
}

// Put the program where the launches read it: a kept program that is resident stays where it is; otherwise through the staging ring (and
// into the kept program's own device copy), or — a tree of > ~60 000 nodes — through a staging buffer of its own, synchronously
static int stageProgram(Instance* in, Instance::Resolved& r, PackedProgram& pp) {
    if (r.kept && r.dProgValid) { pp.dev = r.dProg.p; return 0; }          // a cached plan's program is already on the device, bit for bit
    if (pp.total > RING_BYTES / 4) {
        HIP_TRY(hipStreamSynchronize(live(in)));
        { int rc = growDevice(in, in->bigStage, pp.total, pp.total, Grow::SyncIfHeld); if (rc) return rc; }      // (its drain finds the stream idle)
        for (const PackedProgram::Part& q : pp.part) if (q.bytes) HIP_TRY(hipMemcpy(in->bigStage.p + q.off, q.src, q.bytes, hipMemcpyHostToDevice));
        pp.dev = in->bigStage.p;
        return 0;
    }
    const long off = stage(in, pp.part[0].src, pp.part[0].bytes, pp.total);      // reserves `total` bytes, copies the ops ...
    if (off < 0) return BEAGLE_ERROR_GENERAL;
    for (int k = 1; k < 5; k++) if (pp.part[k].bytes) memcpy(in->hRing + off + pp.part[k].off, pp.part[k].src, pp.part[k].bytes);      // ... the rest is filled in behind them
    { int rc = queueCopy(in, in->dRing + off, (size_t)off, pp.total); if (rc) return rc; }
    pp.dev = in->dRing + off;
    if (in->kernelUploads) pp.staged = (const char*)in->hRingDev + off;
    if (r.kept) {                                 // keep a device copy for the next time this plan comes out of the cache
        { int rc = growDevice(in, r.dProg, pp.total, pp.total + pp.total / 4, Grow::SyncIfHeld); if (rc) return rc; }
        if (in->kernelUploads) { int rc = queueCopy(in, r.dProg.p, (size_t)off, pp.total); if (rc) return rc; }     // (from the same staged bytes)
        else HIP_TRY(hipMemcpyAsync(r.dProg.p, in->dRing + off, pp.total, hipMemcpyDeviceToDevice, live(in)));
        r.dProgValid = true;
    }
    return 0;
}

// 4 states, a program staged by this call (a partial update, a list the engine has not seen): its upload — and whatever else is
// queued — rides in the gather's launch, which reads the program through the ring's mapping meanwhile (kernels_walk4.hip
// k_gatherAndSnapshot): three launches per such evaluation instead of four.  Not when a queued copy lands in what the gather
// reads or writes (the matrix block, the stream), or two queued copies overlap in part: then they go first, in order (live()).
static bool uploadsCanRide(const Instance* in, const PackedProgram& pp) {
    if (in->walkT || !in->fuseLaunches || !pp.staged || in->pendingCopies.empty() || (int)in->pendingCopies.size() > mi355::HOST_COPY_MAX) return false;
    const char* m0 = (const char*)in->matrices;
    const char* m1 = m0 + (size_t)std::max(1, in->planner.matrixSlots()) * in->C * in->S * in->S * sizeof(double);
    const char* t0 = in->matStream.p; const char* t1 = t0 + in->matStream.bytes;
    const std::vector<Instance::PendingCopy>& pc = in->pendingCopies;
    for (size_t a = 0; a < pc.size(); a++) {
        const char* d0 = (const char*)pc[a].dst; const char* d1 = d0 + pc[a].bytes;
        if ((d0 < m1 && m0 < d1) || (d0 < t1 && t0 < d1)) return false;
        for (size_t b = a + 1; b < pc.size(); b++) {
            const char* e0 = (const char*)pc[b].dst; const char* e1 = e0 + pc[b].bytes;
            if (d0 < e1 && e0 < d1 && !(e0 <= d0 && d1 <= e1)) return false;
        }
    }
    return true;
}
// the queued uploads as the copy list of one launch (the queue is empty afterwards); returns the 4 KiB blocks they take
static unsigned takeQueuedCopies(Instance* in, mi355::HostCopyList& L) {
    L.n = 0;
    unsigned blocks = 0;
    for (const Instance::PendingCopy& pc : in->pendingCopies) {
        mi355::HostCopyList::Entry& e = L.e[L.n++];
        e.dst = pc.dst; e.src = in->hRingDev + pc.ringOff; e.bytes = (unsigned)pc.bytes; e.firstBlock = blocks;
        blocks += (unsigned)((pc.bytes + 4095) / 4096);
    }
    for (int a = 0; a < L.n; a++)                 // (an array queued twice: the later upload wins, the covered one is dropped)
        for (int b = a + 1; b < L.n; b++)
            if ((const char*)L.e[b].dst <= (const char*)L.e[a].dst && (const char*)L.e[a].dst + L.e[a].bytes <= (const char*)L.e[b].dst + L.e[b].bytes) L.e[a].bytes = 0;
    in->pendingCopies.clear();
    return blocks;
}

// The plan's matrix snapshots and the matrix stream (after the snapshots it may name); *rode: the queued uploads went in the same launch
static int gatherMatrices(Instance* in, const Instance::Resolved& r, const PackedProgram& pp, bool* rode) {
    const int elems = in->C * in->S * in->S;
    const bool fusedSnapshot = pp.nPairs && !in->walkT && in->fuseLaunches;          // 4 states: together with the gather below
    if (pp.nPairs && !fusedSnapshot) mi355::launchSnapshotMatrices(live(in), in->matrices, pp.pairs(pp.dev), pp.nPairs, elems);
    const size_t streamBytes = matStreamBytes(in, r);
    { int rc = growDevice(in, in->matStream, streamBytes, std::max(streamBytes + streamBytes / 4, (size_t)1 << 20), Grow::SyncAndFree); if (rc) return rc; }
    *rode = uploadsCanRide(in, pp);
    if (*rode) {
        if (in->pendingWalk.valid) { int rc = flushWalk(in); if (rc) return rc; }          // (cannot be: queueCopy launched it)
        mi355::HostCopyList L;
        const unsigned blocks = takeQueuedCopies(in, L);
        mi355::launchGatherAndSnapshot(in->stream, pp.ops(pp.staged), pp.nOps, in->C, in->matStream.p, in->matrices, pp.pairs(pp.staged), pp.nPairs, elems,
                                       &L, (int)blocks, pp.cherryMats(pp.staged));
    }
    else if (in->walkT) mi355::launchGatherFragments(live(in), pp.ops(pp.dev), pp.nOps, in->C, in->S, in->matStream.p);
    else if (fusedSnapshot) mi355::launchGatherAndSnapshot(live(in), pp.ops(pp.dev), pp.nOps, in->C, in->matStream.p, in->matrices, pp.pairs(pp.dev), pp.nPairs, elems,
                                                           nullptr, 0, pp.cherryMats(pp.dev));
    else mi355::launchGatherMatrices(live(in), pp.ops(pp.dev), pp.nOps, in->C, in->matStream.p, pp.cherryMats(pp.dev));
    return 0;
}

// development (LAB builds, BEAGLE_MI355_DUMP_PLAN): the slices of this program, wave by wave
static void dumpPlan(const Instance::Resolved& r, const mi355::Plan& plan) {
    if (!labEnv("BEAGLE_MI355_DUMP_PLAN")) return;
    const mi355::Plan& UP = planInUse(r, plan);
    const size_t lowN = lowerSlices(r), upN = r.segs.size() - lowN;
    fprintf(stderr, "[mi355] plan: %zu micro-ops in %zu slices (+ %zu class-table programs):", plan.prog.size(), upN, lowN);
    for (size_t i = 0; i < upN; i++) {
        const mi355::PlanSeg& ps = UP.segs[r.oneLaunch ? (size_t)r.order[i] : i];
        fprintf(stderr, " w%d:%d", ps.wave, r.segs[i].progCount);
        if (r.oneLaunch) fprintf(stderr, "(t%d d%d)", ps.tail, ps.depCount);
    }
    fprintf(stderr, "\n");
    if (atoi(labEnv("BEAGLE_MI355_DUMP_PLAN")) > 1)
        for (size_t i = 0; i < r.w.size(); i++)
            fprintf(stderr, "[mi355]   %3zu: k1 %u k2 %u hold %u scale %u store %d\n", i, (r.w[i].flags >> 5) & 7, (r.w[i].flags >> 8) & 7, (r.w[i].flags >> 11) & 3,
                    (r.w[i].flags >> 13) & 3, (r.w[i].flags & mi355::WF_STORE) ? 1 : 0);
}

// the class tables of this evaluation: every class-table program in ONE launch in front of the walk — they wait for nothing, and
// stream order is all the walk needs to find their rows written
static void launchClassTables(Instance* in, const Instance::Resolved& r, const PackedProgram& pp) {
    const size_t lowN = lowerSlices(r);
    in->lowerLaunched = lowN > 0;
    if (!lowN) return;
    const mi355::WalkSeg* dLow = pp.segs(pp.dev) + (r.segs.size() - lowN);
    if (in->fastWalk)
        mi355::launchWalk4Fast(live(in), pp.ops(pp.dev), dLow, (int)lowN, r.lowerRange, in->matStream.p, in->P, in->C, (long)in->scaleStride,
                               nullptr, nullptr, 0, 0, nullptr, 0, nullptr, nullptr, 0, false, cherryRegionOff(in, r));
    else
        mi355::launchWalk4(live(in), pp.ops(pp.dev), dLow, (int)lowN, r.lowerRange, in->matStream.p, in->P, in->C, (long)in->scaleStride);
}

// ONE launch (Resolved::oneLaunch): slice y of the device program is dispatched before slice y + 1 (x fastest), every slice behind the ones
// it waits for; a workgroup signals flags[y][x] = epoch when its stores are out, its dependants poll for exactly that value.  Launched
// now (flushWalk: on tickets or flags), or held back for the root call.
static int launchWalk(Instance* in, const Instance::Resolved& r, const PackedProgram& pp, bool timed) {
    const size_t upN = r.segs.size() - lowerSlices(r);
    const int flagStride = (in->P + 127) / 128 + 1;
    const size_t flagBytes = r.segs.size() * (size_t)flagStride * sizeof(unsigned);
    const size_t want = (std::max(flagBytes + flagBytes / 2, (size_t)1 << 16) + 255) & ~(size_t)255;
    bool grew = false;
    in->walkTickets = nullptr;                                                  // (re-derived below: a failed growth leaves none)
    { int rc = growDevice(in, in->walkFlags, 2 * flagBytes, 2 * want, Grow::SyncAndFree, &grew); if (rc) return rc; }      // [flags | tickets]
    if (grew) HIP_TRY(hipMemsetAsync(in->walkFlags.p, 0, in->walkFlags.bytes, live(in)));
    in->walkTickets = (unsigned*)(in->walkFlags.p + in->walkFlags.bytes / 2);
    if (++in->walkEpoch == 0u) in->walkEpoch = 1u;
    Instance::PendingWalk& pw = in->pendingWalk;
    if (pw.valid) { int rc = flushWalk(in); if (rc) return rc; }            // (cannot happen: every path here went through live())
    pw.prog = pp.ops(pp.dev); pw.segs = pp.segs(pp.dev); pw.deps = pp.deps(pp.dev);
    pw.nSegs = (int)upN; pw.range = r.maxRange; pw.flagStride = flagStride; pw.epoch = in->walkEpoch;
    pw.leaves = r.leaves;
    pw.cherryOff = cherryRegionOff(in, r);
    in->statFastWalks++; in->statWalks++;
    // hold the launch back for the root call?  (one partition, the whole range, not inside a timer bracket)
    // ... and only a program whose slices ALL lead to one last slice: the root call's result word then says that every workgroup
    // of the launch is done (waitResult and its callers reset the staging ring on seeing it) — a forest's other trees could
    // still be running behind the slice that publishes
    // (a partitioned instance, round 6: up to eight partitions in the list, every one ending in ONE slice — the by-partition root call
    // names them all or the launch goes out without it: engine_abi.cpp beagleCalculateRootLogLikelihoodsByPartition)
    const bool holdParts = in->partitionCount > 1 && r.sinks >= 1 && r.sinks <= mi355::ROOT_MAX_PARTS && in->fuseRootParts;
    const bool hold = in->deferWalk && in->fuseLaunches && !timed && ((in->partitionCount == 1 && pw.range == in->P && r.sinks == 1) || holdParts);
    if (hold) {
        pw.finalStore = r.finalStore; pw.finalPart = r.finalPart; pw.sinkRows = r.sinkRows;
        (void)live(in);                           // the program's copies and the gather are enqueued; only the walk itself waits
        pw.valid = true;
        return 0;
    }
    pw.valid = true;
    return flushWalk(in);
}

// one launch per wave of independent slices (a single one unless the planner cut the forest for a small shard)
static int launchWaves(Instance* in, const Instance::Resolved& r, const mi355::Plan& UP, const PackedProgram& pp) {
    const size_t lowN = lowerSlices(r), upN = r.segs.size() - lowN;
    for (size_t b = 0; b < upN;) {
        size_t e = b + 1;
        while (e < upN && UP.segs[e].wave == UP.segs[b].wave) e++;
        int range = 0;
        for (size_t i = b; i < e; i++) range = std::max(range, r.segs[i].pEnd - r.segs[i].pStart);
        if (in->walkT) {
            if (!mi355::launchWalkT32(live(in), pp.ops(pp.dev), pp.segs(pp.dev) + b, (int)(e - b), range,
                                      in->matStream.p, in->P, in->S, in->C, in->holdSlots, r.traffic.scaleWrites > 0)) return BEAGLE_ERROR_GENERAL;
        } else if (in->fastWalk) {                 // the assembly loop (BEAGLE_MI355_NO_FAST_WALK=1: the C++ reference kernel)
            mi355::launchWalk4Fast(live(in), pp.ops(pp.dev), pp.segs(pp.dev) + b, (int)(e - b), range,
                                   in->matStream.p, in->P, in->C, (long)in->scaleStride, nullptr, nullptr, 0, 0, nullptr, 0, nullptr, nullptr, 0, false,
                                   cherryRegionOff(in, r));
            in->statFastWalks++;
        } else
            mi355::launchWalk4(live(in), pp.ops(pp.dev), pp.segs(pp.dev) + b, (int)(e - b), range,
                               in->matStream.p, in->P, in->C, (long)in->scaleStride, lowN > 0);
        in->statWalks++;
        b = e;
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

// nothing to compute (every destination became virtual): the definitions' matrix snapshots still have to be taken
static int snapshotsOnly(Instance* in, const mi355::Plan& plan) {
    if (plan.snapPairs.empty()) return 0;
    void* dPairs = nullptr;
    int rc = uploadTransient(in, plan.snapPairs.data(), plan.snapPairs.size() * sizeof(int), &dPairs); if (rc) return rc;
    mi355::launchSnapshotMatrices(live(in), in->matrices, (const int*)dPairs, (int)(plan.snapPairs.size() / 2), in->C * in->S * in->S);
    HIP_TRY(hipGetLastError());
    return 0;
}

// Run a planned program: resolve it to device addresses (or take the kept resolution of a plan out of the planner's cache: buffer
// addresses never change once a buffer exists), upload it where it is not resident and enqueue the snapshot copies, the gather and the walk.
int runPlan(Instance* in, const mi355::Plan& plan, long planTag, hipEvent_t recordBeforeWalk) {
    typedef std::chrono::steady_clock PhaseClock;                    // (BEAGLE_MI355_HOST_TIMING=2: where a call that resolves a program spends its time)
    const PhaseClock::time_point ph0 = PhaseClock::now();
    if (plan.prog.empty()) return snapshotsOnly(in, plan);
    Instance::Resolved& r = planTag && !ablateMode() ? in->resolved[planTag & 7] : in->scratch;
    r.kept = &r != &in->scratch;
    bool reuse = r.kept && r.tag == planTag && r.epoch == in->resolveEpoch;
    in->lastResolveMiss = !reuse;
    in->lastPlanCached = planTag != 0;
    if (!reuse) { int rc = resolveProgram(in, plan, planTag, r); if (rc) return rc; }
    if (r.traffic.scaleWrites > 0) scalesWritten(in);          // (before the folds are compared with the epoch)
    bool badFolds = false;
    { int rc = refreshProgramFolds(in, r, &badFolds); if (rc) return rc; }
    if (badFolds) {                                // out of range: this plan keeps per-node factors from now on (such a program reads no fold)
        r.noFoldTag = planTag; reuse = false; in->lastResolveMiss = true;
        int rc = resolveProgram(in, plan, planTag, r); if (rc) return rc;
    }
    accountTraffic(in, r);
    recordSliceSums(in, r);
    const PhaseClock::time_point ph1 = PhaseClock::now();
    PackedProgram pp(r, plan);
    { int rc = stageProgram(in, r, pp); if (rc) return rc; }
    const PhaseClock::time_point ph2 = PhaseClock::now();
    bool rode = false;
    { int rc = gatherMatrices(in, r, pp, &rode); if (rc) return rc; }
    dumpPlan(r, plan);
    const PhaseClock::time_point ph3 = PhaseClock::now();
    if (in->hostTrace) {                               // (BEAGLE_MI355_HOST_TIMING=2: what the first few gather launches of the process were made of)
        static std::atomic<int> left{6};
        if (left.fetch_sub(1) > 0)
            fprintf(stderr, "[mi355] gather launch: %zu micro-operations x %d categories%s, %zu matrix snapshots, program %s (%zu bytes), %zu queued uploads ride along\n",
                    r.w.size(), in->C, r.cm.empty() ? "" : " + cherry region", (size_t)pp.nPairs, pp.staged ? "staged by this call" : "on the device",
                    pp.total, rode ? (size_t)1 : (size_t)0);
    }
    if (in->hostTrace && !reuse && plan.prog.size() >= 64) {
        auto us = [](PhaseClock::time_point a, PhaseClock::time_point b) { return std::chrono::duration<double, std::micro>(b - a).count(); };
        fprintf(stderr, "[mi355] program of %zu micro-operations resolved: descriptors and waits %.1f us, upload %.1f us, stream + gather launch %.1f us\n", plan.prog.size(), us(ph0, ph1), us(ph1, ph2), us(ph2, ph3));
    }
    if (recordBeforeWalk) HIP_TRY(hipEventRecord(recordBeforeWalk, live(in)));
    launchClassTables(in, r, pp);
    if (r.oneLaunch) return launchWalk(in, r, pp, recordBeforeWalk != nullptr);
    return launchWaves(in, r, planInUse(r, plan), pp);
}

// Launch the walk that was held back (engine_internal.h PendingWalk) — as it is, or with the slice `root` names finishing the evaluation.
int flushWalk(Instance* in, const mi355::RootFused* root) {
    Instance::PendingWalk& pw = in->pendingWalk;
    if (!pw.valid) return 0;
    pw.valid = false;                                  // (before anything that could come back here through live())
    if (!in->pendingCopies.empty()) { int rc = flushUploads(in); if (rc) return rc; }
#ifdef BEAGLE_MI355_LAB
    // BEAGLE_MI355_WALK_TRACE=<n>: the n-th held-or-not one-launch walk of the instance with more than one slice is timed workgroup by workgroup
    static const int traceAt = labEnv("BEAGLE_MI355_WALK_TRACE") ? atoi(labEnv("BEAGLE_MI355_WALK_TRACE")) : 0;
    static int traceSeen = 0;
    unsigned long long* dTrace = nullptr;
    const int groupsX = (pw.range + 127) / 128;
    if (traceAt > 0 && pw.nSegs > 1 && ++traceSeen == traceAt) {
        HIP_TRY(hipMalloc((void**)&dTrace, (size_t)pw.nSegs * groupsX * 3 * sizeof(unsigned long long)));
        HIP_TRY(hipMemsetAsync(dTrace, 0, (size_t)pw.nSegs * groupsX * 3 * sizeof(unsigned long long), in->stream));
        mi355::setWalkTrace(dTrace);
    }
#endif
    mi355::launchWalk4Fast(in->stream, pw.prog, pw.segs, pw.nSegs, pw.range, in->matStream.p, in->P, in->C, (long)in->scaleStride,
                           pw.deps, in->walkFlags.as<unsigned>(), pw.epoch, pw.flagStride, root, in->walkSpinLimit, in->walkSelfServed,
                           pw.leaves > 0 ? in->walkTickets : nullptr, pw.leaves, in->xcdAware, pw.cherryOff);
#ifdef BEAGLE_MI355_LAB
    if (dTrace) {
        HIP_TRY(hipStreamSynchronize(in->stream));
        std::vector<unsigned long long> t((size_t)pw.nSegs * groupsX * 3);
        HIP_TRY(hipMemcpy(t.data(), dTrace, t.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        mi355::setWalkTrace(nullptr);
        hipFree(dTrace);
        unsigned long long t0 = ~0ull;
        for (size_t i = 0; i < t.size(); i += 3) if (t[i] && t[i] < t0) t0 = t[i];
        fprintf(stderr, "[mi355] walk trace, %d slices x %d groups (us from the first workgroup's entry: entry min..max | wait over min..max | end min..max):\n", pw.nSegs, groupsX);
        for (int s = 0; s < pw.nSegs; s++) {
            double lo[3] = {1e30, 1e30, 1e30}, hi[3] = {0, 0, 0};
            for (int g = 0; g < groupsX; g++)
                for (int k = 0; k < 3; k++) {
                    const unsigned long long v = t[((size_t)s * groupsX + g) * 3 + k];
                    if (!v) continue;
                    const double us = (double)(v - t0) / 100.0;
                    lo[k] = std::min(lo[k], us); hi[k] = std::max(hi[k], us);
                }
            fprintf(stderr, "[mi355]   slice %2d: %6.1f..%6.1f | %6.1f..%6.1f | %6.1f..%6.1f\n", s, lo[0], hi[0], lo[1], hi[1], lo[2], hi[2]);
        }
    }
#endif
    if (root) in->statRootFused++;
    if (pw.leaves > 0) in->statTicketWalks++; else in->statFlagWalks++;
    in->lastLaunchRows = pw.leaves > 0 ? pw.leaves : pw.nSegs; in->lastLaunchSlices = pw.nSegs;
    HIP_TRY(hipGetLastError());
    return 0;
}

// Give every definition of `xs` its real partials: one program, one launch.  xs are definition KEYS (planner.h: buffer x
// partitionCount + partition; the buffer index itself on an instance with one partition).
int materializeList(Instance* in, const std::vector<int>& xs) {
    if (!in->virt || xs.empty()) return 0;
    if (!in->walk && !in->walkT) return materializeCherries(in, xs);
    mi355::Plan mp;
    in->planner.planMaterialize(xs, mp);
    return runPlan(in, mp);
}
int materializeVirtual(Instance* in, int X) {         // every partition of buffer X
    ReadSet reads(in);
    return reads.note(X) ? reads.materialize() : 0;
}
int materializeScaleUsers(Instance* in, int scaleIdx) {
    if (!in->virt || in->planner.scaleUsers(scaleIdx).empty()) return 0;
    return materializeList(in, std::vector<int>(in->planner.scaleUsers(scaleIdx)));
}
int materializeTipUsers(Instance* in, int tip) {
    if (!in->virt || in->planner.tipUsers(tip).empty()) return 0;
    return materializeList(in, std::vector<int>(in->planner.tipUsers(tip)));
}


// A walk is one workgroup per 128 patterns, and every wave executes its program one dependent step after the other.  The
// planner therefore cuts the forest into independent subtrees that run side by side, wave after wave (planner.h): with few
// patterns (a shard of a multi-GPU run, a small alignment) that is what fills the 256 CUs at all (12 500 patterns:
// 0.83 -> 0.33 ms per evaluation); with many it keeps more workgroups than the chip holds in the queue, so that a wave
// waiting for its stores is replaced by another one instead of idling (1e5 patterns: 1.73 -> 1.37 ms).  Returns the target
// number of micro-operations per subtree, 0 = one walk.  BEAGLE_MI355_CHUNK overrides (0 = never).
// This is the cut of a list by its LENGTH: of every program that runs as many micro-operations as the list has operations — write-mode
// evaluations, partial updates, materialisations, the gradient chain, partitioned instances, 16..64 states.  A list that will be
// compressed (class tables) leaves a tenth of them in the walk and is cut by walkRepeatChunkOps below.
int walkChunkOps(const Instance* in, int opCount) {
    static const int forced = labEnv("BEAGLE_MI355_CHUNK") ? atoi(labEnv("BEAGLE_MI355_CHUNK")) : -1;
    if (forced >= 0) return forced;
    // (a short list is one walk — below 64 operations since round 2; on tickets, where a slice above the first wave costs no workgroup
    // slots and no polling, from 32: the reference's benchmark2 alignment — 62 taxa, 44 pattern groups — ran its 61 operations as ONE
    // serial slice, 32 us; cut into three and a top it takes 23: tools/r06_small_sweep.sh)
    if (opCount < (in->fuseWaves && in->fastWalk && !in->walkT && in->useTickets ? 32 : 64)) return 0;
    const long groups = (in->P + 127) / 128;
    // One launch per wave of slices (BEAGLE_MI355_NO_WALK_FUSION=1, the C++ walk, the T32 walk): about 2 560 workgroups per
    // wave, 2.5 rounds of the 1 024 the chip holds (4 per CU).  Measured with the assembly loop (tools/chunk_sweep.sh): 12 500
    // patterns 129 us at 40 micro-operations per slice vs 145 at 99; flat between 50 and 300 from 25 000 patterns up.
    // All slices in ONE launch (the default at 4 states): a wave of slices is no launch and no chip-wide barrier any more, so
    // slices can be longer — fewer stored slice roots, less polling — while the planner keeps the slices ABOVE the first wave
    // short (planner.h chunkTopOps: near the root few subtrees are left side by side).  12 500 patterns, kernel us per
    // evaluation at 40 / 56 / 72 / 96 / 128 micro-operations per first-wave slice: 130 / 122 / 113 / 114 / 114 with 16 above
    // (135 / 122 / 141 / 127 / 122 with the same length above); 25 000 and more: flat (profiles/r04_experiments.txt) — a reading of
    // UNCOMPRESSED programs, whose first wave was eleven twelfths of the work: it does not hold for compressed ones (walkRepeatChunkOps).
    // On tickets (round 6) the grid is the first wave alone: 12 500 patterns, kernel us at 40 / 56 / 70 / 96 / 128 / 150 per first-wave
    // slice with 8 above: 136 / 126 / 125 / 112 / 105 / 106 (16 above: 136 / 131 / 122 / 117 / 109 / 111; flags at their best: 108).
    // 6 250 patterns: 76 us at a divisor of 500, 80 at 765, 99 at 1 400; 25 000 and more: flat.  A partitioned instance's slices span one
    // partition's groups each, so the same divisor means fewer workgroups: config E (4 partitions) is best where it was, 73 us at 1 400 against
    // 91 at 765 (tools/r06_ticket_sweep2.sh, profiles/r06_experiments.txt).
    const bool fused = in->fuseWaves && in->fastWalk && !in->walkT;
    static const long ticketDiv = labEnv("BEAGLE_MI355_CHUNK_DIV") ? atol(labEnv("BEAGLE_MI355_CHUNK_DIV")) : 0;
    // (the T32 walk since it runs three workgroups per CU — 768 places, round 6 —: config B, 20 states, evaluations/s at 40 / 56 / 76 / 100 /
    // 130 / 180 micro-operations per slice: 467 / 467 / 475 / 479 / 480 / 455; 76 is what 2 560 gives there, 102 what 1 900 does)
    // (21..64 states, k_walkT64 — 512 places of four tiles, a stage is microseconds long: config C, 61 states, evaluations/s at 8 / 12 / 16 / 24 /
    // 32 / 48 / 64 micro-operations per slice: 340 / 342 / 338 / 332 / 334 / 336 / 334, one walk: 180 — tools/r06_t64_ring.sh)
    if (in->walkT && in->S > 20) return (int)std::min<long>(150, std::max<long>(8, (long)opCount * groups / 2600));
    const long div = in->walkT ? 1900 : !fused ? 2560 : !in->useTickets ? 1400 : ticketDiv > 0 ? ticketDiv : in->partitionCount > 1 ? 1400 : 765;
    return (int)std::min<long>(150, std::max<long>(24, (long)opCount * groups / div));
}

// The slice sizes of a list that will be compressed (engine_internal.h repeatSlicing), from its weight: the micro-operations compression
// leaves and one per table row gathered (planner.h repeatWeights).  chunk / top arrive as walkChunkOps' and the instance's chunkTopOps.
// BEAGLE_MI355_CHUNK / _CHUNK_TOP override here too.
void walkRepeatChunkOps(const Instance* in, long weight, int& chunk, int& top) {
    static const int forced = labEnv("BEAGLE_MI355_CHUNK") ? atoi(labEnv("BEAGLE_MI355_CHUNK")) : -1;
    if (forced >= 0) { chunk = forced; return; }      // (the top size: taken from the environment at creation)
    if (chunk <= 0) return;                           // (a list too short to cut at all: one walk, as before)
    // Measured on the 1000-taxon coalescent tree, whose compressed program is 78 micro-operations and 76 gathers (evaluations/s at 24 / 32 /
    // 48 / 64 / 80 / 100 per first-wave slice, one walk, and the cut of the uncompressed list; profiles/compressed_slicing.txt):
    //   1e5 patterns     2 306 / 2 416 / 2 622 / 2 712 / 2 708 / 2 719, one walk 2 582, uncompressed cut 2 437 .. 2 452
    //   25 000 patterns  5 009 / 5 409 / 6 075 / 6 482 /   -   / 6 305,                 uncompressed cut 5 456 .. 5 490
    // Slices of 9 to 20 micro-operations that remain — eight of them where the uncompressed cut made eighteen of 1 to 12 — and one wave
    // above them: the size above the first wave (8 or 32) has nothing left to act on and stays.  With fewer groups than compression is on
    // for by default (BEAGLE_MI355_REPEATS_ANY_SIZE=1 only) the divisor of walkChunkOps sizes the slices, from the weight.
    const long groups = (in->P + 127) / 128;
    chunk = groups >= 128 ? 64 : (int)std::min<long>(64, std::max<long>(24, weight * groups / 765));
}

// 4 states: the operation list becomes one (or, for a list with hazards, a few) pattern-walk launches.
int runOperationsWalk(Instance* in, const int* ops, int count, int tuple, int globalCum) {
    if (count <= 0) return 0;
    typedef std::chrono::steady_clock Clock;
    const Clock::time_point t0 = Clock::now();
    auto usSince = [](Clock::time_point a) { return std::chrono::duration<double, std::micro>(Clock::now() - a).count(); };
    in->hostCalls++;
    const int parts = in->partitionCount;
    // destinations may become virtual: 7-int lists of an unpartitioned instance, 9-int lists (definitions are per partition)
    bool allowVirtual = tuple == BEAGLE_PARTITION_OP_COUNT || parts == 1;
    // (gradient evaluations want the partials of every node the pre-order pass cannot re-evaluate itself: engine_preorder.cpp
    // runPreOperations, walkableDefinition)
    struct StepLimit { mi355::WalkPlanner& pl; ~StepLimit() { pl.stepLimit = 0; } } stepLimitGuard{in->planner};
    if (in->storeAllEvaluations > 0) {
        in->storeAllEvaluations--;
        if (in->gradientVirtual && parts == 1 && tuple == BEAGLE_OP_COUNT) in->planner.stepLimit = in->gradientVirtualSteps;
        else allowVirtual = false;
    }
    // The chain's steady state — the SAME full-evaluation list as one seen before, no rescaling in it — needs none of the
    // per-operation work below: it was range-checked and planned then, nothing has to be materialised or accumulated for it,
    // the planner re-establishes its definitions with one comparison per operation and the program is resident on the
    // device (config E, 6 436 operations: 116 -> 35 us of host time per call; profiles/r03_experiments.txt).
    // (a list that will be compressed is cut by what is left of it: planner.h repeatWeights acts on closed lists without rescaling only)
    in->planner.repeatWeights = in->repeatSlicing && !in->repeatSlicingOff && parts == 1 && allowVirtual && in->planner.stepLimit == 0;
    in->planner.preferSeenCap = in->closedListRun >= 2;
    {
        bool simple = false;
        if (in->planner.replayCached(ops, count, tuple, parts, allowVirtual, walkChunkOps(in, count), &simple)) {
            in->closedListRun++;
            const double usPlan = usSince(t0);
            in->hostPlanUs += usPlan; in->hostPlanHitUs += usPlan; in->hostHits++;
            const Clock::time_point t1 = Clock::now();
            CallTimer timer(in);
            if (!in->planner.planned->prog.empty()) { int rce = timer.begin(); if (rce) return rce; }
            int rc = runPlan(in, *in->planner.planned, in->planner.plannedTag, timer.first()); if (rc) return rc;
            rc = timer.stop(in->lowerLaunched ? 2 : 1); if (rc) return rc;
            const double usRun = usSince(t1);
            in->hostRunUs += usRun; in->hostRunHitUs += usRun;
            if (in->hostTrace && usPlan + usRun > 40.0)
                fprintf(stderr, "[mi355] call %ld (replayed, tag %ld): planner %.1f us, run %.1f us (resolved again: %d, folds rebuilt so far %ld)\n", in->hostCalls,
                        in->planner.plannedTag, usPlan, usRun, (int)in->lastResolveMiss, in->statFoldBuilds);
            return 0;
        }
    }
    for (int k = 0; k < count; k++) {
        const int* op = ops + (size_t)k * tuple;
        const int dest = op[0], wS = op[1], rS = op[2], c1 = op[3], m1 = op[4], c2 = op[5], m2 = op[6];
        int part = 0, cum = globalCum;
        if (tuple == BEAGLE_PARTITION_OP_COUNT) { part = op[7]; cum = op[8]; }
        if (badIndex(dest, in->partialsCount) || badIndex(c1, in->partialsCount) || badIndex(c2, in->partialsCount) ||
            badMatrix(in, m1) || badMatrix(in, m2) || badIndex(part, parts) ||
            (wS != BEAGLE_OP_NONE && badIndex(wS, in->scaleCount)) || (rS != BEAGLE_OP_NONE && badIndex(rS, in->scaleCount)) ||
            (cum != BEAGLE_OP_NONE && badIndex(cum, in->scaleCount)))
            return BEAGLE_ERROR_OUT_OF_RANGE;
    }
    CallTimer timer(in);
    { int rce = timer.begin(); if (rce) return rce; }
    int launches = 0;
    in->hostPrepUs += usSince(t0);
    for (int begin = 0; begin < count;) {
        Clock::time_point t1 = Clock::now();
        const int n = in->planner.hazardFreePrefix(ops, begin, count, tuple, parts);
        const int* sub = ops + (size_t)begin * tuple;
        for (int k = 0; k < n; k++) {                       // a tip index reused as a destination now holds partials
            const int dest = sub[(size_t)k * tuple];
            if (isCompactTip(in, dest) || in->planner.leafPartials[dest]) { int rcm = materializeTipUsers(in, dest); if (rcm) return rcm; in->tipStates[dest] = nullptr; setCompact(in, dest, false); }
        }
        std::vector<int> need;
        in->planner.mustMaterializeBefore(sub, n, tuple, need);
        // (long memory definitions the list only reads — a branch move's siblings — are stored once, not walked by every move that passes them)
        if (allowVirtual && in->planner.stepLimit == 0) in->planner.longMemoryOperands(sub, n, tuple, in->memDefInlineSteps, need);
        { int rc = materializeList(in, need); if (rc) return rc; }
        in->hostPrepUs += usSince(t1); t1 = Clock::now();
        const long hitsBefore = in->planner.cacheHits;
        int rc = in->planner.plan(sub, n, tuple, parts, allowVirtual, in->plan, walkChunkOps(in, n));
        if (rc) return rc;
        const bool hit = in->planner.cacheHits != hitsBefore;
        in->closedListRun = in->planner.plannedTag ? in->closedListRun + 1 : 0;
        double usPlanThis = 0.0;
        { const double us = usSince(t1); usPlanThis = us; in->hostPlanUs += us; if (hit) { in->hostPlanHitUs += us; in->hostHits++; } }
        t1 = Clock::now();
        // with the kernel timer on, ONE HIP-event pair brackets the walk launches of the call (the program upload and the
        // snapshot copies are outside: the events time the pruning kernel, which is what the roofline is about)
        const bool walks = !in->planner.planned->prog.empty();
        rc = runPlan(in, *in->planner.planned, in->planner.plannedTag, walks ? timer.first() : nullptr); if (rc) return rc;
        if (walks) launches += in->lowerLaunched ? 2 : 1;
        { const double us = usSince(t1); in->hostRunUs += us; if (hit) in->hostRunHitUs += us;
          if (in->hostTrace && usPlanThis + us > 40.0)
              fprintf(stderr, "[mi355] call %ld (%d ops from %d, cache %s, tag %ld): planner %.1f us, run %.1f us (resolved again: %d, folds rebuilt so far %ld)\n", in->hostCalls, n, begin,
                      hit ? "hit" : "miss", in->planner.plannedTag, usPlanThis, us, (int)in->lastResolveMiss, in->statFoldBuilds); }
        begin += n;
    }
    { int rce = timer.stop(launches); if (rce) return rce; }
    return foldCumulative(in, ops, count, tuple, globalCum);
}


}  // namespace eng
}  // namespace mi355
