// planner.h — the walk planner: turns an updatePartials operation list into the micro-operation program the 4-state
// pattern-walk kernel executes (kernels_walk4.hip), and keeps the definitions of "virtual" partials buffers.
//
// Pure host logic: no HIP types, no device pointers — everything is expressed in buffer / matrix / scale INDICES; the
// engine resolves them to addresses (engine_walk.cpp).  That keeps the planner testable without a GPU: tests/native/ holds
// an index-level interpreter of the micro-operations and checks planner output against list-order evaluation.
//
// Reference behaviour this has to preserve (all paths relative to /root/reference):
//   * an operation list is any dependency-ordered list of 7-int tuples {dest, writeScale, readScale, child1, matrix1,
//     child2, matrix2} (src/dr/evomodel/treelikelihood/BeagleTreeLikelihood.java:1266-1299), post-order or the reverse
//     level order of src/dr/evomodel/treedatalikelihood/LikelihoodTreeTraversal.java:133-205; 9-int tuples add
//     {partition, cumulativeScale} (MultiPartitionDataLikelihoodDelegate.java:972-997);
//   * every buffer index is independent storage that keeps the value its last operation gave it
//     (src/dr/evomodel/treedatalikelihood/BufferIndexHelper.java:71-106 flips between two indices per node and expects
//     the unflipped one to survive a rejected proposal).
#pragma once
#include <cstddef>
#include <cstdint>
#include <functional>
#include <unordered_map>
#include <vector>

namespace mi355 {

constexpr int PLAN_MAX_STEPS = 32;       // capacity of a virtual definition (snapshot slots per buffer = 2 * this)
constexpr int PLAN_NONE = -1;

// kinds / scale modes: numerically identical to WK_* / WS_* of kernels.h (static_assert in engine_internal.h)
enum { PK_MEM = 0, PK_TIPS = 1, PK_ACC = 2, PK_H0 = 3, PK_H1 = 4, PK_H2 = 5, PK_TAB = 7 };
// PK_TAB (first or second child; only in programs emitRepeatPlan made, below): the child is a clade over compact tips whose value was
// evaluated once per distinct sub-pattern into a class table; a = the clade (RepeatIndex id).  Not a hold slot: compare kinds against
// PK_H0 .. PK_H2, not ">= PK_H0".
inline bool isHoldKind(int k) { return k >= PK_H0 && k <= PK_H2; }
enum { PS_NONE = 0, PS_READ = 1, PS_WRITE = 2 };

struct MicroOp {
    int storeBuf;        // partials buffer that receives the result, or PLAN_NONE
    int k1, a1;          // first child: kind, and the partials / tip buffer index for PK_MEM / PK_TIPS
    int k2, a2;          // second child (PK_MEM, PK_TIPS or PK_ACC)
    int mat1, mat2;      // matrix slot of each child's branch (caller's index, or a snapshot slot >= matrixCount)
    int scaleIdx, smode; // scale buffer and PS_*
    int hold;            // 0, or 1 + hold slot that ALSO receives the result
};

// A program slice: every pattern group of `partition` walks it.  Slices of the same `wave` are independent of each other
// (one launch); a slice may read what slices of EARLIER waves stored.
// depStart / depCount: the slices whose stored results this one reads (indices into Plan::segs, all of earlier waves), as a
// range of Plan::deps.  tail: micro-operations from the start of this slice to the end of the last slice that (transitively)
// waits for it — the critical path behind it.  A single launch may run ALL slices side by side when every workgroup first
// waits for the slices in its dependency list (same pattern group) and the slices are dispatched by descending tail — an
// order in which every slice comes after the ones it reads (tail(child) > tail(parent)); Plan::launchOrder is that order.
// next: the ONE slice that waits for this one (-1: none — a root of the forest; meaningful when Plan::leaves > 0).  A slice's stored
// result normally has one reader, so the slices form a forest and a launch needs no waiting at all: only the slices without
// dependencies ("leaves") get workgroups, a workgroup that finishes slice s counts itself in at s.next for its pattern group, and
// the one that arrives LAST there carries on with that slice itself — everything it reads was stored by workgroups that counted
// in before it (kernels_walk4.hip: "tickets").
struct PlanSeg { int progStart, progCount, partition, wave, depStart, depCount, tail, next; };
// micro-operations [start, start + count) of Plan::prog evaluate ONE definition inside its consumer's program (emitReal): the result of the
// last of them is in ACC for the micro-operation that follows, or parked in a hold slot for a later one of the same slice
struct PlanRun { int start, count; };

struct Plan {
    std::vector<MicroOp> prog;
    std::vector<PlanSeg> segs;       // sorted by wave
    std::vector<int> deps;           // PlanSeg::depStart / depCount
    std::vector<int> launchOrder;    // permutation of segs: descending tail (critical path first), dependencies before dependants
    std::vector<int> snapPairs;      // (source matrix slot, destination snapshot slot) pairs to copy BEFORE the program runs
    std::vector<PlanRun> runs;       // the definitions plan() evaluated inside a real operation's program, in program order (findRepeatRuns)
    int leaves = 0;                  // > 0: the slices form a forest (every slice has at most one dependant, none is empty) and this many of
                                     // them wait for nothing — the program can run on tickets (PlanSeg::next); 0: dependency flags only
    void clear() { prog.clear(); segs.clear(); deps.clear(); launchOrder.clear(); snapPairs.clear(); runs.clear(); leaves = 0; }
};

// Read-mode programs: where the reciprocal scale factors are applied.  A result that is not stored is seen by nobody but the
// micro-operation that consumes it, and a partial is linear in each of its children — so an unstored result may pass the
// factors it owes (its own and those its unstored operands passed on) to its consumer, and only a result that IS stored, that
// ends its slice, or that has gathered `maxMembers` of them pays: one multiplication by the product of the members'
// reciprocals.  foldScaleFactors says, per micro-operation of plan.prog, which scale buffers it pays for:
// members[payStart[i] .. payStart[i + 1]), in ascending order (none: it multiplies by nothing; one: that buffer's own reciprocals; several: a fold the
// engine builds, engine_walk.cpp).  false: the program rescales in write mode somewhere (nothing is folded then).
struct FoldMap { std::vector<int> payStart, members; };
bool foldScaleFactors(const Plan& plan, int maxMembers, FoldMap& out);

// ---- repeated sub-patterns -----------------------------------------------------------------------------------------------
// The partial of a node depends on the states of the tips below it and on nothing else of a pattern, and real alignments repeat: under a
// clade of a dozen tips the 1e5 patterns of a 1000-taxon alignment show a few hundred distinct sub-patterns.  RepeatIndex keeps, per clade
// over compact tips, the CLASS of every pattern (patterns of a class agree on every tip of the clade), the class count D and one
// representative pattern per class (the smallest).  Built bottom-up from the children's classes (key = class(A) * D(B) + class(B); a tip's
// class is its state code, every code >= 4 one class), memoised by the two child clades — tips as leaves — so that whatever a new operation
// list keeps of the tree finds its clades here, whichever buffers the nodes sit in.  Pure host data; the engine owns what it derives for
// the device (engine_walk.cpp) and drops everything when tip states change.
class RepeatIndex {
public:
    struct Clade {
        int a = -1, b = -1;              // children: a tip (< tipCount: its buffer) or a clade (tipCount + index)
        int D = 0;
        bool built = false, over = false;    // over: more classes than the limit (or a child that is) — no index
        std::vector<std::uint16_t> cls;      // [P]
        std::vector<int> rep;                // [D]: the smallest pattern of each class; classes are numbered by it
        std::vector<int> tips;               // the clade's tips, left to right
    };
    void init(int tipCount, int patterns, int maxClasses);
    void clear();                                    // forget every clade (the tips' states stay registered)
    // Nothing is forgotten clade by clade (ids are what tables and kept programs name), and every list a topology move makes adds the
    // clades on two paths to the root — so the index has a CAPACITY: past it the owner drops everything (clear(), and what it derived)
    // and the live clades come back with the next list.  8 clades per tip + 1024: a tree's worth many times over.
    std::size_t capacity() const { return capacity_; }
    void setCapacity(std::size_t n) { capacity_ = n; }
    bool overCapacity() const { return clades_.size() > capacity_; }
    std::size_t bytes() const;                       // host memory of the indices kept
    void setTip(int tip, const std::uint8_t* states) { if (tip >= 0 && tip < tipCount_) tip_[(std::size_t)tip] = states; }   // [P] state codes (kept by the caller); nullptr: none
    int intern(int a, int b);                        // the clade over these two children (order does not matter), made on first sight
    int find(int a, int b) const;                    // ... or -1
    // index of clade `id`, children first; false: it has none.  budget: at most *budget clades are indexed by this call (counted down;
    // false with clade(id).built still false: call again)
    bool build(int id, int* budget = nullptr);
    const Clade& clade(int id) const { return clades_[(std::size_t)(id - tipCount_)]; }
    bool isTip(int id) const { return id < tipCount_; }
    int tipCount() const { return tipCount_; }
    int patterns() const { return P_; }
    int maxClasses() const { return maxClasses_; }
    std::size_t size() const { return clades_.size(); }
    long builds = 0;                                 // clades indexed so far (tests count them)
private:
    int tipCount_ = 0, P_ = 0, maxClasses_ = 0;
    std::size_t capacity_ = 1024;
    std::vector<const std::uint8_t*> tip_;
    std::vector<Clade> clades_;
    std::unordered_map<std::uint64_t, int> memo_;
    std::vector<int> table_;                         // build()'s scratch
};

// Where the class tables live: arenas laid out [C][P][4] like a partials buffer, back to back; a clade of D classes takes D rows padded to
// whole groups of 128 (a slice of the walk starts at a multiple of 128 patterns) inside ONE arena.  A bump allocator: tables are never
// freed one by one — when the arenas are full of clades no list names any more, everything is dropped and the live ones come back.
struct RepeatRows {
    int arenas = 0, P = 0, nextArena = 0, nextRow = 0;
    void init(int arenaCount, int patterns) { arenas = arenaCount; P = patterns; reset(); }
    void reset() { nextArena = 0; nextRow = 0; }
    bool place(int D, int& arena, int& row) {           // false: no room (or a clade that no arena can hold)
        const int pad = (D + 127) & ~127;
        if (D <= 0 || pad > P || nextArena >= arenas) return false;
        if (nextRow + pad > P) { if (nextArena + 1 >= arenas) return false; nextArena++; nextRow = 0; }
        arena = nextArena; row = nextRow; nextRow += pad;
        return true;
    }
};

// A run of Plan::runs that can be taken from a class table: every leaf a compact tip, nothing stored, nothing rescaled in write mode, no
// micro-operation of it pays reciprocals (`fold`: the plan's own FoldMap — its memberships are kept, the consumer pays what it paid; without
// one every read-mode micro-operation pays for itself and such a run stays), its consumer in the same slice.
// What is taken is a RANGE of the program, [start, start + count): a whole run, or — `sub` — a SUB-RUN, a maximal plain sub-clade inside a run
// that cannot be taken whole.  A memory definition evaluated from memory (a slice above the one that stored its operand, WalkPlanner::memStepCap)
// is ONE run with a PK_MEM leaf, yet most of its steps are the plain clades hanging off the path from that leaf to its last step: each of
// them is a contiguous post-order range that reads tips, ACC and hold slots written inside the range, stores nothing, pays nothing, and
// hands its result to a micro-operation of the same run — the next one through ACC, or a later one through the hold slot it is parked in —
// which is all a whole run is asked for.  Interned and limited by the class count as a whole run is.
struct RepeatRun { int start, count, clade, consumer; bool viaHold, sub; };
// the candidates of `plan`, in program order; a clade whose index is missing is built (`build`) or listed in `missing` and left out.
// subRuns false: whole runs only (WalkPlanner::memDefTables)
void findRepeatRuns(const Plan& plan, const FoldMap* fold, RepeatIndex& idx, bool build, std::vector<RepeatRun>& out, std::vector<int>* missing = nullptr,
                    bool subRuns = true);
// The plan with the runs of `take` evaluated once per class.  out.plan: the UPPER program — the source's slices in the source's order, with its
// dependencies, launch order and leaves, the runs gone and their consumers reading PK_TAB operands — and behind it in out.plan.prog the
// LOWER programs, one slice per run (out.lower; PlanSeg::partition = the clade): the run's own micro-operations, paying nothing, the last
// one's result to be stored as the clade's table.  origin[i]: the micro-operation of the source that out.plan.prog[i] came from.
// twoTables: consumers with both children from tables;  unstoredConsumers: consumers that are not stored themselves — steps of a memory
// definition evaluated behind its operand's program (planner.h memStepCap) or, with sub-runs, from memory: the only unstored micro-operations
// with a table as a child;  subRuns / subRunOps: the sub-runs among `take`, and the micro-operations they took out of the walk
struct RepeatPlan { Plan plan; std::vector<PlanSeg> lower; std::vector<int> origin; int tableReads = 0, twoTables = 0, unstoredConsumers = 0, subRuns = 0, subRunOps = 0; };
void emitRepeatPlan(const Plan& plan, const std::vector<RepeatRun>& take, RepeatPlan& out);

// Definition of a virtual buffer: one step per internal node of a small all-compact-tip subtree, in post-order (a step's
// sub-steps precede it; the last step is the buffer's own node).  An operand of a step is a compact tip or an earlier
// step; `need` = hold slots its evaluation takes (Sethi-Ullman: two internal operands -> the costlier one first, parked
// in a hold slot while the other one is evaluated), at most one less than the walk has, so that a parent can still park
// the definition's own result.
enum { VT_CHERRY = 1, VT_EXTEND = 2, VT_JOIN = 3 };
struct VirtStep {
    int type;               // VT_CHERRY: tipA, tipB;  VT_EXTEND: subA, tipB;  VT_JOIN: subA, subB
    int tipA, tipB;         // leaf buffers (or -1): compact tip states, or (memA / memB) partials the caller uploaded for a tip
    bool memA, memB;        // (no initialisers: a definition's unused steps are never looked at, and never copied — VirtDef below)
    int subA, subB;         // earlier steps of the same definition (or -1)
    int scaleIdx;           // this node's scale buffer, or PLAN_NONE
    int originA, originB;   // matrix slots the snapshots of operand A's / B's branch were last copied FROM
    int need;               // hold slots the evaluation of this step takes
};
// (1.5 KB with all 32 steps; a list of 1000 operations makes, keeps and copies a thousand of them, most of one to three steps:
// copies take the steps in use only — the planner's time on a list it has not seen: 87 -> 52 us with that, profiles/r05_experiments.txt 12)
struct VirtDef {
    bool on = false;
    bool chainOnly = true;  // evaluates without a hold slot (need of the last step == 0)
    int nSteps = 0;
    int stamp = -1;         // planner stamp of the list that created or last re-confirmed it
    // the op that defined it, for the steady-state path (an MCMC chain re-issues the same op on the same buffers every
    // other evaluation): a definition whose op and children are unchanged is re-confirmed, not rebuilt
    int version = 0;
    int sigC1 = -1, sigM1 = -1, sigC2 = -1, sigM2 = -1, sigScale = -2;
    bool sigTip1 = false, sigTip2 = false, sigMem1 = false, sigMem2 = false, fresh1 = false, fresh2 = false;   // sigTip: the child is a leaf
    int childVer1 = -1, childVer2 = -1;
    long cacheTag = 0;      // plan-cache entry that last wrote or confirmed this definition (0: none) — see WalkPlanner::replay
    // a MEMORY definition (WalkPlanner::memStepCap): one leaf of it is a stored INTERNAL node — memKey, read as partials in step memStep
    // (tipA with memA of a VT_CHERRY, tipB with memB of a VT_EXTEND) — instead of a tip; -1: every leaf is a tip
    int memKey = -1, memStep = -1;
    VirtStep steps[PLAN_MAX_STEPS];      // (copies take steps[0 .. nSteps) only)
    VirtDef() {}
    VirtDef(const VirtDef& o) { copyFrom(o); }
    VirtDef& operator=(const VirtDef& o) { if (this != &o) copyFrom(o); return *this; }
private:
    void copyFrom(const VirtDef& o);
};

inline void VirtDef::copyFrom(const VirtDef& o) {
    on = o.on; chainOnly = o.chainOnly; nSteps = o.nSteps; stamp = o.stamp; version = o.version;
    sigC1 = o.sigC1; sigM1 = o.sigM1; sigC2 = o.sigC2; sigM2 = o.sigM2; sigScale = o.sigScale;
    sigTip1 = o.sigTip1; sigTip2 = o.sigTip2; sigMem1 = o.sigMem1; sigMem2 = o.sigMem2; fresh1 = o.fresh1; fresh2 = o.fresh2;
    childVer1 = o.childVer1; childVer2 = o.childVer2; cacheTag = o.cacheTag; memKey = o.memKey; memStep = o.memStep;
    for (int s = 0; s < o.nSteps; s++) steps[s] = o.steps[s];
}

class WalkPlanner {
public:
    // holdSlots: per-thread slots a value can wait in while its sibling's subtree is evaluated (2 or 3; kernels.h)
    void init(int partialsCount, int tipCount, int matrixCount, int scaleCount, int maxVirtSteps, bool virtualEnabled, int holdSlots = 2);

    // maintained by the engine through setCompactTip: buffer holds compact tip states (index < tipCount and setTipStates was
    // the last setter).  compactEpoch counts the changes (a cached plan is only valid for the flags it was made with).
    std::vector<char> compactTip;
    long compactEpoch = 0;
    void setCompactTip(int buf, bool on) { const char v = on ? 1 : 0; if (compactTip[buf] != v) { compactTip[buf] = v; compactEpoch++; } }
    // ... or holds PARTIALS the caller uploaded for a tip (setTipPartials / setPartials on a tip index: ambiguity codes as
    // partials, sequence-error models — BeagleTreeLikelihood.java:497-509): data no operation computes, so a definition may
    // read it as a leaf too (32 C bytes per pattern from memory instead of a state byte)
    std::vector<char> leafPartials;
    void setLeafPartials(int buf, bool on) { const char v = on ? 1 : 0; if (leafPartials[buf] != v) { leafPartials[buf] = v; compactEpoch++; } }

    // A definition belongs to a (buffer, partition) pair — a partitioned instance updates the pattern ranges of one buffer
    // independently (MultiPartitionDataLikelihoodDelegate.java:972-997: every partition flips its own buffer indices) — and
    // is identified by its KEY = buffer * partitionCount + partition; with one partition the key is the buffer index.
    void setPartitionCount(int parts);       // forgets every definition (the engine materialises them first)
    int partitionCount() const { return keyParts_; }
    int key(int buf, int part) const { return buf * keyParts_ + part; }
    int bufferOf(int key) const { return key / keyParts_; }
    int partitionOf(int key) const { return key % keyParts_; }
    bool isVirtualKey(int key) const { return virt_[key].on; }
    bool isVirtual(int buf) const { for (int k = 0; k < keyParts_; k++) if (virt_[key(buf, k)].on) return true; return false; }
    void keysOf(int buf, std::vector<int>& out) const { for (int k = 0; k < keyParts_; k++) if (virt_[key(buf, k)].on) out.push_back(key(buf, k)); }
    const VirtDef& definition(int key) const { return virt_[key]; }
    bool virtualEnabled() const { return enabled_; }
    int snapSlot(int key, int step, int which) const { return matrixCount_ + key * 2 * maxSteps_ + 2 * step + which; }
    int matrixSlots() const { return matrixCount_ + (enabled_ ? partialsCount_ * keyParts_ * 2 * maxSteps_ : 0); }

    const std::vector<int>& tipUsers(int tip) const { return tipUsers_[tip]; }       // KEYS of the definitions that read this tip
    const std::vector<int>& scaleUsers(int idx) const { return scaleUsers_[idx]; }   // ... this scale buffer
    void clearVirtualKey(int key);       // forget the definition (that range of the buffer is about to get real data)
    void clearVirtual(int buf) { for (int k = 0; k < keyParts_; k++) clearVirtualKey(key(buf, k)); }
    // Define `buf` as the cherry node(tipA over matrix mA, tipB over matrix mB) [read-mode scale buffer scaleIdx or PLAN_NONE]
    // (the level-scheduled T32 path, engine_levels.cpp runOperationsLevels: one partition); appends the matrix snapshot copies to snapPairs.
    bool defineCherry(int buf, int tipA, int mA, int tipB, int mB, int scaleIdx, std::vector<int>& snapPairs);

    // Length of the longest prefix of ops[begin..count) that can run as one walk: no buffer (or scale buffer) is written
    // twice, written after an earlier op of the prefix read it, or read through a scale index another op writes.
    int hazardFreePrefix(const int* ops, int begin, int count, int tuple, int partitionCount);

    // Definitions (KEYS) that must get real data before this (hazard-free) list runs: those that read a scale buffer the list
    // rewrites (unless the list redefines them anyway), and a virtual destination that is its own child.
    void mustMaterializeBefore(const int* ops, int count, int tuple, std::vector<int>& out);

    // Memory definitions of more than `minSteps` steps that this (hazard-free) list reads as a child of one of its operations without
    // writing them or their stored operand: every evaluation of such a list would walk the whole definition, full width, where a stored
    // node costs one read — the engine gives them real data once instead (engine_internal.h memDefInlineSteps).  Appends KEYS to `out`.
    void longMemoryOperands(const int* ops, int count, int tuple, int minSteps, std::vector<int>& out);

    // Plan a hazard-free list.  Indices must have been range-checked by the caller; partitionCount must be the planner's.
    // `allowVirtual`: destinations may become virtual.  Returns 0, or a BEAGLE error code.
    // `chunkOps` > 0 (few pattern groups, so a launch cannot fill the chip with one walk per group): the forest is cut
    // into independent subtrees of about that many micro-operations, run side by side, wave after wave.
    int plan(const int* ops, int count, int tuple, int partitionCount, bool allowVirtual, Plan& out, int chunkOps = 0);

    // The steady state of a chain: the SAME closed list as one planned before (byte for byte, same compact-tip flags).  Returns
    // true and leaves the planner as plan() would — `planned` is the kept program — after one memcmp and one tag comparison per
    // operation.  `simple` (out): the list has no rescaling operation, no in-place update and no tip as a destination, so
    // nothing has to be materialised before it and nothing accumulated after it: the engine may skip its per-operation
    // checks too (they passed when the entry was made).  With `simple` given, a list that is not simple is left alone (false).
    bool replayCached(const int* ops, int count, int tuple, int partitionCount, bool allowVirtual, int chunkOps, bool* simple);

    // Program that gives every definition of `keys` its real partials (one slice per partition); the definitions are dropped.
    void planMaterialize(const std::vector<int>& keys, Plan& out);

    // statistics of the last plan() (bench / tests)
    int lastStored = 0, lastMemReads = 0, lastHolds = 0, lastWaves = 0;
    // chunkTopOps > 0: every wave above the first peels subtrees of at most this many micro-operations (the engine sets it once,
    // when ALL slices of a program run in one launch and a wave is not a launch: near the root few subtrees are left side by
    // side, so long slices there are a long serial tail on a few CUs; short ones keep more of them in flight)
    int chunkTopOps = 0;
    // How many slices the chip runs side by side (workgroup slots / pattern groups of a slice; the engine sets it): linkSlices
    // orders a one-launch program by simulating a greedy critical-path schedule on that many machines, so that a slice is
    // dispatched about when the slices it waits for are done — dispatched earlier it would only hold its workgroup slots
    // while it polls.  <= 0: plain descending-tail order.
    double launchMachines = 0.0;
    // stepLimit > 0: definitions made by the next plan() hold at most this many steps (a gradient chain: the pre-order walk
    // re-evaluates an unstored operand from its tips every time it meets it, kernels_preorder4.hip — tip-tip nodes and a tip-tip node
    // under one more tip, nothing longer); part of a cached plan's identity.  The snapshot slots keep the instance's own spacing.
    int stepLimit = 0;
    int stepCap() const { return stepLimit > 0 && stepLimit < maxSteps_ ? stepLimit : maxSteps_; }
    // memStepCap > 0: MEMORY definitions.  A node over ONE stored internal node A and a tip or a plain definition — or over a memory
    // definition and a tip or a plain definition: the chain goes on upwards — is defined, not stored, while the definition has at most
    // this many steps (<= stepCap()) and its evaluation fits the hold slots.  A stands in the definition as a leaf read from memory
    // (VirtStep::memA / memB, VirtDef::memKey), so tipUsers(A) lists the definitions that read it and whoever overwrites A — an
    // operation list (mustMaterializeBefore), an upload — gives them real data first.  A program that produces A itself evaluates the
    // definition BEHIND A, taking A from ACC or a hold slot as a stored parent would (emitReal: path frames); only a program that does
    // not produce A — a branch move passing the node as a sibling, a materialisation, a slice above the one that stored A — reads A.
    // One partition, no step limit, a walk with hold slots; a definition that nothing in its list consumes is stored after all (a root).
    // Part of a cached plan's identity.  0 (the default): off.
    int memStepCap = 0;
    // memStepCapSeen > memStepCap: the cap of a closed list that comes a SECOND time.  A list is planned with memStepCap when it is first
    // seen — partial updates, which are planned every time, and the full evaluation behind an accepted topology or branch move, whose list is
    // new, among them: long definitions make the branch moves behind them walk their steps —; when the same closed list comes again (a chain
    // of model moves alternates between two of them) its cache entry is dropped and the list planned once more under this cap, and that is
    // the program every later evaluation of the list replays.  0: memStepCap for every list.
    int memStepCapSeen = 0;
    // ... and a NEW closed list is planned under the longer cap at once while the caller says that full evaluations are all it has been
    // asked for lately (the engine: the last two lists were closed ones, of any kind — a chain of model moves whose scale buffers have just
    // flipped meets new lists too, and the write-mode list of the flip is one of the two)
    bool preferSeenCap = false;
    int memCapSeen() const { return memStepCapSeen > memStepCap && memStepCap > 0 ? memStepCapSeen : memStepCap; }
    // repeatWeights: the engine will take this list's plain definitions — every leaf a compact tip — from class tables (RepeatIndex,
    // emitRepeatPlan), so pass 2 weighs such a definition as what it leaves in the walk, ONE gather on its consumer, not as its steps, and
    // linkSlices' schedule simulation takes a slice's duration the same way (PlanSeg::tail stays in program micro-operations).  Acts on
    // closed lists of one partition without a rescaling operation — what the engine compresses; any other list is planned as without it.
    // Part of a cached plan's identity.  lastWeighed: such a plan's weight in all, 0: the last plan() was not weighed this way.
    bool repeatWeights = false;
    long lastWeighed = 0;
    // memDefTables: ... and the plain clades INSIDE its memory definitions too (planner.h RepeatRun: sub-runs), so under repeatWeights a memory
    // definition weighs what it leaves in the walk as well: the steps on the path from its stored operand to its last step plus ONE per plain
    // clade hanging off that path — whether it is evaluated from memory or behind its operand's program, where those clades are runs of their
    // own.  With all of its steps counted, a list planned under the longer cap was peeled into two to three times the slices and waves of the
    // same list under the shorter one (profiles/memdef_tables.txt).  Part of a cached plan's identity.  false: whole runs only, a memory
    // definition weighs its steps.
    bool memDefTables = true;
    // ... and the slice sizes of such a plan, chosen from its weight once pass 2 knows it (the engine's rule, engine_walk.cpp
    // walkRepeatChunkOps): chunk and top arrive as plan()'s chunkOps and chunkTopOps and leave as what the plan is cut with.  None: as they are.
    std::function<void(long weight, int& chunk, int& top)> repeatChunkRule;
    long cacheHits = 0;                  // plans served from the cache below
    long replayInPlace = 0;              // definitions a replay took over from another entry with their leaves unchanged (user lists edited in place)
    bool cacheEnabled = true;            // false: no plan is replayed — a closed list is planned from scratch every time, under the cap its kept plan had, and is kept (a tag) all the same
    // what the last plan() produced: `out`, or the cache's copy (no copy is made on a hit).  plannedTag identifies the
    // cache entry (0: not cached) so that the engine can keep what it derives from the plan.
    const Plan* planned = nullptr;
    long plannedTag = 0;

private:
    // a child of an operation: its buffer and branch matrix, the op of this list that produced it (or -1);  tip: compact states;
    // leaf: that, or uploaded tip partials
    struct Operand { int buf, mat, prod; bool tip, leaf; };
    struct OpInfo {
        int dest, wS, rS, part;
        Operand ch[2];
        bool virtDest;
        int need;           // hold slots the evaluation needs (-1: not computed yet)
        int size;           // real micro-ops below (ordering heuristic)
        bool emitted;
    };
    bool buildVirtual(int X, int c1, bool leaf1, bool mem1, int m1, int c2, bool leaf2, bool mem2, int m2, int scaleIdx, std::vector<int>& snapPairs,
                      bool stored1 = false, bool stored2 = false);   // X, and a non-leaf child: KEYS;  stored: the leaf is a stored internal node (memStepCap)
    void registerVirtual(int X);
    // emission
    void emitReal(int root, unsigned freeMask, Plan& out);
    void emitVirtualStep(int buf, int idx, unsigned freeMask, bool writeMode, Plan& out);
    void emitVirtual(int buf, unsigned freeMask, bool writeMode, Plan& out);
    bool memDefsOn(int parts) const { return memStepCap > 0 && parts == 1 && stepLimit == 0 && allSlots_ != 0u; }
    int operandOp(int vkey) const;       // the real op of the list being planned that produces the definition's stored operand, or -1
    int pathNeed(const VirtDef& v, int upTo, int needA) const;       // hold slots of steps memStep .. upTo evaluated behind the operand's own program
    bool onPath(const VirtDef& v, int idx) const;                    // is step memStep in the subtree of step idx
    void realInfo(int k);                // OpInfo::need / size of the (real) op k
    int virtNeed(int buf) const { return virt_[buf].nSteps ? virt_[buf].steps[virt_[buf].nSteps - 1].need : 0; }
    void linkSlices(Plan& out, int repeatDurations = 0);           // PlanSeg::dep*, tail and Plan::launchOrder (1: whole plain runs count as one gather, 2: sub-runs too)
    void linkDependencies(Plan& out);                              // ... its first step: PlanSeg::depStart / depCount and Plan::deps
    bool plainDefinition(const VirtDef& v) const;                  // every leaf a compact tip: what a class table can stand for (repeatWeights)
    int memDefWeight(const VirtDef& v) const;                      // a memory definition's path steps + one per plain clade off the path (memDefTables)
    std::size_t scaleKey(int idx, int part) const { return (std::size_t)idx * parts_ + part; }      // key()'s counterpart for the per-partition marks of a scale buffer
    std::vector<int> storedBy_, storedStamp_;          // per (buffer, partition): the slice of the current plan that stores it
    int linkStamp_ = 0;
    int memCapNow_ = 0;                                // the cap of the list being planned (memStepCap, or memCapSeen())

    int partialsCount_ = 0, tipCount_ = 0, matrixCount_ = 0, scaleCount_ = 0, maxSteps_ = 6, keyParts_ = 1;
    bool enabled_ = false;
    std::vector<VirtDef> virt_;
    std::vector<int> pairScratch_;                     // buildVirtual's snapshot pairs before they are known to be wanted
    std::vector<long> tagOf_;                          // per key: -1 not virtual, 0 virtual, > 0 virtual and written by that cache entry
    long tagEpoch_ = 0;                                // counts the writes to tagOf_: an entry replayed at this count and asked for again at
                                                       // the same count finds every key as it left it (CacheEntry::cleanAtEpoch) — the chain's
                                                       // steady state, two lists alternating, costs no pass over the list at all
                                                       // (a compact mirror of on / cacheTag: replaying a plan touches 8 bytes per op)
    std::vector<std::vector<int>> tipUsers_, scaleUsers_;
    int virtVersion_ = 0;
    int stamp_ = 0;
    // per-list scratch (stamped, so nothing is cleared between calls)
    std::vector<int> wStamp_, rStamp_, wOp_;          // per (buffer, partition)
    std::vector<int> sWStamp_, sRStamp_, sDone_;      // per scale buffer: written / read in this list, write emitted
    std::vector<OpInfo> info_;
    unsigned allSlots_ = 3u;                           // mask of the hold slots
    int parts_ = 1;

    // Plans of CLOSED lists (every child is a compact tip or the destination of an earlier operation of the same list:
    // a full evaluation, what BEAST issues whenever a model parameter changes — MarkovChain.java:207-263 with all nodes
    // dirty) depend on nothing but the list itself and the tips' compact flags, so they are kept and replayed: the chain
    // alternates between two such lists (BufferIndexHelper.java:71-106).  Partial updates are planned every time.
    struct CacheEntry {
        bool valid = false;
        long tag = 0;
        int count = 0, tuple = 0, parts = 0, chunkOps = 0, stepLimit = 0, memStepCap = 0;
        bool allowVirtual = false, repeatWeights = false, memDefTables = true;
        std::vector<int> ops;
        long tipEpoch = -1;                            // compactEpoch the plan was made under
        bool simple = false;                           // see replayCached
        Plan plan;
        std::vector<VirtDef> defs;                     // per op: the definition its destination ends up with (on = false: real)
        std::vector<char> defOn;                       // defs[k].on
        int stored = 0, memReads = 0, holds = 0, waves = 0;
        long weighed = 0;
        mutable long cleanAtEpoch = -1;                // tagEpoch_ right after the last replay of this entry (-1: never replayed since it was filled)
    };
    // (8: a chain under DYNAMIC rescaling cycles through 2 buffer-flip states x 2 scale-buffer sets of its read-mode list and the
    // same four of the list that recomputes the factors every 100th evaluation — with 4 ways every such evaluation evicted a
    // read-mode entry and the next evaluations planned, resolved and uploaded from scratch: 1.4 ms each on the 12 500-pattern shard)
    static constexpr int CACHE_WAYS = 8;
    CacheEntry cache_[CACHE_WAYS];
    int cacheNext_ = 0;
    long wayGen_[CACHE_WAYS] = {0, 0, 0, 0, 0, 0, 0, 0};      // fills of each way (a plan's tag: plan())
    void replay(const CacheEntry& e, const int* ops);
    bool promotable(const CacheEntry& e, bool allowVirtual) const;
    CacheEntry* findCached(const int* ops, int count, int tuple, int parts, bool allowVirtual, int chunkOps);

    // What the steps of one plan() call hand each other (planner.cpp: "plan(): the steps"; each step's contract says which of these it
    // reads and leaves behind).  A member for the vectors' capacity only: nothing in it outlives the call.
    struct ListState {
        const int* ops = nullptr;                      // plan()'s arguments
        int count = 0, tuple = 0, parts = 1, chunkOps = 0;
        bool allowVirtual = false;
        Plan* out = nullptr;
        CacheEntry* fill = nullptr;                    // cache step: the entry a closed list's plan goes into (nullptr: not kept)
        bool anyRescale = false, simple = false;       // cache step: the list has a write-mode operation;  CacheEntry::simple
        bool memDefs = false, anyMem = false;          // pass 1: memory definitions may be made;  one was made
        std::vector<char> consumed;                    // pass 1, settlement: per op, its result is evaluated inside another op's program
        std::vector<int> partsSeen;                    // the partitions the list names, in the order it names them
        bool repeatW = false, ruled = true;            // pass 2: weigh for compression (planner.h repeatWeights);  the slice sizes are final
        int cutOps = 0, cutTop = 0;                    // pass 2: what the plan is cut with (chunkOps / chunkTopOps, or repeatChunkRule's)
        std::vector<int> weight, chunkRoots, stack;    // pass 2: per op, the micro-operations below it that are still to be emitted;  scratch
    };
    ListState list_;
    bool cacheStep(ListState& L);
    void definePass(ListState& L);
    void defineOp(ListState& L, int k);
    bool definitionStands(const VirtDef& ev, const OpInfo& o, int ownScale, const bool stored[2]) const;
    void signDefinition(VirtDef& nv, const OpInfo& o, int ownScale, const bool stored[2]);
    void settleMemoryConsumers(ListState& L);
    void listPartitions(ListState& L);
    int emitPartition(ListState& L, int part);
    long weighPartition(ListState& L, int part);
    bool peelWave(ListState& L, int part, int chunk, int wave);
    bool emitRemainder(ListState& L, int part, int wave);
    void fillCache(ListState& L);
};

}  // namespace mi355
