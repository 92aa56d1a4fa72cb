// engine_internal.h — what the engine's translation units share: the instance record and its staging / allocation helpers
// (engine_instance.cpp), the 4-state walk runner (engine_walk.cpp), the level scheduler for every other state count
// (engine_levels.cpp), the pre-order / gradient paths (engine_preorder.cpp).  The C ABI of include/beagle_mi355.h is spread over
//   engine_create.cpp    instance creation, the -beagle_auto self-benchmark
//   engine_abi.cpp       everything a caller SETS or ENQUEUES: patterns, tips, partials, model arrays, transition matrices,
//                        updatePartials, scale factors, the pre-order entry points; the two Beagle*Api tables
//   engine_root.cpp      the calls that observe a likelihood: root sums, the polled result page, site log-likelihoods
//   engine_readback.cpp  partials and scale factors back to the host
//   engine_sampling.cpp  the device samplers (ancestral draws, Markov jumps, uniformized histories)
//   engine_simulate.cpp  sequence simulation down the tree from the branch matrices
//   engine_robustcounts.cpp  codon robust counts over three instances' draws, unconditioned count simulation
//   engine_history.cpp   complete substitution histories simulated down the tree from the generators
//   engine_nodeheight.cpp  node-height gradients and diagonal Hessians in one call
//   engine_tipemission.cpp  tip error models: emission tables folded into the tip branch matrices
//   engine_differential.cpp  substitution-parameter differential matrices of every branch in one call
//   engine_eigen.cpp     eigen systems of reversible models decomposed on the device in one call, an eigen slot back to the host
//   engine_generator.cpp transition matrices straight from generators in one call, no eigen system
//   engine_epoch.cpp     branch matrices of epoch models (products of per-segment transition matrices) in one call
//   engine_nodepattern.cpp  the stochastic Dollo node-pattern likelihood over a post-order node list in one call
//   engine_nodeposterior.cpp  marginal node state posteriors from resident pre- and post-order partials in one call
//   engine_placement.cpp  scores of attaching new sequences at candidate points of the tree in one call
//   engine_regraft.cpp    scores of hanging a pruned subtree at candidate points of the tree it was cut from in one call
//   engine_stats.cpp     stream, synchronisation, kernel timer, counters
// each of them argument checks, buffer bookkeeping and one call into the files above.
// All arithmetic is in the .hip files; these files validate indices, resolve buffer indices to device pointers and enqueue
// kernels on the instance's HIP stream.  Results are only observed at calculateRootLogLikelihoods / get*, so every other
// call returns as soon as its work is enqueued (SURVEY 8b "Threading").
//
// Device memory: every allocation of an instance goes through devAlloc onto Instance::allocations — the partials / scale / tip-state
// slabs, the model arrays and matrix blocks, the staging ring's mirror, fold vectors, the repeat arena and pool, BASTA's arrays, tip
// emission tables and codes, and every grow-on-demand DevBuf (samplers, edge scratch, cherry tables, pre-order program, fold range
// check, matrix stream, walk flags, slice sums, kept programs, export buffers).  destroy() frees that list.  Not on it: pinned host
// memory, events, streams, and the per-call ScopedDevice temporaries.
//
// There is no CPU path in this library: with no visible MI355X beagleCreateInstance returns BEAGLE_ERROR_NO_RESOURCE.
#pragma once
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>
#include <chrono>
#include <atomic>
#include <unordered_map>
#include "../../include/beagle_mi355.h"
#include "kernels.h"
#include "planner.h"
#include "scratch_layout.h"
#include "sharded.h"

namespace mi355 {
namespace eng {


#define HIP_TRY(expr)                                                                         \
    do {                                                                                      \
        hipError_t e__ = (expr);                                                              \
        if (e__ != hipSuccess) {                                                              \
            if (getenv("BEAGLE_MI355_DEBUG"))                                                 \
                fprintf(stderr, "[beagle-mi355] %s failed: %s (%s:%d)\n", #expr, hipGetErrorString(e__), __FILE__, __LINE__); \
            return e__ == hipErrorOutOfMemory ? BEAGLE_ERROR_OUT_OF_MEMORY : BEAGLE_ERROR_GENERAL; \
        }                                                                                     \
    } while (0)

constexpr size_t RING_BYTES = 16u << 20;   // pinned host staging ring + its device mirror
constexpr int SLAB_BUFFERS = 32;           // partials buffers per hipMalloc
constexpr int PRE_SCRATCH = 32;            // pre-order ops per two-pass chunk on the T32 layout
constexpr int GRADIENT_VIRT_STEPS = 2;     // longest definition a gradient chain can leave unstored (Instance::gradientVirtual)
constexpr int MEM_DEF_STEPS = 8;           // longest definition over a stored internal node (planner.h memStepCap; engine_create.cpp)
constexpr int MEM_DEF_SEEN_STEPS = 24;     // ... in the plan of a closed list that has come a second time (planner.h memStepCapSeen)
constexpr int MEM_DEF_INLINE_STEPS = 8;    // ... and the longest one a list that only READS it evaluates inside its own program (Instance::memDefInlineSteps)
constexpr int GRADIENT_VIRT_DEFAULT = 1;   // ... and what it does leave unstored by default: nodes over two tips (engine_create.cpp)

struct Basta;                              // engine_basta.cpp
struct TipEmissions;                       // engine_tipemission.cpp

// A device buffer an instance owns and grows on demand (growDevice / releaseDevice below).  Its block is on Instance::allocations like
// every other device allocation, so destroy() frees it without knowing the field.
struct DevBuf {
    char* p = nullptr; size_t bytes = 0;
    bool counted = true;                                 // its bytes are part of Instance::deviceBytes (beagleMi355DeviceBytes)
    template <class T> T* as() const { return reinterpret_cast<T*>(p); }
};
// KNOWN DEFECT, kept on purpose: the buffers declared with this type were never added to deviceBytes (matStream, bigStage, walkFlags,
// sliceMant / sliceExp, Resolved::dProg, exportDev), so beagleMi355DeviceBytes under-counts what a walk instance holds.  The figure is
// a benchmark output and a test's reference; counting them is a change of behaviour and belongs to a pull request of its own.
struct DevBufUncounted : DevBuf { DevBufUncounted() { counted = false; } };
// what growing does with the block it replaces
enum class Grow {
    SyncAndFree,                                         // drain the instance's stream (on the first allocation too), free the old block, allocate
    SyncIfHeld,                                          // the same, but a buffer that holds nothing yet is allocated without draining
    KeepOld                                              // no synchronisation: work in flight may still read the old block, which stays on the
};                                                       // allocation list until the instance is destroyed; the field points at the new one

struct Instance {
    int device = 0;
    // 4 states: every operation list runs as ONE launch of the pattern-walk kernel (kernels_walk4.hip), programmed by the
    // walk planner (planner.h), which also owns the definitions of virtual buffers
    bool walk = false;
    mi355::WalkPlanner planner;
    mi355::Plan plan;                                    // scratch of the current call
    size_t scaleStride = 0;                              // walk instances: a scale buffer is [factors | reciprocals (pair-interleaved,
                                                         // kernels.h walkPairIndex)], this many doubles apart
    size_t statePairOff = 0;                             // walk instances: a tip's pair-interleaved states follow its plain ones, this many bytes on
    // walk instances: position of pattern p in the pair-interleaved arrays (tip states, reciprocal scale factors).  They are
    // laid out partition by partition, each padded to whole blocks of 128 patterns (kernels.h WalkSeg), so that the assembly
    // loop runs whatever the caller's partition boundaries are; one partition: walkPairIndex(p).
    std::vector<unsigned> pairPos; size_t pairLen = 0; std::vector<int> padStart; unsigned* dPairPos = nullptr;
    DevBufUncounted matStream;                              // walk instances: the matrix stream of the program being run (k_gatherMatrices)
    uint8_t* dummyTips = nullptr; double* onesScale = nullptr;   // walk instances: all-missing states / all-one factors for the operands a
                                                                 // micro-operation does not use (the assembly loop loads them unconditionally)
    long statFastWalks = 0;
    // what a walk program stands for in the instance's counters (resetWalkCounters): added once per run, resolved or reused
    struct WalkTraffic {
        long memReads = 0, tipReads = 0, scaleReads = 0, scaleWrites = 0, stored = 0, fused = 0;      // (fused: cherries, kernels.h WK_CHERRY)
        long microOps = 0;                               // of the walk proper (class-table programs: tableRows)
        long tableRows = 0, tableReads = 0, repeatClades = 0, twoTables = 0, unstoredConsumers = 0;   // repeated sub-patterns (below)
        long subRuns = 0, subRunOps = 0;                  // ... of them the plain clades inside runs not taken whole (planner.h RepeatRun::sub), their micro-operations
        // ... as the device program has them (ProgramResolver::microOp; beagleMi355TableOperandStats): first children read from tables, those
        // directly behind a micro-operation whose first child comes from memory / that has a fused cherry, the most classes of a table read
        long tabFirst = 0, tabFirstBehindMem = 0, tabFirstBehindCherry = 0, tabMaxClasses = 0;
    };
    // a plan resolved to device addresses (engine_walk.cpp resolveProgram).  A cached plan's (planner.h plannedTag) is kept in one of
    // `resolved`; any other resolves into `scratch`, which is never reused and keeps nothing on the device.
    struct Resolved {
        bool kept = false;                               // one of `resolved`: dProg, folds, repeats and noFoldTag apply to kept programs only
        long tag = 0, epoch = -1;                        // the plan and the resolveEpoch it was resolved under (scratch: tag stays 0)
        std::vector<mi355::WalkOp> w; std::vector<mi355::WalkSeg> segs; std::vector<int> deps;      // deps: per device slice the device slices it waits for
        // how the program is launched, decided when it is resolved (launchWalk / launchWaves)
        bool oneLaunch = false;                          // every slice in ONE launch of the assembly loop, in `order`
        std::vector<int> order;                          // oneLaunch: device slice -> slice of the plan in use (critical path first; on tickets the leaves first)
        int leaves = 0;                                  // > 0: the device program is laid out for a launch on tickets — its first `leaves` slices wait for nothing
        int maxRange = 0, sinks = 0;                     // widest pattern range of a slice; slices no other slice waits for — one: the whole program leads to its last slice
        std::vector<int> finalStore, finalPart, sinkRows;   // oneLaunch, per device slice: what PendingWalk carries of them when the launch is held back
        std::vector<int> sumRows, wroteScale;            // write-mode programs: the device slices that leave their product of factors behind, the scale buffers the program writes (Instance::lastSums)
        std::vector<const double*> cm;                   // fused cherries (kernels.h WK_CHERRY): per device micro-operation the cherry's two branch matrices (empty: none fused)
        WalkTraffic traffic;                             // (traffic.scaleWrites > 0: a run of it writes per-node scale buffers — folds built from them are stale then)
        DevBufUncounted dProg; bool dProgValid = false;    // the packed program (engine_walk.cpp PackedProgram), resident on the device
        std::vector<int> folds;                          // folded reciprocal vectors the program reads (Instance::folds)
        long foldEpoch = -1;                             // scaleWriteEpoch those vectors were last checked against
        long noFoldTag = 0;                              // the plan whose folds left the safe range: resolved with per-node factors
        // repeated sub-patterns (below): the program was made from `repeats.plan` instead of the planner's own; its last `lower` slices are
        // the class-table programs, launched in front of the others
        bool compressed = false; mi355::RepeatPlan repeats; int lowerRange = 0;
        bool repeatsMissing = false;                     // a clade of it had no index yet: resolved again once the index is there
    } resolved[8], scratch;                              // (as many as the planner's cache has ways: planner.h CACHE_WAYS)
    // Read mode, 4 states: a node that is not stored is seen by nobody but its parent, and a partial is linear in each child — so
    // the reciprocal scale factors of the unstored nodes below a stored one are applied ONCE, at that node, as one vector: the
    // entry-wise product of their reciprocal halves (a "fold"; built by k_foldReciprocals whenever a scale buffer has been written
    // since — scaleWriteEpoch — and kept by member list).  A cached full-evaluation program then reads one scale vector per STORED
    // node instead of one per node (config A: 78 + slice roots instead of 999; 0.8 of the evaluation's 2.2 GB).  The per-node
    // buffers stay what getLogScaleFactors, accumulateScaleFactors, partial updates and the gradient pass expect.  A fold whose
    // largest product leaves [1, 1e100] is refused and its plan falls back to per-node factors.  BEAGLE_MI355_NO_SCALE_FOLD=1 at
    // creation switches folding off: every node is then rounded the same way on every evaluation path (bitwise-equal partial
    // updates and full evaluations); with folding the paths agree to rounding (1e-15 relative).
    struct FoldVec { std::vector<int> members; double* recip = nullptr; long builtEpoch = -1; bool bad = false; };
    std::vector<FoldVec> folds;
    std::vector<std::pair<size_t, int>> foldIndex;       // (hash of the member list, index into folds), sorted by hash
    std::vector<double*> foldFree;                       // vectors of a dropped cache generation, reused
    long scaleWriteEpoch = 0;                            // bumped by everything that writes (or re-lays) a per-node scale buffer
    bool foldScales = true;
    DevBuf foldWorst;                                    // device: k_foldReciprocals' range check, a word per fold of a launch
    long resolveEpoch = 0;                               // bumped when pattern ranges change
    // Repeated sub-patterns (planner.h RepeatIndex): in a cached read-mode full evaluation, a clade of compact tips that the
    // plan evaluates inside its consumer's program (a plain definition) and whose patterns fall into at most repeatMaxClasses classes is
    // evaluated ONCE PER CLASS — by an ordinary slice of the walk over the class representatives' tip states, stored as rows of a table
    // arena, in a launch of its own in front of the walk — and its consumer reads the pattern's row (kernels.h WK_TAB).  Every pattern
    // still goes through the arithmetic it went through, on the same matrices and the same folded reciprocals: bit for bit the
    // uncompressed program.  One partition, buffers of 2 MiB and more (BEAGLE_MI355_REPEATS_ANY_SIZE=1: any size), BEAGLE_MI355_NO_REPEATS=1: off,
    // BEAGLE_MI355_REPEAT_MAX_FRAC=<1/n>: the class limit as a fraction of the pattern count.
    bool repeatsOn = false; int repeatMaxClasses = 0;
    // repeatSlicing: lists that will be compressed are cut by what compression leaves of them (planner.h repeatWeights; engine_walk.cpp
    // walkRepeatChunkOps) — repeatsOn, the assembly loop, all slices in one launch on tickets; BEAGLE_MI355_NO_REPEAT_SLICING=1: the cut
    // of the uncompressed list.  repeatSlicingOff: a program cut this way had fewer than half of its definitions' micro-operations
    // compressed (an alignment whose clades exceed the class limit): later lists are cut as uncompressed ones, until new tip states.
    bool repeatSlicing = false, repeatSlicingOff = false;
    // memDefInlineSteps: a list that reads a memory definition of MORE steps than this without producing its stored operand — a branch move
    // passing the node as a sibling — gives it real data first, once (runOperationsWalk): every later move reads the node from memory, as
    // it reads a stored one, and the next full evaluation defines it again.  Shorter ones are evaluated inside the list's own program every
    // time, as they always were.  BEAGLE_MI355_MEM_DEF_INLINE_STEPS=n at creation (at or above the cap: never).
    int memDefInlineSteps = MEM_DEF_INLINE_STEPS;
    int closedListRun = 0;                               // closed lists of 16 operations and more (the planner keeps their plans: read mode or write mode)
                                                         // planned or replayed since the last list that was not one (planner.h preferSeenCap)
    mi355::RepeatIndex repeatIndex;
    std::vector<std::vector<uint8_t>> hostTips;          // per tip: the state codes as uploaded (what the index is built from)
    long tipDataEpoch = 0, repeatEpoch = -1, repeatCompactEpoch = -1;     // setTipStates calls; what the index and the tables were made under
    struct RepeatTable { int D = 0, arena = 0, row = 0; char* dev = nullptr; size_t bytes = 0, tipStride = 0; std::vector<int> tips; };   // dev: [row vector (uint16 class ids, kernels.h WK_TAB) | tip rows]
    std::unordered_map<int, RepeatTable> repeatTables;   // by clade
    // where the tables' row vectors and tip rows live: a few large device blocks handed out front to back (all of it is given up at
    // once, dropRepeatTables), filled by stream-ordered copies out of a pinned staging buffer — no allocation and no blocking copy per table
    struct RepeatBlock { char* dev = nullptr; size_t size = 0, used = 0; };
    std::vector<RepeatBlock> repeatPool;
    char* repeatStage = nullptr; size_t repeatStageSize = 0, repeatStageUsed = 0;
    double* repeatArena = nullptr; int repeatArenas = 0; mi355::RepeatRows repeatRows;      // [arenas][C][P][4]; who has which rows
    std::vector<int> repeatQueue;                        // clades waiting for their index (built where the host waits for a result)
    long statTableRows = 0, statTableReads = 0, statRepeatClades = 0, statTwoTables = 0, statUnstoredConsumers = 0;      // since the last timer reset
    long statSubRuns = 0, statSubRunOps = 0;                                                                             // (the same; beagleMi355RepeatSubRunStats)
    long statTabFirst = 0, statTabFirstBehindMem = 0, statTabFirstBehindCherry = 0, statTabMaxClasses = 0;               // (the same)
    size_t repeatTableCap = 0;                           // most tables kept (three times what the last compressed plan took): past it, as when the arena is full
    bool lastPlanCached = false;                         // the last runPlan ran a cached full-evaluation plan (the result wait behind it is long enough for index work)
    long statRepeatResets = 0;                           // times the indices were dropped at their capacity, since creation
    long statRepeatBuildUs = 0;                          // host time spent building indices and tables, since creation
    bool lowerLaunched = false;                          // the last runPlan launched class-table programs (a launch more for the kernel timer)
    bool fastWalk = true;                                // BEAGLE_MI355_NO_FAST_WALK=1 at creation: k_walk4 only (A/B runs, tests)
    // 4 states: a pre-order operation list is HELD BACK (engine_preorder.cpp): the chain that evaluates gradients wants the
    // edge-derivative sums that follow it, not the pre-order partials, and those sums can be had without writing a single
    // pre-order partial (kernels_preorder4.hip k_preWalk4).  The list stays held — as a closure over what it reads — until a
    // call reads something it writes or writes something it reads; then it runs first (GET_INSTANCE -> executeHeldPre).
    // Calls that provably do neither leave it alone (GET_INSTANCE_KEEP_PENDING + heldTouches* below), and a newer list that
    // rewrites everything it would have written replaces it unexecuted.
    struct HeldPreNode { int par, preA, preB, postA, postB, matA, matB, level, jobA, jobB, size; };
    struct HeldPreList {
        bool held = false;
        std::vector<int> ops;                            // as the caller wrote it
        std::vector<HeldPreNode> nodes;                  // one per parent: its two operations together
        std::vector<int> order;                          // depth-first, smaller subtree first (the walk's program order)
        std::vector<unsigned> walkFlags;                 // per entry of `order`: PW_* source / continuation bits
        std::vector<int> segStart, segRoot;              // the walk's segments: entries segStart[s] .. segStart[s + 1] of `order`, headed by job segRoot[s]
        int maxLevel = 0, holdSlots = 0, rootBuf = -1;
        std::vector<char> readsMatrix, readsBuf, writesBuf;   // by matrix / partials-buffer index
    } heldPre;
    double* preRootCopy = nullptr;                       // the held list's own copy of its root's pre-order partial
    uint8_t* preDummyStates = nullptr;                   // [P] "missing": what a descriptor's unused tip pointer points at
    DevBuf dPreProg;                                     // the walk's program on the device (grow-only)
    // which scale buffer a partials buffer's last operation divided it by (-1: none / unknown), and that buffer's version then: the
    // pre-order walk multiplies a step into an internal node by the reciprocal of exactly that factor (kernels_preorder4.hip) and
    // is refused when the scale buffer has been written since (beagleUpdatePartials, the scale-factor calls)
    // Kept only once a pre-order list has arrived (trackScales; everything written before that is "unknown", -2, and the first
    // gradient of a chain takes the path that forms every edge's denominator itself).
    std::vector<int> scaleOfPartial; std::vector<unsigned> scaleVersionAtWrite, scaleVersion;
    bool trackScales = false;
    long statFusedGradients = 0, statPreLists = 0, statWalkedGradients = 0, statLateLists = 0;
    int storeAllEvaluations = 0;                         // > 0: a gradient chain is running — its post-order passes store what the pre-order
                                                         // pass will read: every node, or (gradientVirtual) every node but the short
                                                         // definitions the pre-order walk re-evaluates from the tips itself
    // 4 states: a gradient chain's post-order passes keep definitions of up to GRADIENT_VIRT_STEPS steps (tip-tip nodes, and those
    // under one more tip — half the nodes of a coalescent tree) instead of storing every node, and k_preWalk4 re-evaluates them where
    // it needs them (engine_preorder.cpp walkableDefinition).  BEAGLE_MI355_GRADIENT_VIRTUAL at creation (engine_create.cpp): 0 = every
    // node stored, as in round 4; 1 = THE DEFAULT (GRADIENT_VIRT_DEFAULT): nodes over two tips stay unstored and are evaluated inside
    // their parents' descriptors (a third of the bytes of both passes: 6.1 -> 5.3-5.5 ms per gradient at 1e5 patterns); 2 = also such a
    // node under one more tip, by descriptors of their own (half the bytes, slower: a descriptor costs a stage whatever it computes).
    // (the initialisers below are overwritten at creation)
    bool gradientVirtual = false; int gradientVirtualSteps = GRADIENT_VIRT_STEPS;
    DevBuf edgeScratch;                                  // per-64-pattern derivative sums of the edges of one call (grow-only)
    bool preWalk = true;                                 // BEAGLE_MI355_NO_PRE_WALK=1 at creation: always write the pre-order partials
    bool fuseGradient = true;                            // BEAGLE_MI355_NO_FUSED_GRADIENT=1 at creation: operation by operation (A/B runs)
    // 16..20 states: operation lists without write-mode rescaling run as the walk's programs on the T32 layout (kernels_mfma.hip
    // k_walkT32: same planner, same descriptors; engine_walk.cpp); everything 4-state-specific (`walk`) stays off
    bool walkT = false;
    // ... and its write-mode form (k_walkT32W1: lists that rescale in write mode stay on the walk; at most four categories, two hold slots;
    // BEAGLE_MI355_NO_T32_WRITE_WALK=1: they run level by level, as until round 6)
    bool walkTWrite = false;
    // 4-state partitioned instances: the top slices of the partitions finish calculateRootLogLikelihoodsByPartition inside the walk's launch
    // (kernels.h RootFusedParts; BEAGLE_MI355_NO_ROOT_PARTS_FUSION=1: a launch of its own behind it, k_rootSite4WParts — the same bits)
    bool fuseRootParts = true;
    long statRootPartsFused = 0;                         // by-partition root calls that were finished inside the walk's launch
    // the tables the kernel reads and what each holds: a chain's evaluations alternate between a few (buffer flips: two programs, two
    // root slices), so four are kept and one is uploaded only when none of them matches
    static constexpr int ROOT_PARTS_TABLES = 4;
    mi355::RootFusedParts* rootPartsDev = nullptr;       // [ROOT_PARTS_TABLES]
    std::vector<char> rootPartsShadow[ROOT_PARTS_TABLES];
    int rootPartsNext = 0;
    bool fuseLaunches = true;                            // BEAGLE_MI355_NO_LAUNCH_FUSION=1: snapshot / gather and root site / final as separate launches (A/B runs)
    // A one-launch walk whose launch is held back until the next call: calculateRootLogLikelihoods on the result of one of its
    // slices launches it WITH that slice finishing the evaluation (no root kernel, no read-back of the root's partials); any other
    // call launches it as it is (live()).  Only full-range walks of unpartitioned instances outside a timer bracket are held.
    struct PendingWalk {
        bool valid = false;
        const mi355::WalkOp* prog = nullptr; const mi355::WalkSeg* segs = nullptr; const int* deps = nullptr;
        int nSegs = 0, range = 0, flagStride = 0; unsigned epoch = 0;
        int leaves = 0;                                  // > 0: launch on tickets, that many rows
        unsigned cherryOff = 0;                          // byte offset of the matrix stream's cherry region (0: the program has no fused cherries)
        std::vector<int> finalStore;                     // per device slice: the buffer its last micro-operation stores (-1: none)
        std::vector<int> finalPart;                      // ... and its partition; sinkRows: the slices nothing waits for (a partitioned
        std::vector<int> sinkRows;                       // instance: one per partition in the list — their epilogues finish the partitions' roots)
    } pendingWalk;
    std::vector<int> snapSourceOf;                       // resolveProgram's scratch: matrix slot -> the slot its snapshot is being taken from in this plan (-1 between calls)
    bool deferWalk = true;                               // BEAGLE_MI355_NO_ROOT_FUSION=1: never hold a launch back
    bool copyKeepsWalk = false;                          // (set around an upload the held walk does not read: engine_instance.cpp queueCopy)
    long statRootFused = 0;
    long statFoldedVectors = 0, statFoldBuilds = 0;      // read-mode programs: folded reciprocal vectors in use / (re)builds of them (engine_walk.cpp)
    unsigned* rootCounter = nullptr;                     // device word of k_rootSite's last-workgroup sum (kernels.hip)
    DevBuf cherryTables;                                 // 21..64 states: column tables of a list's virtual cherries (grow-only)
    int holdSlots = 3;                                   // what the planner was given
    bool eigenComplex = false;                           // created with BEAGLE_FLAG_EIGEN_COMPLEX: eigenvalue arrays are [S real parts | S imaginary parts]
    bool strictWaits = true;                             // a stage's wait does not count on the previous stage's stores retiring behind its
                                                         // loads (kernels.h walkStageWaits); BEAGLE_MI355_STRICT_WAITS=0 at creation: it does (1 % faster)
    bool virt = false;                                   // some partials buffers may be virtual (walk instances; T32 instances: cherries)
    bool cherry = false;                                 // T32 instance with <= 20 states: tip-tip nodes are not stored (kernels.h CherryDesc)
    long statCherries = 0;
    double hostPlanUs = 0, hostRunUs = 0, hostPrepUs = 0, hostPlanHitUs = 0, hostRunHitUs = 0; long hostCalls = 0, hostHits = 0; bool hostTrace = false, lastResolveMiss = false;   // BEAGLE_MI355_HOST_TIMING=1: where updatePartials spends host time
    DevBufUncounted bigStage;                            // device staging for programs that do not fit the ring
    // read-back (getPartials): API-layout export buffers on the device and a pinned bounce buffer on the host
    DevBufUncounted exportDev[2]; double* exportHost[2] = {nullptr, nullptr}; size_t exportBytes = 0;   // two chunks in flight
    hipEvent_t exportEvent[2] = {nullptr, nullptr};
    // The samplers' scratch, grown on demand (growScratch); what is inside each is the layout of scratch_layout.h named behind it:
    DevBuf ancestralDev;                                 // ancestral-state draws (engine_sampling.cpp drawAncestral): ancestralLayout
    DevBuf jumpDev;                                      // Markov jumps (sampleJumps): jumpLayout
    DevBuf uniformDev;                                   // uniformized Markov jumps (uniformRun): uniformLayout
    DevBuf eventDev;                                     // the event list of the last call that asked for one (growEvents): eventLayout
    DevBuf simulateDev;                                  // sequence simulation (engine_simulate.cpp): simulateLayout
    DevBuf robustDev;                                    // robust counts, on the call's first instance (engine_robustcounts.cpp): robustLayout / unconditionedLayout
    DevBuf historyDev;                                   // complete histories (engine_history.cpp): historyLayout
    DevBuf differentialDev;                              // differential matrices (engine_differential.cpp): the rotated dQ of a call, [pairs][S][S] doubles
    DevBuf eigenSweepsDev;                               // reversible-model decompositions (engine_eigen.cpp): the sweeps of the last call's models, ints
    long statEigenCalls = 0, statEigenModels = 0; int eigenLastCount = 0;      // (beagleMi355EigenStats)
    // BASTA structured coalescent (beagleBastaAllocateCoalescentBuffers, engine_basta.cpp): null on every other instance
    Basta* basta = nullptr;
    // tip error models (beagleMi355SetTipEmission, engine_tipemission.cpp): null on an instance that was never given an emission table
    TipEmissions* emis = nullptr;
    long statMicroOps = 0, statStored = 0, statMemReads = 0, statTipReads = 0, statScaleReads = 0, statWalks = 0, statScaleWrites = 0;   // since the last timer reset
    hipStream_t stream = nullptr, ownStream = nullptr;
    int tipCount = 0, partialsCount = 0, compactCount = 0, S = 0, P = 0, eigenCount = 0, matrixCount = 0, C = 0, scaleCount = 0;
    size_t partialsBytes = 0;
    std::vector<double*> partials;
    std::vector<uint8_t*> tipStates;
    struct DevBlock { void* p; size_t bytes; bool counted; };
    std::vector<DevBlock> allocations;                   // every device allocation of the instance: what destroy() frees
    char* slabCur = nullptr; int slabLeft = 0;
    char* scaleSlabCur = nullptr; int scaleSlabLeft = 0;
    char* stateSlabCur = nullptr; int stateSlabLeft = 0;
    double* matrices = nullptr; double* eigen = nullptr; double* rates = nullptr; double* weights = nullptr;
    double* freqs = nullptr; double* patternWeights = nullptr; double* siteLogL = nullptr;
    std::vector<double*> scale; std::vector<char> scaleIsRaw;
    double* blockSums = nullptr; double* dResult = nullptr; double* hResult = nullptr; double* hResultDev = nullptr; unsigned long long resultSeq = 0;
    char* hRing = nullptr; char* dRing = nullptr; size_t ringHead = 0;
    // Small host arrays (model parameters, branch lengths, programs) do not go through a copy engine: they are staged in the
    // pinned ring, which the device maps (hRingDev), and queued here; ONE kernel (kernels.hip k_hostCopies) moves everything
    // queued so far right before the next kernel or copy of the stream (live()).  A copy-engine transfer per array costs a
    // dependent blit or SDMA packet each — 25 us of a 12 500-pattern evaluation's 190 (profiles/r04_experiments.txt).
    // BEAGLE_MI355_COPY_ENGINE_UPLOADS=1 at creation: hipMemcpyAsync per array, as before round 4 (A/B runs).
    struct PendingCopy { void* dst; size_t ringOff; size_t bytes; };
    std::vector<PendingCopy> pendingCopies;
    char* hRingDev = nullptr;
    bool kernelUploads = true;
    // one process per GPU, patterns sharded over the processes: the all-reduce of the root sum runs INSIDE the engine, on the
    // instance's stream right behind the reduction kernel, and its result reaches the host through the same mapped words as a
    // single-GPU sum (beagleMi355CommInit / beagleMi355CalculateRootLogLikelihoodsAllReduce)
    ncclComm_t comm = nullptr; int commRanks = 0;
    // BeagleTreeLikelihood reads the site log-likelihoods back after EVERY evaluation (BeagleTreeLikelihood.java:1050: P doubles, 800 KB at
    // the metric's size — through a pageable destination a quarter of a 4-state evaluation's step).  A caller that has done so after each
    // of the last two whole-alignment root sums gets the next one's site values sent to a pinned host buffer (hSites; the device writes it
    // through its mapping, a kernel right behind the root's: no copy engine, no staging) before it asks: beagleGetSiteLogLikelihoods is then
    // a wait for siteEvent — over by the time the call arrives — and one host copy.  Any later root sum of the instance makes the prefetched
    // values stale (sitePrefetched = false: rootEnqueue / the by-partition sums); a caller that stops asking stops being served
    // (siteReadStreak).  BEAGLE_MI355_NO_SITE_PREFETCH=1 at creation: always the stream-ordered download (A/B runs, tests).
    bool sitePrefetch = true, sitePrefetched = false, siteReadSinceRoot = true;
    int siteReadStreak = 0; long statSitePrefetched = 0;
    double* hSites = nullptr; double* hSitesDev = nullptr; hipEvent_t siteEvent = nullptr;
    ~Instance() { if (hSites) hipHostFree(hSites); if (siteEvent) hipEventDestroy(siteEvent); }      // (destroy() has drained the streams by then)
    // first error of a deferred operation; surfaces at the next call that observes results.  Atomic: the sharded handle's caller reads and
    // clears it (sharded.cpp takeAsyncError) while the shard's own worker thread may be setting it
    std::atomic<int> asyncError{0};
    // 4 states: every slice of a walk program in ONE launch (engine_walk.cpp decideLaunch, launchWalk): per (slice, pattern group) flag words the
    // workgroups signal and poll with the launch's epoch.  BEAGLE_MI355_NO_WALK_FUSION=1 at creation: one launch per wave of slices
    bool fuseWaves = true;
    DevBufUncounted walkFlags; unsigned walkEpoch = 0;   // [flags | tickets], each half of it walkFlags.bytes / 2
    // ... or, when the slices of a program form a forest (every stored slice root has one reader: planner.h PlanSeg::next), with no
    // waiting at all: only the slices without dependencies get workgroups, and the workgroup that arrives last at a slice above runs it
    // (kernels_walk4.hip "tickets"; walkTickets: per (slice, pattern group) arrival counts, zero between launches, in the same
    // allocation behind the flags).  BEAGLE_MI355_NO_WALK_TICKETS=1 at creation: dependency flags always (A/B runs, tests)
    bool useTickets = true; unsigned* walkTickets = nullptr;
    // ... and such a launch, when the chip holds all of it at once and it has rows for every XCD, lays its rows out XCD by XCD (kernels_walk4.hip
    // launchWalk4Fast: small partitioned alignments).  BEAGLE_MI355_NO_XCD_MAP=1 at creation: always the plain 2-D grid (A/B runs)
    bool xcdAware = true;
    // 4 states, assembly loop: a node over two compact tips that is not stored, pays no scale factors and is consumed by the very next
    // micro-operation is not a micro-operation of the device program at all: its consumer evaluates it inside its own stage (kernels.h
    // WK_CHERRY; engine_walk.cpp ProgramResolver::microOp).  Same arithmetic in the same order: bitwise the unfused program.  A third of a tree's nodes.
    // BEAGLE_MI355_NO_CHERRY_FUSION=1 at creation: every micro-operation of the plan is one of the device program (A/B runs, tests)
    bool fuseCherries = true; long statFused = 0;
    // ... and the loop's fetch loads tip states only for children that ARE compact tips (kernels.h WF_NOLOAD1 / 2; programs without
    // write-mode rescaling).  BEAGLE_MI355_NO_LOAD_SKIP=1 at creation: both tip-state loads in every fetch, as before round 6 (A/B runs)
    bool skipTipLoads = true;
    // Write-mode programs (4 states, one partition): every slice leaves the product of the factors it wrote per pattern — mantissa and binary
    // exponent, [slice row][pair position] — and an accumulateScaleFactors call over EXACTLY the scale buffers the last such program wrote (what
    // BEAST issues right behind it: BeagleTreeLikelihood.java:1013-1026) adds a few dozen logarithms per pattern instead of reading a factor per
    // node (kernels.hip k_accumulateSlices; config A, ALWAYS rescaling: 250 us and 0.8 GB per evaluation).  Anything else — another list, a
    // scale buffer written since (scaleWriteEpoch) — takes the general kernel.  BEAGLE_MI355_NO_SLICE_SUMS=1 at creation: always the general kernel.
    bool sliceSums = true;
    DevBufUncounted sliceMant, sliceExp; size_t sliceRows = 0;      // (doubles; ints)
    struct LastSums { bool valid = false; long epoch = -1, gen = 0; std::vector<int> rows; int nWritten = 0; } lastSums;
    std::vector<long> scaleGen, scaleSeen; long sliceGen = 0, seenCounter = 0, statSliceAccum = 0;
    long statTicketWalks = 0, statFlagWalks = 0, lastLaunchRows = 0, lastLaunchSlices = 0;      // (beagleMi355WalkLaunchInfo)
    // how long a workgroup of that launch polls before it computes what it waits for itself (kernels_walk4.hip: forward progress does
    // not rest on the dispatch order), in ticks of the device's 100 MHz wall clock: 20 ms — an evaluation of the largest alignment
    // this engine is measured on takes 0.6; BEAGLE_MI355_WALK_SPIN_US=<us> at creation (tests: 0 forces the self-serve path).
    // walkSelfServed: device word that counts the workgroups whose wait ran out (beagleMi355WalkHealth).
    unsigned long long walkSpinLimit = 2000000ull; unsigned* walkSelfServed = nullptr;
    int partitionCount = 1;
    std::vector<int> partStart, partEnd;
    // levelisation scratch
    std::vector<int> wStamp, wLevel, rStamp, rLevel, wOp; int stamp = 0;
    bool tiled = false; int ntile = 0;   // T32 partials layout (MFMA path)
    // pre-order on the T32 layout runs as two passes of the pruning kernel (see runPreOperations): scratch partials
    // buffers, an identity matrix and transposed-matrix slots behind the caller's matrices, an all-missing tip
    std::vector<double*> preScratch; uint8_t* preMissing = nullptr; int preIdentity = -1, preTransposed = -1;
    bool schedAlap = true;               // BEAGLE_MI355_SCHED=asap restores as-soon-as-possible levels
    int schedDfs = 0;                    // > 0 (BEAGLE_MI355_SCHED=dfs[:K]): launches of at most K operations in depth-first order (engine_levels.cpp)
    // kernel timer
    bool timing = false;
    int timingEvery = 1, timingTick = 0; long timedCalls = 0;      // every timingEvery-th updatePartials call is bracketed (beagleMi355KernelTimer)
    std::vector<std::pair<hipEvent_t, hipEvent_t>> events; size_t eventsUsed = 0;
    double timedMs = 0.0; long timedLaunches = 0, pendingLaunches = 0;
    size_t deviceBytes = 0;
    std::vector<double> shEigen, shFreqs, shWeights, shRates;      // host shadows of the small model arrays ...
    std::vector<char> okEigen, okFreqs, okWeights, okRates;         // ... valid flags per index
    std::string resourceName;
    DevBuf generatorDev;                                 // matrices from generators (engine_generator.cpp): the power tables of a launch, [generators][21][S][S] doubles
    DevBuf generatorStatsDev;                            // ... and two words the kernels keep: the largest s, the matrices refused
    long statGeneratorCalls = 0, statGeneratorMatrices = 0;                    // (beagleMi355GeneratorStats)
    long statEpochCalls = 0, statEpochMatrices = 0, statEpochSegments = 0, statEpochLongest = 0;      // (beagleMi355EpochStats)
    DevBuf nodePatternDev;                               // stochastic Dollo node-pattern likelihood (engine_nodepattern.cpp): nodePatternLayout
    long statNodePatternCalls = 0, statNodePatternRows = 0, statNodePatternEmpty = 0, statNodePatternMaterialised = 0;      // (beagleMi355NodePatternStats)
    DevBuf nodePosteriorDev;                             // marginal node state posteriors (engine_nodeposterior.cpp): nodePosteriorLayout
    long statNodePosteriorCalls = 0, statNodePosteriorRows = 0, statNodePosteriorMaterialised = 0, statNodePosteriorLaunches = 0;   // (beagleMi355NodePosteriorStats)
    DevBuf placementDev;                                 // placement scores (engine_placement.cpp): placementLayout
    long statPlacementCalls = 0, statPlacementCandidates = 0, statPlacementMaterialised = 0, statPlacementLaunches = 0;   // (beagleMi355PlacementStats)
    DevBuf regraftDev;                                   // regraft scores (engine_regraft.cpp): regraftLayout
    long statRegraftCalls = 0, statRegraftCandidates = 0, statRegraftMaterialised = 0, statRegraftLaunches = 0;           // (beagleMi355RegraftStats)
};

extern std::mutex g_mutex;
extern std::vector<Instance*> g_instances;
Instance* lookup(int h);

// ---- engine_instance.cpp: memory, staging, resources
int devAlloc(Instance* in, void** p, size_t bytes, bool counted = true);
void devFree(Instance* in, void* p);                     // a block devAlloc gave out, off the list; synchronising is the caller's business
// at least `need` bytes in b: when it has to grow it allocates `want` (>= need) and deals with the old block as `how` says.
// *grew (nullable): the buffer's address changed.  A failed allocation leaves b empty, never half-set.
int growDevice(Instance* in, DevBuf& b, size_t need, size_t want, Grow how, bool* grew = nullptr);
void releaseDevice(Instance* in, DevBuf& b);             // (synchronising is the caller's business)
// the samplers' scratch: exactly `need` bytes when it grows
inline int growScratch(Instance* in, DevBuf& b, size_t need) { return growDevice(in, b, need, need, Grow::SyncIfHeld); }
static_assert(mi355::scratch::FLAG_SLOTS == mi355::MAX_JUMP_REGISTERS, "scratch_layout.h keeps one flag word per possible register");
long stage(Instance* in, const void* src, size_t bytes, size_t reserve = 0);
int upload(Instance* in, void* dst, const void* src, size_t bytes);
int uploadTransient(Instance* in, const void* src, size_t bytes, void** dptr);
int download(Instance* in, void* dst, const void* src, size_t bytes);
int ensurePartials(Instance* in, int idx);
int ensureScale(Instance* in, int idx);
int ensureStates(Instance* in, int idx);
void destroy(Instance* in);
struct Resources {
    std::vector<std::string> names, descs;
    std::vector<BeagleResource> list;
    BeagleResourceList rl;
    int gpuCount = 0;
};
extern const long GPU_FLAGS;
Resources* resources();
void setPairLayout(Instance* in);
int holdPreList(Instance* in, const int* ops, int count);
bool supersedesHeld(Instance* in, const int* ops, int count);
int ensureWalkDummies(Instance* in);
// the instance's stream, with everything queued in pendingCopies enqueued on it first: what every launch, copy and
// synchronisation of the engine passes as its stream (only flushUploads itself and the stream setters touch in->stream)
int flushUploads(Instance* in);
// ... and a walk launch that is being held back for the root call (PendingWalk, engine_walk.cpp) launched behind them
int flushWalk(Instance* in, const mi355::RootFused* root = nullptr);
inline hipStream_t live(Instance* in) {
    if (!in->pendingCopies.empty()) flushUploads(in);
    if (in->pendingWalk.valid) flushWalk(in);
    return in->stream;
}
// queue `bytes` already staged at ring offset `off` for device address dst (or copy them now: kernelUploads off)
int queueCopy(Instance* in, void* dst, size_t off, size_t bytes);
// the stream is idle, or a result behind everything staged so far has been seen: with nothing queued the ring starts over
inline void ringIdle(Instance* in) { if (in->pendingCopies.empty() && !in->pendingWalk.valid) in->ringHead = 0; }
// while one of these lives, an upload leaves a held walk launch held: what is uploaded is the root's input or the held walk's own,
// nothing the walk's kernels before it read (Instance::copyKeepsWalk, queueCopy)
struct KeepWalkHeld {
    Instance* in;
    explicit KeepWalkHeld(Instance* i) : in(i) { in->copyKeepsWalk = true; }
    ~KeepWalkHeld() { in->copyKeepsWalk = false; }
};

// (a held-back pre-order list — Instance::heldPre — runs before anything else touches the instance; the few calls that cannot
// interact with it use GET_INSTANCE_KEEP_PENDING)
#define GET_INSTANCE_KEEP_PENDING(h)                             \
    Instance* in = lookup(h);                                    \
    if (!in) return BEAGLE_ERROR_UNINITIALIZED_INSTANCE;         \
    if (hipSetDevice(in->device) != hipSuccess) return BEAGLE_ERROR_GENERAL;
#define GET_INSTANCE(h)                                          \
    GET_INSTANCE_KEEP_PENDING(h)                                 \
    if (in->heldPre.held) { const int rcPending__ = executeHeldPre(in); if (rcPending__) return rcPending__; }

// A device temporary of one call: drains the instance's stream and frees the block when it leaves scope, on every exit path.  Not on
// the allocation list and not counted — it never outlives the call.
struct ScopedDevice {
    Instance* in; void* p = nullptr;
    explicit ScopedDevice(Instance* i) : in(i) {}
    ScopedDevice(const ScopedDevice&) = delete; ScopedDevice& operator=(const ScopedDevice&) = delete;
    int alloc(size_t bytes);                             // BEAGLE_ERROR_OUT_OF_MEMORY when there is none
    template <class T> T* as() const { return static_cast<T*>(p); }
    void reset();
    ~ScopedDevice() { reset(); }
};

inline bool badIndex(int i, int n) { return i < 0 || i >= n; }

// ---- engine_tipemission.cpp: tips whose partials are a lookup E[code][state].  With K <= S codes such a tip stays a
// compact tip and its branch matrix becomes M E^T, written into a SHADOW slot behind every other matrix slot of the instance (one
// shadow per caller matrix index) in front of each operation list that names the tip; otherwise, and for every caller that needs the
// tip's partials as data, the lookup is written out as a partials buffer on the device ("expanded").
struct TipEmission {
    int K = 0;                                           // 0: the tip has no emission
    bool folded = false;                                 // route 1 (K <= S and no caller has needed the partials since the codes came); otherwise expanded
    std::vector<uint8_t> codes;                          // [P], 255 = outside the table (missing)
    std::vector<double> table;                           // [K][S] as the caller gave it
    DevBuf dTable;                                       // ... on the device (doubles)
    uint8_t* dCodes = nullptr; bool codesOnDevice = false;      // expanded tips: the codes on the device
};
struct TipEmissions {
    std::vector<TipEmission> tips;
    int shadowBase = 0;                                  // matrix slot of caller index 0's shadow (engine_create.cpp matrixSlotLayout)
    int foldedCount = 0, expandedCount = 0;
    long foldLaunches = 0, demotions = 0;
    std::vector<int> ops, useOf; std::vector<long> useStamp; long stamp = 0;      // runOperations' rewritten list; per matrix index who uses it in this list
    std::vector<mi355::TipFoldJob> jobs;
};
inline bool foldedTip(const Instance* in, int X) { return in->emis && X >= 0 && X < in->tipCount && in->emis->tips[(size_t)X].folded; }
// a matrix index an operation may name: the caller's, or (lists rewritten by foldTipOperations) a shadow slot
inline bool badMatrix(const Instance* in, int m) {
    return badIndex(m, in->matrixCount) && !(in->emis && m >= in->emis->shadowBase && m < in->emis->shadowBase + in->matrixCount);
}
// runOperations' pre-pass: *ops becomes the list with every folded tip's matrix index replaced by its shadow, and the shadows are written
int foldTipOperations(Instance* in, const int** ops, int count, int tuple);
int demoteFoldedTip(Instance* in, int tip);              // a folded tip becomes an expanded one (its partials exist)
int demoteFoldedTips(Instance* in);                      // ... every folded tip
void dropTipEmission(Instance* in, int tip);             // setTipStates / setTipPartials: the tip is the caller's again
void freeTipEmissions(Instance* in);
#define DEMOTE_FOLDED_TIPS(in) do { if ((in)->emis) { const int rcDemote__ = demoteFoldedTips(in); if (rcDemote__) return rcDemote__; } } while (0)
// The kernel timer's bracket around the launches of ONE call (beagleMi355KernelTimer): begin() in front of them, the first event in
// front of the first launch (start(), or a callee that is handed first()), stop() behind the last one.  Whichever way the call ends,
// error returns included, Instance::eventsUsed counts exactly the pairs with both events recorded and Instance::timedCalls the
// calls that contributed one: a pair stopped without a launch, or never stopped, goes back.  live(in) is taken only when there is an
// event to record (on an untimed call it would launch a walk that is being held back for the root call: PendingWalk).
struct CallTimer {
    explicit CallTimer(Instance* i) : in(i) {}
    CallTimer(const CallTimer&) = delete; CallTimer& operator=(const CallTimer&) = delete;
    ~CallTimer() { stop(0); if (counted && !pairs) in->timedCalls--; }
    // Is this call one the timer brackets (an event costs a barrier packet on the stream: 6 us of an evaluation each — a sampled timer
    // keeps that out of most of a timed region)?  Decided at the call's first begin(); if so, the next HIP-event pair of the instance
    // (one is created when none is left).  A call that brackets its chunks one by one begins again per chunk: one counted call, a pair each.
    int begin() {
        if (!decided && in->timing && ++in->timingTick >= in->timingEvery) { in->timingTick = 0; in->timedCalls++; counted = true; }
        decided = true;
        if (!counted || e1) return 0;
        if (in->eventsUsed == in->events.size()) {
            hipEvent_t a = nullptr, b = nullptr;
            HIP_TRY(hipEventCreate(&a)); HIP_TRY(hipEventCreate(&b));
            in->events.emplace_back(a, b);
        }
        e0 = in->events[in->eventsUsed].first; e1 = in->events[in->eventsUsed].second; in->eventsUsed++;
        return 0;
    }
    // the first event, once: handed to a callee that records it itself right in front of its launch (runPlan's recordBeforeWalk), or
    // recorded here — what a loop over chunks calls in front of every chunk's first launch (it begins, where the caller has not)
    hipEvent_t first() { hipEvent_t e = e0; e0 = nullptr; return e; }
    int start() {
        const int rc = begin(); if (rc) return rc;
        if (hipEvent_t e = first()) HIP_TRY(hipEventRecord(e, live(in)));
        return 0;
    }
    // behind the last launch: the second event and the launches the pair stands for; nothing was launched: the pair goes back
    int stop(int launches) {
        if (!e1) return 0;
        if (launches > 0) { HIP_TRY(hipEventRecord(e1, live(in))); in->pendingLaunches += launches; pairs++; }
        else in->eventsUsed--;
        e0 = e1 = nullptr;
        return 0;
    }
private:
    Instance* const in;
    hipEvent_t e0 = nullptr, e1 = nullptr;               // the pair in hand (e0: until it is handed out)
    bool decided = false, counted = false; int pairs = 0;      // (pairs: of this call, with both events recorded)
};

// ---- the pattern walk (4 states) ------------------------------------------------------------------------------------
// A partials buffer is "virtual" when its content is DEFINED instead of stored (planner.h VirtDef): a few steps over
// compact tips, private snapshots of every branch matrix in the subtree (kept behind the caller's matrices) and each
// node's scale buffer.  Nothing is written to HBM for such a buffer; the walk recomputes it in registers where a parent
// needs it, bitwise as the ordinary operation would have.  The definition is self-contained: it never refers to other
// partials buffers or to the caller's matrix buffers, so buffer flips and matrix updates cannot invalidate it.  What CAN
// change a defining input — new tip states, a write to one of its scale buffers — and everything that needs the real
// data — getPartials, use as root, the pre-order kernels — first calls materializeList, which runs the definition with
// a store.
static_assert(mi355::PK_MEM == mi355::WK_MEM && mi355::PK_TIPS == mi355::WK_TIPS && mi355::PK_ACC == mi355::WK_ACC &&
              mi355::PK_H0 == mi355::WK_H0 && mi355::PK_H1 == mi355::WK_H1 && mi355::PK_H2 == mi355::WK_H2, "planner kinds = kernel kinds");
static_assert(mi355::PS_NONE == mi355::WS_NONE && mi355::PS_READ == mi355::WS_READ && mi355::PS_WRITE == mi355::WS_WRITE, "scale modes");

inline bool isVirt(const Instance* in, int X) { return in->virt && in->planner.isVirtual(X); }
inline void clearVirtual(Instance* in, int X) { if (in->virt) in->planner.clearVirtual(X); }
inline bool isCompactTip(const Instance* in, int X) { return in->tipStates[X] && X < in->tipCount; }
// what buffer X holds changed: compact tip states (on), or something else — in which case it is no uploaded-partials leaf
// either until setLeaf says so (planner.h leafPartials)
void repeatsForget(Instance* in);     // (engine_walk.cpp: the class indices and tables are of the tip states they were built from)
void repeatsIdle(Instance* in);
inline void setCompact(Instance* in, int X, bool on) {
    in->planner.setCompactTip(X, on); in->planner.setLeafPartials(X, false);
    if (in->repeatsOn && !on && X < in->tipCount && !in->hostTips[(size_t)X].empty()) { in->repeatIndex.setTip(X, nullptr); in->hostTips[(size_t)X].clear(); repeatsForget(in); }
}
inline void setLeaf(Instance* in, int X) { if (X < in->tipCount) in->planner.setLeafPartials(X, true); }

// ---- engine_walk.cpp
int runPlan(Instance* in, const mi355::Plan& plan, long planTag = 0, hipEvent_t recordBeforeWalk = nullptr);
inline void scalesWritten(Instance* in) { in->scaleWriteEpoch++; }       // (Instance::folds)
void forgetFolds(Instance* in);                                          // the layout of the scale buffers changes
int materializeList(Instance* in, const std::vector<int>& xs);
int materializeVirtual(Instance* in, int X);
int materializeScaleUsers(Instance* in, int scaleIdx);
int materializeTipUsers(Instance* in, int tip);
int walkChunkOps(const Instance* in, int opCount);
void walkRepeatChunkOps(const Instance* in, long weight, int& chunk, int& top);
int runOperationsWalk(Instance* in, const int* ops, int count, int tuple, int globalCum);
// ---- engine_levels.cpp
int materializeCherries(Instance* in, const std::vector<int>& xs);
int runOperationsLevels(Instance* in, const int* ops, int count, int tuple, int globalCum);
int foldCumulative(Instance* in, const int* ops, int count, int tuple, int globalCum);
int runOperations(Instance* in, const int* ops, int count, int tuple, int globalCum);
// ---- engine_preorder.cpp
int ensurePreScratch(Instance* in);
int ensureEdgeScratch(Instance* in, size_t bytes);
// does a call that writes matrix m / reads or writes partials buffer b have to wait for the held pre-order list?
inline bool heldReadsMatrix(const Instance* in, int m) { return in->heldPre.held && m >= 0 && m < (int)in->heldPre.readsMatrix.size() && in->heldPre.readsMatrix[m]; }
inline bool heldWrites(const Instance* in, int b) { return in->heldPre.held && b >= 0 && b < (int)in->heldPre.writesBuf.size() && in->heldPre.writesBuf[b]; }
inline bool heldTouches(const Instance* in, int b) { return in->heldPre.held && b >= 0 && b < (int)in->heldPre.writesBuf.size() && (in->heldPre.writesBuf[b] || in->heldPre.readsBuf[b]); }
int runPreOperations(Instance* in, const int* ops, int count, int globalCum, bool mayHold = false, int tuple = BEAGLE_OP_COUNT);
int executeHeldPre(Instance* in);
int edgeDifferentials(Instance* in, const int* postIdx, const int* preIdx, const int* dIdx, int wIdx, int count,
                      double* outDerivatives, double* outSum, double* outSumSquared);
int crossProducts(Instance* in, const int* postIdx, const int* preIdx, int rateIdx, int wIdx, const double* lengths, int count, double* outSum);
// ---- what a call reads as data must BE data: the partials buffers (valid indices) a call is about to read.  A buffer is stored;
// unstored (defined by the 4-state walk: its definition keys are noted, in order of first appearance, each once); a compact tip, read
// as states; a folded emission tip, which the caller demotes or does not read as data; or never written to: BEAGLE_ERROR_OUT_OF_RANGE.
// materialize() gives the noted definitions real data in one materializeList.  Nothing changes before it: a list that fails leaves
// the instance as it was.
struct ReadSet {
    explicit ReadSet(Instance* i) : in(i) {}
    int post(int b) { return isCompactTip(in, b) || foldedTip(in, b) ? 0 : pre(b); }       // a post-order operand
    // a pre-order operand: compact states are no partials (nor is a pre-order buffer ever a destination the walk leaves unstored: a
    // caller that names an unstored post-order buffer here still reads real data)
    int pre(int b) { return note(b) || (!isCompactTip(in, b) && in->partials[b]) ? 0 : (int)BEAGLE_ERROR_OUT_OF_RANGE; }
    // b's definition keys if it is unstored (-> true): all that a caller needs that has classified b itself (an operand that an
    // earlier operation of its own list writes is no error)
    bool note(int b) {
        if (!isVirt(in, b)) return false;
        ofOne.clear(); in->planner.keysOf(b, ofOne);
        for (int key : ofOne) noteKey(key);
        return true;
    }
    // ... and a definition key the caller has from elsewhere (the planner's lists of who reads a tip or a scale buffer)
    void noteKey(int key) {
        if ((size_t)key >= noted.size()) noted.resize(std::max((size_t)key + 1, (size_t)in->partialsCount * in->planner.partitionCount()), 0);
        if (!noted[(size_t)key]) { noted[(size_t)key] = 1; need.push_back(key); }
    }
    size_t keys() const { return need.size(); }            // distinct definitions noted so far
    int materialize() { return materializeList(in, need); }
private:
    Instance* const in;
    std::vector<int> need, ofOne; std::vector<char> noted;
};
// ... and where a descriptor finds such an operand once the read set is materialised: a post-order operand's partials or (*states)
// compact states, a pre-order operand's partials.  Null: nothing there, the fill's BEAGLE_ERROR_OUT_OF_RANGE.
inline const void* postOperand(const Instance* in, int b, int* states) {
    *states = isCompactTip(in, b);
    return *states ? (const void*)in->tipStates[b] : (const void*)in->partials[b];
}
inline const double* preOperand(const Instance* in, int b) { return isCompactTip(in, b) ? nullptr : in->partials[b]; }
// What an entry point that reads pre- and post-order partials where they are calls once, behind its own checks and under
// GET_INSTANCE_KEEP_PENDING; collect(ReadSet&) checks the call's indices and feeds the read set.  The whole list BEFORE anything changes
// (a list that fails leaves the instance, and a held-back pre-order list, as they were); then the held list, which writes the pre-order
// partials the call reads and gives its own unstored operands — the call's among them — real data; folded tips demoted (their partials
// are read as data: engine_tipemission.cpp); the list again, for what is STILL unstored (*unstoredAtEntry: the first pass's distinct
// definitions, what the ...Materialised statistics count); one materializeList.
template <class Collect> int makeResident(Instance* in, Collect&& collect, long* unstoredAtEntry) {
    ReadSet atEntry(in), reads(in);
    int rc = collect(atEntry); if (rc) return rc;
    *unstoredAtEntry = (long)atEntry.keys();
    if (in->heldPre.held) { rc = executeHeldPre(in); if (rc) return rc; }
    DEMOTE_FOLDED_TIPS(in);
    rc = collect(reads); if (rc) return rc;
    return reads.materialize();
}
// One candidate attachment of beagleMi355PlacementScores / beagleMi355RegraftScores, {parentPre, siblingPost, siblingMatrix, childPost,
// upperMatrix, lowerMatrix, pendantMatrix}: its indices checked (only the sibling pair, together, and the upper matrix may be
// BEAGLE_OP_NONE) and its three buffers fed to the read set — what both entry points call per row inside their makeResident collect.
constexpr int ATTACH_FIELDS = 7;
enum { ATTACH_PARENT_PRE, ATTACH_SIBLING_POST, ATTACH_SIBLING_MATRIX, ATTACH_CHILD_POST, ATTACH_UPPER_MATRIX, ATTACH_LOWER_MATRIX, ATTACH_PENDANT_MATRIX };
inline int checkAttachment(const Instance* in, const int* c, ReadSet& reads) {
    const int pre = c[ATTACH_PARENT_PRE], sib = c[ATTACH_SIBLING_POST], mSib = c[ATTACH_SIBLING_MATRIX], child = c[ATTACH_CHILD_POST];
    if (badIndex(pre, in->partialsCount) || badIndex(child, in->partialsCount)) return BEAGLE_ERROR_OUT_OF_RANGE;
    if ((sib == BEAGLE_OP_NONE) != (mSib == BEAGLE_OP_NONE)) return BEAGLE_ERROR_OUT_OF_RANGE;
    if (sib != BEAGLE_OP_NONE && (badIndex(sib, in->partialsCount) || badIndex(mSib, in->matrixCount))) return BEAGLE_ERROR_OUT_OF_RANGE;
    if (c[ATTACH_UPPER_MATRIX] != BEAGLE_OP_NONE && badIndex(c[ATTACH_UPPER_MATRIX], in->matrixCount)) return BEAGLE_ERROR_OUT_OF_RANGE;
    if (badIndex(c[ATTACH_LOWER_MATRIX], in->matrixCount) || badIndex(c[ATTACH_PENDANT_MATRIX], in->matrixCount)) return BEAGLE_ERROR_OUT_OF_RANGE;
    if (int bad = reads.pre(pre)) return bad;
    if (sib != BEAGLE_OP_NONE) if (int bad = reads.post(sib)) return bad;
    return reads.post(child);
}
// ... and its descriptor once the read set is resident (pendant: which of the call's distinct pendant matrices; slot: its row of
// the launch).  BEAGLE_ERROR_OUT_OF_RANGE: a buffer that holds nothing.
inline int fillAttachment(const Instance* in, const int* c, int pendant, int slot, mi355::PlacementCandidate* row) {
    const size_t SS = (size_t)in->C * in->S * in->S;
    *row = mi355::PlacementCandidate{};
    row->pre = preOperand(in, c[ATTACH_PARENT_PRE]);
    if (c[ATTACH_SIBLING_POST] != BEAGLE_OP_NONE) {
        row->sib = postOperand(in, c[ATTACH_SIBLING_POST], &row->sibStates);
        row->mSib = in->matrices + SS * c[ATTACH_SIBLING_MATRIX];
        if (!row->sib) return BEAGLE_ERROR_OUT_OF_RANGE;
    }
    row->child = postOperand(in, c[ATTACH_CHILD_POST], &row->childStates);
    row->mUp = c[ATTACH_UPPER_MATRIX] == BEAGLE_OP_NONE ? nullptr : in->matrices + SS * c[ATTACH_UPPER_MATRIX];
    row->mLow = in->matrices + SS * c[ATTACH_LOWER_MATRIX];
    row->pendant = pendant;
    row->slot = slot;
    return row->pre && row->child ? 0 : (int)BEAGLE_ERROR_OUT_OF_RANGE;
}

// ---- engine_sampling.cpp
// Where a device-side draw left its results (in->ancestralDev, scratch_layout.h ancestralLayout)
struct AncestralDraw { uint8_t* states; int* cats; unsigned* error; };
// the draw of beagleMi355SampleAncestralStates left on the device (one launch on the instance's stream), and its copy-out
int drawAncestral(Instance* in, const int* nodes, int nodeCount, int wIdx, int fIdx, unsigned long long seed, int flags, int globalP,
                  int pOffset, AncestralDraw* d);
int copyAncestral(Instance* in, const AncestralDraw& d, int nodeCount, int globalP, int pOffset, unsigned char* outStates,
                  int* outCategories, unsigned* error);
// every register's flags within `allowed` (flags == nullptr: none set)
inline bool checkRegisterFlags(const int* flags, int K, int allowed) {
    for (int k = 0; flags && k < K; k++) if (flags[k] & ~allowed) return false;
    return true;
}
// Per-row values [K][R][P] leave through a stage of at most 256 MiB (and `cap` rows): the rows of one launch
inline size_t stageRowCount(size_t R, size_t K, size_t P, size_t cap = SIZE_MAX) {
    return std::max<size_t>(1, std::min<size_t>({R, (256ull << 20) / (K * P * sizeof(double)), cap}));
}
// rows r0 .. r1 - 1 of the stage [K][stride][P] (its row 0 = row r0) to out[k][R][globalP] at column pOffset, one copy per register —
// linear where the instance has every column — then the synchronisation the next chunk's launch needs (it overwrites the stage)
int copyStagedRows(Instance* in, const double* stage, size_t stride, size_t r0, size_t r1, int K, size_t R, size_t P, size_t globalP,
                   size_t pOffset, double* out);
// pattern totals [K][P] into their columns of outPatternTotals [K][globalP], this instance's row totals [K][R]; either may be NULL (queued)
int copyJumpTotals(Instance* in, const double* dPat, const double* dRow, int K, size_t R, size_t P, size_t globalP, size_t pOffset,
                   double* outPatternTotals, double* outRowTotals);
// an event list of n events on the device (in->eventDev, scratch_layout.h eventLayout)
int growEvents(Instance* in, size_t n, uint8_t** states, double** heights);
// ... and its way out (either may be NULL), synchronised
int copyEvents(Instance* in, size_t n, const uint8_t* states, const double* heights, unsigned char* outStates, double* outHeights);

// ---- engine_simulate.cpp: the front end of the site-keyed simulators (sequences, complete histories).  A node list names per row
// {outRow or -1, matrix or generator, parent row}; a node with an outRow keeps its states in scratch row ("slot") outRow, so that the
// wanted rows leave as a few strided copies, the others behind the largest outRow.
// The list's shape (outRow >= -1 and unique, parent before child) and the caller's root states and categories; *maxOut: the largest outRow
int checkSiteCall(const int* nodes, int nodeCount, int siteCount, const unsigned char* inRootStates, const int* inRateCategories, int S,
                  int C, int* maxOut);
// rows[r].slot / parentSlot / parentIsPrev of every row (Row: SimRow, HistoryRow); *slots: scratch rows in all
template <class Row>
int assignSlots(const int* nodes, int nodeCount, int maxOut, std::vector<Row>& rows, size_t* slots) {
    size_t next = (size_t)maxOut + 1;
    for (int r = 0; r < nodeCount; r++) {
        const int out = nodes[3 * r], parent = nodes[3 * r + 2];
        const size_t slot = out >= 0 ? (size_t)out : next++;
        if (slot > (size_t)INT_MAX) return BEAGLE_ERROR_OUT_OF_RANGE;
        rows[r].slot = (int)slot;
        rows[r].parentSlot = r == 0 ? -1 : rows[parent].slot;
        rows[r].parentIsPrev = r > 0 && parent == r - 1;
    }
    *slots = next;
    return 0;
}
// the sites of one launch: `wanted`, or the environment's `envName`=<n> (tests: chunk independence at a small size), no more than
// `sites`, in whole `unit`s
size_t chunkSites(const char* envName, size_t unit, size_t wanted, size_t sites);
// the outRows of a list in ascending order, and their scratch rows' first `count` sites out to outStates[outRow][siteCount] at site
// `first`: runs of consecutive rows as one strided copy each (queued)
std::vector<int> wantedRows(const int* nodes, int nodeCount);
int copyWantedRows(Instance* in, const std::vector<int>& wanted, const uint8_t* dStates, size_t chunk, size_t count, unsigned char* outStates,
                   size_t siteCount, size_t first);
// a call over siteCount sites on a handle of `shards` instances (a plain handle: one) of S states and C categories: the instances
// take sites [siteCount k / n, siteCount (k + 1) / n) by order of arrival (the results are keyed on the site, so which takes which
// part does not matter)
struct SiteSplit {
    int S = 0, C = 0, shards = 1, siteCount = 0; std::atomic<int> arrivals{0};
    int init(int handle, int sites);
    bool next(int* site0, int* site1) {
        const int k = arrivals.fetch_add(1);
        *site0 = (int)((long long)siteCount * k / shards); *site1 = (int)((long long)siteCount * (k + 1) / shards);
        return k < shards;
    }
};

// ---- engine_create.cpp
size_t matrixSlotLayout(Instance* in);
int uploadIdentityMatrix(Instance* in);

// ---- engine_basta.cpp: an instance that has BASTA buffers keeps its S-double vectors there (setPartials / getPartials)
int bastaSetPartials(Instance* in, int bufferIndex, const double* inPartials);
int bastaGetPartials(Instance* in, int bufferIndex, double* outPartials);
void bastaFree(Instance* in);

}  // namespace eng
}  // namespace mi355
