// planner.cpp — see planner.h.  Pure host logic (compiled into the engine by hipcc and into the planner test by g++).
#include "planner.h"

#include <algorithm>
#include <cstring>

namespace mi355 {

namespace {
constexpr int OP_NONE = -1;                 // BEAGLE_OP_NONE
enum { CL_TIPS = 0, CL_MEM = 1, CL_VIRT = 2, CL_REAL = 3, CL_PATH = 4 };      // (CL_PATH: planner.h memStepCap, emitReal)
inline int popcount2(unsigned m) { return (int)(m & 1u) + (int)((m >> 1) & 1u) + (int)((m >> 2) & 1u); }      // free hold slots (up to 3)
inline int lowestSlot(unsigned m) { return (m & 1u) ? 0 : (m & 2u) ? 1 : 2; }

// The path of a memory definition (planner.h memStepCap): the steps from memStep — the one that reads the stored operand — up to step
// `upTo`, each of them the step that has the one before it as an operand (steps are in post-order: it comes later).  visit(t, off) is
// called for every step t on the path, bottom up; `off` is the operand of t that is NOT on the path when that is an earlier step of the
// definition — the other side of a VT_JOIN, subA of a VT_EXTEND that reads the stored operand as its leaf — and -1 when it is a tip.
// Returns the last step reached: `upTo` exactly when that step is on the path.
template <class Visit> int walkMemPath(const VirtDef& v, int upTo, Visit visit) {
    int p = v.memStep;
    visit(p, v.steps[p].type == VT_EXTEND ? v.steps[p].subA : -1);
    for (int t = p + 1; t <= upTo && p != upTo; t++) {
        const VirtStep& s = v.steps[t];
        if (s.subA != p && s.subB != p) continue;
        visit(t, s.type == VT_JOIN ? (s.subA == p ? s.subB : s.subA) : -1);
        p = t;
    }
    return p;
}

// The slice (index into plan.segs) that holds micro-operation `at` of plan.prog, -1: none.  Slices tile the program in any order and a
// plan has a handful of them, so this is a scan.
inline int sliceHolding(const Plan& plan, int at) {
    for (size_t s = 0; s < plan.segs.size(); s++)
        if (at >= plan.segs[s].progStart && at < plan.segs[s].progStart + plan.segs[s].progCount) return (int)s;
    return -1;
}
}  // namespace

void WalkPlanner::init(int partialsCount, int tipCount, int matrixCount, int scaleCount, int maxVirtSteps, bool virtualEnabled, int holdSlots) {
    allSlots_ = (1u << std::max(0, std::min(3, holdSlots))) - 1u;          // (0: no hold slots at all — the 21..64-state walk)
    partialsCount_ = partialsCount; tipCount_ = tipCount; matrixCount_ = matrixCount; scaleCount_ = std::max(1, scaleCount);
    maxSteps_ = std::max(1, std::min(maxVirtSteps, PLAN_MAX_STEPS));
    enabled_ = virtualEnabled;
    keyParts_ = 1;
    virt_.assign(partialsCount, VirtDef());
    tagOf_.assign(partialsCount, -1); tagEpoch_++;
    tipUsers_.assign(partialsCount, std::vector<int>());
    scaleUsers_.assign(scaleCount_, std::vector<int>());
    compactTip.assign(partialsCount, 0);
    leafPartials.assign(partialsCount, 0);
    wStamp_.assign(partialsCount, 0); rStamp_.assign(partialsCount, 0); wOp_.assign(partialsCount, 0);
    sWStamp_.assign(scaleCount_, 0); sRStamp_.assign(scaleCount_, 0); sDone_.assign(scaleCount_, 0);
    stamp_ = 0; virtVersion_ = 0;
}

void WalkPlanner::setPartitionCount(int parts) {
    keyParts_ = std::max(1, parts);
    virt_.assign((size_t)partialsCount_ * keyParts_, VirtDef());
    tagOf_.assign((size_t)partialsCount_ * keyParts_, -1); tagEpoch_++;
    for (auto& u : tipUsers_) u.clear();
    for (auto& u : scaleUsers_) u.clear();
    for (CacheEntry& e : cache_) e.valid = false;
}

void WalkPlanner::clearVirtualKey(int X) {
    VirtDef& v = virt_[X];
    if (!v.on) return;
    auto drop = [X](std::vector<int>& u) { u.erase(std::remove(u.begin(), u.end(), X), u.end()); };
    for (int s = 0; s < v.nSteps; s++) {
        const VirtStep& h = v.steps[s];
        if (h.tipA >= 0) drop(tipUsers_[h.tipA]);
        if (h.tipB >= 0) drop(tipUsers_[h.tipB]);
        if (h.scaleIdx >= 0) drop(scaleUsers_[h.scaleIdx]);
    }
    v.on = false;
    tagOf_[X] = -1; tagEpoch_++;
}

void WalkPlanner::registerVirtual(int X) {
    const VirtDef& v = virt_[X];
    auto add = [X](std::vector<int>& u) { if (std::find(u.begin(), u.end(), X) == u.end()) u.push_back(X); };
    for (int s = 0; s < v.nSteps; s++) {
        const VirtStep& h = v.steps[s];
        if (h.tipA >= 0) add(tipUsers_[h.tipA]);
        if (h.tipB >= 0) add(tipUsers_[h.tipB]);
        if (h.scaleIdx >= 0) add(scaleUsers_[h.scaleIdx]);
    }
}

// Try to define buffer X = node(child1 over matrix m1, child2 over matrix m2, scale).  Children are compact tips or
// virtual buffers.  Appends (source, destination) matrix-copy pairs.  false: too many steps, or its evaluation would need
// more hold slots than a definition may take.
bool WalkPlanner::buildVirtual(int X, int c1, bool tip1, bool mem1, int m1, int c2, bool tip2, bool mem2, int m2, int scaleIdx, std::vector<int>& snapPairs,
                               bool stored1, bool stored2) {
    // (tip1 / tip2: the child is a LEAF — compact states, or with mem1 / mem2 uploaded tip partials, or with stored1 / stored2 as well
    // a stored internal node: a memory definition, planner.h memStepCap — at most one such leaf in the whole definition)
    if (stored1 && stored2) return false;
    VirtDef nv;
    nv.on = true; nv.stamp = stamp_; nv.nSteps = 0; nv.chainOnly = true;
    std::vector<int>& pairs = pairScratch_;
    pairs.clear();
    const int maxNeed = popcount2(allSlots_) - 1;
    const int cap = stepCap();
    // copies the steps of srcBuf's definition behind what nv holds; returns the index of its last step, -1: no room
    auto append = [&](int srcBuf) -> int {
        const VirtDef& src = virt_[srcBuf];
        const int base = nv.nSteps;
        if (src.memKey >= 0) {
            if (nv.memKey >= 0) return -1;
            nv.memKey = src.memKey; nv.memStep = base + src.memStep;
        }
        for (int s = 0; s < src.nSteps; s++) {
            if (nv.nSteps >= cap) return -1;
            VirtStep h = src.steps[s];
            // a child defined in THIS list has its slots written by the same snapshot launch: copy from its origins
            const int fromA = src.stamp == stamp_ ? h.originA : snapSlot(srcBuf, s, 0);
            const int fromB = src.stamp == stamp_ ? h.originB : snapSlot(srcBuf, s, 1);
            h.originA = fromA; h.originB = fromB;
            if (h.subA >= 0) h.subA += base;
            if (h.subB >= 0) h.subB += base;
            pairs.push_back(fromA); pairs.push_back(snapSlot(X, nv.nSteps, 0));
            pairs.push_back(fromB); pairs.push_back(snapSlot(X, nv.nSteps, 1));
            nv.steps[nv.nSteps++] = h;
        }
        return nv.nSteps - 1;
    };
    VirtStep last;
    last.scaleIdx = scaleIdx; last.tipA = -1; last.tipB = -1; last.subA = -1; last.subB = -1; last.need = 0; last.memA = last.memB = false;
    if (tip1 && tip2) {
        last.type = VT_CHERRY; last.tipA = c1; last.tipB = c2; last.originA = m1; last.originB = m2; last.memA = mem1; last.memB = mem2;
        if (stored1 || stored2) { nv.memKey = stored1 ? c1 : c2; nv.memStep = 0; }
    } else if (tip1 != tip2) {
        const int vb = tip1 ? c2 : c1, t = tip1 ? c1 : c2, mv = tip1 ? m2 : m1, mt = tip1 ? m1 : m2;
        if (!virt_[vb].on) return false;
        const int r = append(vb);
        if (r < 0) return false;
        last.type = VT_EXTEND; last.subA = r; last.tipB = t; last.originA = mv; last.originB = mt; last.memB = tip1 ? mem1 : mem2;
        last.need = nv.steps[r].need;
        if (tip1 ? stored1 : stored2) {
            if (nv.memKey >= 0) return false;
            nv.memKey = t; nv.memStep = nv.nSteps;
        }
    } else {
        if (!virt_[c1].on || !virt_[c2].on) return false;
        const int ra = append(c1);
        if (ra < 0) return false;
        const int rb = append(c2);
        if (rb < 0) return false;
        last.type = VT_JOIN; last.subA = ra; last.subB = rb; last.originA = m1; last.originB = m2;
        const int na = nv.steps[ra].need, nb = nv.steps[rb].need;
        last.need = std::min(std::max(na, 1 + nb), std::max(nb, 1 + na));
        if (last.need > maxNeed) return false;
    }
    if (nv.nSteps >= (nv.memKey >= 0 ? std::min(cap, memCapNow_) : cap)) return false;
    pairs.push_back(last.originA); pairs.push_back(snapSlot(X, nv.nSteps, 0));
    pairs.push_back(last.originB); pairs.push_back(snapSlot(X, nv.nSteps, 1));
    nv.steps[nv.nSteps++] = last;
    nv.chainOnly = last.need == 0;
    virt_[X] = nv;
    tagOf_[X] = 0; tagEpoch_++;
    registerVirtual(X);
    snapPairs.insert(snapPairs.end(), pairs.begin(), pairs.end());
    return true;
}

bool WalkPlanner::defineCherry(int X, int tipA, int mA, int tipB, int mB, int scaleIdx, std::vector<int>& snapPairs) {
    if (!enabled_ || !compactTip[tipA] || !compactTip[tipB]) return false;
    stamp_++;
    if (virt_[X].on) clearVirtualKey(X);
    if (!buildVirtual(X, tipA, true, false, mA, tipB, true, false, mB, scaleIdx, snapPairs)) return false;
    VirtDef& nv = virt_[X];
    nv.version = ++virtVersion_;
    nv.sigC1 = tipA; nv.sigM1 = mA; nv.sigC2 = tipB; nv.sigM2 = mB; nv.sigScale = scaleIdx; nv.sigTip1 = nv.sigTip2 = true;
    return true;
}

int WalkPlanner::hazardFreePrefix(const int* ops, int begin, int count, int tuple, int parts) {
    const size_t nKeys = (size_t)partialsCount_ * parts, nS = (size_t)scaleCount_ * parts;
    if (wStamp_.size() < nKeys) { wStamp_.assign(nKeys, 0); rStamp_.assign(nKeys, 0); wOp_.assign(nKeys, 0); }
    if (sWStamp_.size() < nS) { sWStamp_.assign(nS, 0); sRStamp_.assign(nS, 0); sDone_.assign(nS, 0); }
    stamp_++;
    int k = begin;
    for (; k < count; k++) {
        const int* op = ops + (size_t)k * tuple;
        const int part = tuple > 7 ? op[7] : 0;
        // (the CALLER's partition count, which sized the marks above — plan() is what checks it against the planner's: not key())
        auto at = [&](int idx) { return (size_t)idx * parts + part; };
        const size_t kd = at(op[0]), k1 = at(op[3]), k2 = at(op[5]);
        bool hazard = wStamp_[kd] == stamp_ || rStamp_[kd] == stamp_;
        if (op[1] != OP_NONE) { const size_t s = at(op[1]); hazard = hazard || sWStamp_[s] == stamp_ || sRStamp_[s] == stamp_; }
        if (op[2] != OP_NONE && op[1] == OP_NONE) hazard = hazard || sWStamp_[at(op[2])] == stamp_;
        if (hazard && k > begin) break;
        rStamp_[k1] = stamp_; rStamp_[k2] = stamp_; wStamp_[kd] = stamp_;
        if (op[1] != OP_NONE) sWStamp_[at(op[1])] = stamp_;
        else if (op[2] != OP_NONE) sRStamp_[at(op[2])] = stamp_;
    }
    return k - begin;
}

void WalkPlanner::mustMaterializeBefore(const int* ops, int count, int tuple, std::vector<int>& out) {
    if (!enabled_) return;
    stamp_++;
    const size_t nKeys = (size_t)partialsCount_ * keyParts_;
    if (wStamp_.size() < nKeys) { wStamp_.assign(nKeys, 0); rStamp_.assign(nKeys, 0); wOp_.assign(nKeys, 0); }
    auto keyOf = [&](const int* op) { return key(op[0], tuple > 7 ? op[7] : 0); };
    for (int k = 0; k < count; k++) wStamp_[keyOf(ops + (size_t)k * tuple)] = stamp_;
    for (int k = 0; k < count; k++) {
        const int* op = ops + (size_t)k * tuple;
        if ((op[3] == op[0] || op[5] == op[0]) && virt_[keyOf(op)].on) out.push_back(keyOf(op));     // in-place update of a virtual buffer
        const int wS = op[1];
        if (wS == OP_NONE || wS < 0 || wS >= scaleCount_) continue;
        for (int u : scaleUsers_[wS])
            if (wStamp_[u] != stamp_) out.push_back(u);          // a destination of this list is redefined anyway
    }
    // memory definitions (planner.h memStepCap): a buffer keeps the value its operation gave it, so whatever reads a destination of
    // this list as its stored operand — and is not a destination itself — is evaluated from the OLD data first
    if (memStepCap > 0 && keyParts_ == 1)
        for (int k = 0; k < count; k++)
            for (int u : tipUsers_[ops[(size_t)k * tuple]])
                if (wStamp_[u] != stamp_) out.push_back(u);
}

void WalkPlanner::longMemoryOperands(const int* ops, int count, int tuple, int minSteps, std::vector<int>& out) {
    if (!enabled_ || memStepCap <= 0 || keyParts_ != 1 || minSteps >= memCapSeen()) return;
    stamp_++;
    const size_t nKeys = (size_t)partialsCount_;
    if (wStamp_.size() < nKeys) { wStamp_.assign(nKeys, 0); rStamp_.assign(nKeys, 0); wOp_.assign(nKeys, 0); }
    for (int k = 0; k < count; k++) wStamp_[(size_t)ops[(size_t)k * tuple]] = stamp_;
    for (int k = 0; k < count; k++) {
        const int* op = ops + (size_t)k * tuple;
        for (int c : {op[3], op[5]}) {
            const VirtDef& v = virt_[(size_t)c];
            // (a child this list writes is redefined by it; a definition whose stored operand the list writes is evaluated behind that
            // operand's program, or was given real data by mustMaterializeBefore)
            if (!v.on || v.memKey < 0 || v.nSteps <= minSteps || wStamp_[(size_t)c] == stamp_ || wStamp_[(size_t)v.memKey] == stamp_) continue;
            if (std::find(out.begin(), out.end(), c) == out.end()) out.push_back(c);
        }
    }
}

// ---- memory definitions (planner.h memStepCap) ---------------------------------------------------------------------
int WalkPlanner::operandOp(int vkey) const {
    const VirtDef& v = virt_[vkey];
    if (!v.on || v.memKey < 0 || wStamp_[v.memKey] != stamp_) return -1;
    const int a = wOp_[v.memKey];
    return info_[a].virtDest ? -1 : a;
}

bool WalkPlanner::onPath(const VirtDef& v, int idx) const {
    return walkMemPath(v, idx, [](int, int) {}) == idx;
}

// Steps memStep .. upTo of a memory definition evaluated where the program has just produced the stored operand (needA: the hold
// slots the operand's own evaluation takes): at every step of the path the costlier side first, parked while the other is evaluated.
int WalkPlanner::pathNeed(const VirtDef& v, int upTo, int needA) const {
    int n = needA;
    walkMemPath(v, upTo, [&](int, int off) {
        if (off >= 0) { const int b = v.steps[off].need; n = std::min(std::max(n, 1 + b), std::max(b, 1 + n)); }
    });
    return n;
}

// hold slots the evaluation of the real op k needs, and its size — children come earlier in the list
void WalkPlanner::realInfo(int k) {
    OpInfo& o = info_[k];
    int need[2] = {0, 0}, size[2] = {0, 0}; bool eval[2] = {false, false}, real[2] = {false, false};
    for (int w = 0; w < 2; w++) {
        const int c = o.ch[w].buf, prod = o.ch[w].prod;
        if (o.ch[w].tip) continue;
        if (prod >= 0 && !info_[prod].virtDest) { eval[w] = real[w] = true; need[w] = info_[prod].need; size[w] = info_[prod].size; }
        else if (virt_[key(c, o.part)].on) {
            const VirtDef& v = virt_[key(c, o.part)];
            const int a = operandOp(key(c, o.part));
            eval[w] = true;
            if (a >= 0) { need[w] = pathNeed(v, v.nSteps - 1, info_[a].need); size[w] = info_[a].size; }
            else need[w] = virtNeed(key(c, o.part));
        }
    }
    o.size = 1 + size[0] + size[1];
    if (eval[0] && eval[1]) {
        auto cost = [&](int a, int b) { return real[a] ? std::max(need[a], need[b]) : std::max(need[a], 1 + need[b]); };
        o.need = std::min(cost(0, 1), cost(1, 0));
    } else o.need = eval[0] ? need[0] : eval[1] ? need[1] : 0;
    if (allSlots_ == 0u) o.need = 0;            // no hold slots: the first of two evaluated children goes through memory
}

// ---- emission ----------------------------------------------------------------------------------------------------
namespace {
struct Child { int cls, buf, mat, prod, need, size, vkey, vstep; };      // vkey: definition key of (buf, the op's partition), vstep: the step of it to evaluate
inline MicroOp blankOp() {
    MicroOp m; m.storeBuf = PLAN_NONE; m.k1 = PK_MEM; m.a1 = 0; m.k2 = PK_MEM; m.a2 = 0; m.mat1 = 0; m.mat2 = 0;
    m.scaleIdx = PLAN_NONE; m.smode = PS_NONE; m.hold = 0;
    return m;
}
inline void setLeaf(MicroOp& m, int which, const Child& c) {
    const int kind = c.cls == CL_TIPS ? PK_TIPS : PK_MEM;
    if (which == 0) { m.k1 = kind; m.a1 = c.buf; m.mat1 = c.mat; } else { m.k2 = kind; m.a2 = c.buf; m.mat2 = c.mat; }
}
}  // namespace

void WalkPlanner::emitVirtualStep(int buf, int idx, unsigned freeMask, bool writeMode, Plan& out) {
    const VirtDef& v = virt_[buf];
    const VirtStep& st = v.steps[idx];
    MicroOp m = blankOp();
    if (st.type == VT_CHERRY) {
        // a leaf read from memory goes first (the kernels prefetch the first child's partials; kernels.h)
        const bool swap = st.memB && !st.memA;
        const int tA = swap ? st.tipB : st.tipA, tB = swap ? st.tipA : st.tipB;
        const bool mA = swap ? st.memB : st.memA, mB = swap ? st.memA : st.memB;
        m.k1 = mA ? PK_MEM : PK_TIPS; m.a1 = tA; m.mat1 = snapSlot(buf, idx, swap ? 1 : 0);
        m.k2 = mB ? PK_MEM : PK_TIPS; m.a2 = tB; m.mat2 = snapSlot(buf, idx, swap ? 0 : 1);
        lastMemReads += (mA ? 1 : 0) + (mB ? 1 : 0);
    } else if (st.type == VT_EXTEND) {
        emitVirtualStep(buf, st.subA, freeMask, writeMode, out);
        m.k1 = st.memB ? PK_MEM : PK_TIPS; m.a1 = st.tipB; m.mat1 = snapSlot(buf, idx, 1);
        m.k2 = PK_ACC; m.mat2 = snapSlot(buf, idx, 0);
        if (st.memB) lastMemReads++;
    } else {   // VT_JOIN: the operand that needs more hold slots first, parked while the other one is evaluated
        const int F = popcount2(freeMask);
        const int na = v.steps[st.subA].need, nb = v.steps[st.subB].need;
        const bool aOK = na <= F && 1 + nb <= F, bOK = nb <= F && 1 + na <= F;
        const bool aFirst = aOK && (!bOK || na >= nb);            // (one of them holds: need <= F by construction)
        const int first = aFirst ? st.subA : st.subB, second = aFirst ? st.subB : st.subA;
        emitVirtualStep(buf, first, freeMask, writeMode, out);
        const int h = lowestSlot(freeMask);
        out.prog.back().hold = h + 1;
        lastHolds++;
        emitVirtualStep(buf, second, freeMask & ~(1u << h), writeMode, out);
        m.k1 = PK_H0 + h; m.mat1 = snapSlot(buf, idx, aFirst ? 0 : 1);
        m.k2 = PK_ACC; m.mat2 = snapSlot(buf, idx, aFirst ? 1 : 0);
    }
    if (st.scaleIdx >= 0) {
        m.scaleIdx = st.scaleIdx;
        const size_t sk = scaleKey(st.scaleIdx, partitionOf(buf));      // scale-buffer use is tracked per partition
        const bool w = writeMode && sWStamp_[sk] == stamp_;
        m.smode = w ? PS_WRITE : PS_READ;
        if (w) sDone_[sk] = stamp_;
    }
    out.prog.push_back(m);
}

void WalkPlanner::emitVirtual(int buf, unsigned freeMask, bool writeMode, Plan& out) {
    emitVirtualStep(buf, virt_[buf].nSteps - 1, freeMask, writeMode, out);
}

// Emission of the real op `root` and everything below it that this walk evaluates.  Iterative (explicit frame stack on the
// heap): the dependency depth of an operation list is unbounded — a 5000-tip ladder tree is 4999 frames deep — and under
// BEAST this runs on a JVM thread whose native stack is 1 MiB or less (-Xss).
void WalkPlanner::emitReal(int root, unsigned rootMask, Plan& out) {
    // A frame is a real op of the list (j >= 0), or — a memory definition evaluated behind its operand's own program, planner.h memStepCap —
    // step pidx of definition pkey on the path from the stored operand to the definition's last step (j < 0): a node like any other,
    // whose children are the path below it (at step memStep: the operand's real op) and a tip or a plain part of the definition, whose
    // matrices are the definition's snapshots and whose result is not stored.
    struct Frame { int j, pkey, pidx; unsigned freeMask; int phase; Child ch[2]; int first; bool hold; MicroOp m; };
    std::vector<Frame> st;
    auto push = [&](int j, int pkey, int pidx, unsigned fm) { Frame f; f.j = j; f.pkey = pkey; f.pidx = pidx; f.freeMask = fm; f.phase = 0; f.first = 0; f.hold = false; f.m = blankOp(); st.push_back(f); };
    auto pushChild = [&](const Child& c, unsigned fm) { if (c.cls == CL_REAL) push(c.prod, -1, -1, fm); else push(-1, c.vkey, c.vstep, fm); };
    // (a definition evaluated inside this program: Plan::runs)
    auto emitRun = [&](const Child& c, unsigned fm) {
        const int s0 = (int)out.prog.size();
        emitVirtualStep(c.vkey, c.vstep, fm, true, out);
        out.runs.push_back(PlanRun{s0, (int)out.prog.size() - s0});
    };
    push(root, -1, -1, rootMask);
    while (!st.empty()) {
        const size_t top = st.size() - 1;                 // (a push invalidates references: every path that pushes `continue`s)
        if (st[top].phase == 0) {
            Frame& f = st[top];
            if (f.j >= 0) {
                const OpInfo& o = info_[f.j];
                for (int w = 0; w < 2; w++) {
                    Child& c = f.ch[w];
                    c.buf = o.ch[w].buf; c.mat = o.ch[w].mat;
                    c.prod = -1; c.need = 0; c.size = 0; c.vkey = key(c.buf, o.part); c.vstep = -1;
                    if (o.ch[w].tip) { c.cls = CL_TIPS; continue; }
                    const int prod = o.ch[w].prod;
                    bool virt = false;
                    if (prod >= 0) {
                        const OpInfo& p = info_[prod];
                        if (p.virtDest) virt = true;
                        else if (p.emitted) c.cls = CL_MEM;
                        else { c.cls = CL_REAL; c.prod = prod; c.need = p.need; c.size = p.size; }
                    } else if (virt_[c.vkey].on) virt = true;
                    else c.cls = CL_MEM;
                    if (virt) {
                        const VirtDef& v = virt_[c.vkey];
                        c.cls = CL_VIRT; c.need = virtNeed(c.vkey); c.vstep = v.nSteps - 1;
                        const int a = v.memKey >= 0 ? operandOp(c.vkey) : -1;
                        if (a >= 0 && !info_[a].emitted) { c.cls = CL_PATH; c.prod = a; c.need = pathNeed(v, c.vstep, info_[a].need); c.size = info_[a].size; }
                    }
                }
            } else {
                const VirtDef& v = virt_[f.pkey];
                const VirtStep& s = v.steps[f.pidx];
                const int a = operandOp(f.pkey);
                auto leaf = [&](Child& c, int buf, bool mem, int which) { c.cls = mem ? CL_MEM : CL_TIPS; c.buf = buf; c.mat = snapSlot(f.pkey, f.pidx, which); c.prod = -1; c.need = 0; c.size = 0; c.vkey = -1; c.vstep = -1; };
                auto operand = [&](Child& c, int which) { c.cls = CL_REAL; c.buf = v.memKey; c.mat = snapSlot(f.pkey, f.pidx, which); c.prod = a; c.need = info_[a].need; c.size = info_[a].size; c.vkey = -1; c.vstep = -1; };
                auto sub = [&](Child& c, int step, int which) {
                    c.buf = -1; c.mat = snapSlot(f.pkey, f.pidx, which); c.prod = -1; c.size = 0; c.vkey = f.pkey; c.vstep = step;
                    if (onPath(v, step)) { c.cls = CL_PATH; c.need = pathNeed(v, step, info_[a].need); c.size = info_[a].size; }
                    else { c.cls = CL_VIRT; c.need = v.steps[step].need; }
                };
                if (s.type == VT_CHERRY) {                // (the path's first step: the stored operand over a tip)
                    const bool opA = s.memA && s.tipA == v.memKey;
                    if (opA) { operand(f.ch[0], 0); leaf(f.ch[1], s.tipB, s.memB, 1); }
                    else { leaf(f.ch[0], s.tipA, s.memA, 0); operand(f.ch[1], 1); }
                } else if (s.type == VT_EXTEND) {
                    sub(f.ch[0], s.subA, 0);
                    if (f.pidx == v.memStep) operand(f.ch[1], 1); else leaf(f.ch[1], s.tipB, s.memB, 1);
                } else { sub(f.ch[0], s.subA, 0); sub(f.ch[1], s.subB, 1); }
            }
            const bool e0 = f.ch[0].cls >= CL_VIRT, e1 = f.ch[1].cls >= CL_VIRT;
            if (!e0 && !e1) {
                const int firstLeaf = (f.ch[0].cls == CL_TIPS && f.ch[1].cls == CL_MEM) ? 1 : 0;      // a child in memory goes first
                setLeaf(f.m, 0, f.ch[firstLeaf]); setLeaf(f.m, 1, f.ch[1 - firstLeaf]);
                if (f.ch[0].cls == CL_MEM) lastMemReads++;
                if (f.ch[1].cls == CL_MEM) lastMemReads++;
                f.phase = 9;
            } else if (e0 != e1) {
                const Child e = e0 ? f.ch[0] : f.ch[1];
                const Child l = e0 ? f.ch[1] : f.ch[0];
                setLeaf(f.m, 0, l);
                if (l.cls == CL_MEM) lastMemReads++;
                f.m.k2 = PK_ACC; f.m.mat2 = e.mat;
                f.phase = 9;
                if (e.cls == CL_VIRT) emitRun(e, f.freeMask);
                else { const unsigned fm = f.freeMask; pushChild(e, fm); continue; }
            } else {
                const int F = popcount2(f.freeMask);
                auto holdOK = [&](const Child& a, const Child& b) { return a.need <= F && 1 + b.need <= F; };
                auto plainOK = [&](const Child& a, const Child& b) { return a.cls == CL_REAL && f.j >= 0 && a.need <= F && b.need <= F; };
                const Child* ch = f.ch;
                const bool h01 = holdOK(ch[0], ch[1]), h10 = holdOK(ch[1], ch[0]);
                if (h01 || h10) {
                    f.hold = true;
                    if (h01 && h10) f.first = (ch[1].need > ch[0].need || (ch[1].need == ch[0].need && ch[1].size > ch[0].size)) ? 1 : 0;
                    else f.first = h01 ? 0 : 1;
                } else {
                    const bool p01 = plainOK(ch[0], ch[1]), p10 = plainOK(ch[1], ch[0]);
                    if (p01 && p10) f.first = ch[1].size > ch[0].size ? 1 : 0;
                    else if (p01 || p10) f.first = p01 ? 0 : 1;      // by construction one of them holds (planner.h: need <= 2) ...
                    // ... unless the walk has no hold slots (21..64 states): a real child first if there is one (it is stored anyway),
                    // otherwise a definition — evaluated and STORED for once (it stays a definition: the data is what it evaluates to)
                    else f.first = ch[0].cls == CL_REAL ? 0 : ch[1].cls == CL_REAL ? 1 : 0;
                }
                f.phase = 1;
                const Child a = ch[f.first];
                if (a.cls == CL_VIRT) emitRun(a, f.freeMask);
                else { const unsigned fm = f.freeMask; pushChild(a, fm); continue; }
            }
        }
        if (st[top].phase == 1) {                         // the first of two evaluated children is done
            Frame& f = st[top];
            const Child a = f.ch[f.first], b = f.ch[1 - f.first];
            unsigned mask2 = f.freeMask;
            if (f.hold) {
                const int h = lowestSlot(f.freeMask);
                out.prog.back().hold = h + 1;
                lastHolds++;
                mask2 = f.freeMask & ~(1u << h);
                f.m.k1 = PK_H0 + h; f.m.mat1 = a.mat;
            } else {
                if (a.cls != CL_REAL) { out.prog.back().storeBuf = a.buf; lastStored++; }      // (a definition, stored for once)
                f.m.k1 = PK_MEM; f.m.a1 = a.buf; f.m.mat1 = a.mat;
                lastMemReads++;
            }
            f.m.k2 = PK_ACC; f.m.mat2 = b.mat;
            f.phase = 9;
            if (b.cls == CL_VIRT) emitRun(b, mask2);
            else { pushChild(b, mask2); continue; }
        }
        {                                                 // phase 9: the node itself
            Frame& f = st[top];
            MicroOp& m = f.m;
            if (f.j >= 0) {
                OpInfo& o = info_[f.j];
                m.storeBuf = o.dest;
                if (o.wS != OP_NONE) { m.scaleIdx = o.wS; m.smode = PS_WRITE; sDone_[scaleKey(o.wS, o.part)] = stamp_; }
                else if (o.rS != OP_NONE) { m.scaleIdx = o.rS; m.smode = PS_READ; }
                o.emitted = true;
                lastStored++;
            } else {
                const VirtStep& s = virt_[f.pkey].steps[f.pidx];
                if (s.scaleIdx >= 0) {                    // (as emitVirtualStep)
                    m.scaleIdx = s.scaleIdx;
                    const size_t sk = scaleKey(s.scaleIdx, partitionOf(f.pkey));
                    const bool w = sWStamp_[sk] == stamp_;
                    m.smode = w ? PS_WRITE : PS_READ;
                    if (w) sDone_[sk] = stamp_;
                }
            }
            out.prog.push_back(m);
            st.pop_back();
        }
    }
}

// ---- plan(): the steps ---------------------------------------------------------------------------------------------
// What they hand each other is in ListState (planner.h) and in info_; the marks per buffer and scale buffer (wStamp_ / wOp_, sWStamp_,
// sDone_) are valid for the current stamp_ only.
int WalkPlanner::plan(const int* ops, int count, int tuple, int parts, bool allowVirtual, Plan& out, int chunkOps) {
    out.clear();
    planned = &out; plannedTag = 0;
    lastStored = lastMemReads = lastHolds = 0;
    memCapNow_ = memStepCap;
    if (count <= 0) return 0;
    parts_ = parts;
    const size_t nKeys = (size_t)partialsCount_ * parts, nS = (size_t)scaleCount_ * parts;
    if (wStamp_.size() < nKeys) { wStamp_.assign(nKeys, 0); rStamp_.assign(nKeys, 0); wOp_.assign(nKeys, 0); }
    if (sWStamp_.size() < nS) { sWStamp_.assign(nS, 0); sRStamp_.assign(nS, 0); sDone_.assign(nS, 0); }
    stamp_++;
    if (parts != keyParts_) return -1;                 // (BEAGLE_ERROR_GENERAL) the engine sets the partition count first
    ListState& L = list_;
    L.ops = ops; L.count = count; L.tuple = tuple; L.parts = parts; L.chunkOps = chunkOps; L.out = &out;
    L.allowVirtual = allowVirtual && enabled_;
    lastWeighed = 0;
    if (cacheStep(L)) return 0;                        // (replay() has set lastWeighed)
    definePass(L);
    if (L.anyMem) settleMemoryConsumers(L);
    // ---- pass 2: walk order.  One slice per partition; inside it, every unconsumed real op is a root of the forest.
    // With chunkOps > 0 the forest is peeled in waves: a wave = the maximal subtrees of at most chunkOps micro-operations
    // among what is left, one slice each; what is above them reads their (stored) roots in a later wave.
    listPartitions(L);
    // (planner.h repeatWeights: a closed list — one that is cached — of one partition in which nothing rescales)
    L.repeatW = repeatWeights && L.fill && parts == 1 && !L.anyRescale && L.allowVirtual;
    L.cutOps = chunkOps; L.cutTop = chunkTopOps; L.ruled = !L.repeatW;
    lastWaves = 0;
    for (int part : L.partsSeen) lastWaves = std::max(lastWaves, emitPartition(L, part));
    // launches run wave by wave: order the slices that way (stable: partitions keep their order inside a wave)
    std::stable_sort(out.segs.begin(), out.segs.end(), [](const PlanSeg& a, const PlanSeg& b) { return a.wave < b.wave; });
    linkSlices(out, L.repeatW ? (memDefTables ? 2 : 1) : 0);
    if (L.fill) fillCache(L);
    return 0;
}

// Cache step: closed list?  then the plan may be in the cache (planner.h CacheEntry).  Reads the list, the cache and the tips' flags.
// true: the plan was kept and has been replayed (planned, plannedTag and the statistics are the entry's) — plan() is done.  false: the
// list is to be planned, under memCapNow_ — raised to the longer cap here for a kept list's second coming (its entry is dropped) and
// for a new closed list under preferSeenCap; L.fill is the entry to put the plan into, its identity written, when the list is closed,
// L.anyRescale says whether it has a write-mode operation and L.simple is replayCached's `simple`.  Leaves no mark behind: stamp_ is
// moved past the ones its scan made.
bool WalkPlanner::cacheStep(ListState& L) {
    const int* ops = L.ops;
    const int count = L.count, tuple = L.tuple;
    L.fill = nullptr; L.anyRescale = false; L.simple = false;
    if (count < 16) return false;
    int promoteWay = -1;
    if (CacheEntry* hit = findCached(ops, count, tuple, L.parts, L.allowVirtual, L.chunkOps)) {
        if (!promotable(*hit, L.allowVirtual)) {
            if (cacheEnabled) {
                stamp_++;
                replay(*hit, ops);
                cacheHits++;
                return true;
            }
            // cacheEnabled off: nothing is replayed — the list is planned from scratch under the cap its entry was planned under, into the
            // way it had.  It stays a KEPT plan (a tag): what the engine does to kept plans only (folded reciprocals, class tables) does
            // not depend on the switch, and neither does a bit of the results
            hit->valid = false;
            if (L.allowVirtual && hit->memStepCap > 0) memCapNow_ = hit->memStepCap;
            promoteWay = (int)(hit - cache_);
        } else {
            hit->valid = false;                    // the list's second coming: planned again under the longer cap (planner.h memStepCapSeen),
            memCapNow_ = memCapSeen();             // into the way it had: no other kept plan is evicted for it
            promoteWay = (int)(hit - cache_);
        }
    }
    bool closed = true, simple = true;
    for (int k = 0; k < count && closed; k++) {
        const int* op = ops + (size_t)k * tuple;
        const int part = tuple > 7 ? op[7] : 0;
        if (op[1] != OP_NONE) L.anyRescale = true;
        if (!compactTip[op[3]] && wStamp_[key(op[3], part)] != stamp_) closed = false;
        if (!compactTip[op[5]] && wStamp_[key(op[5], part)] != stamp_) closed = false;
        wStamp_[key(op[0], part)] = stamp_;
        if (op[1] != OP_NONE || op[0] == op[3] || op[0] == op[5] || (compactTip[op[0]] || leafPartials[op[0]]) ||
            (tuple > 7 && op[8] != OP_NONE)) simple = false;
    }
    stamp_++;                                      // the marks above must not look like producers to pass 1
    if (!closed) return false;
    if (preferSeenCap) memCapNow_ = memCapSeen();
    // (a way's tags are 8 g + way + 1, g counted per way: unique, and the tags of the eight ways differ in their low three bits,
    // which is how the engine finds the program it keeps for a plan — engine_walk.cpp runPlan)
    const int way = promoteWay >= 0 ? promoteWay : cacheNext_;
    if (promoteWay < 0) cacheNext_ = (cacheNext_ + 1) % CACHE_WAYS;
    CacheEntry* fill = &cache_[way];
    fill->valid = false; fill->cleanAtEpoch = -1; fill->tag = ++wayGen_[way] * CACHE_WAYS + way + 1; fill->count = count; fill->tuple = tuple; fill->parts = L.parts; fill->chunkOps = L.chunkOps; fill->repeatWeights = repeatWeights; fill->memDefTables = memDefTables;
    fill->allowVirtual = L.allowVirtual; fill->stepLimit = L.allowVirtual ? stepLimit : 0; fill->memStepCap = L.allowVirtual ? memCapNow_ : 0; fill->tipEpoch = compactEpoch; fill->simple = simple;
    fill->ops.assign(ops, ops + (size_t)count * tuple);
    L.fill = fill; L.simple = simple;
    return false;
}

// Pass 1, list order: virtual definitions, producers, hold needs.  Reads the list and the definitions the planner holds; leaves info_
// complete for every op (Operand::prod, virtDest, and need / size of the real ones), the definitions of this list's destinations made,
// re-confirmed or dropped (their snapshot copies in out.snapPairs), wStamp_ / wOp_ naming the op that writes each key and sWStamp_
// the scale buffers written, L.consumed and L.anyMem.
void WalkPlanner::definePass(ListState& L) {
    info_.assign(L.count, OpInfo());
    L.consumed.assign(L.count, 0);
    L.memDefs = L.allowVirtual && memDefsOn(L.parts);
    L.anyMem = false;
    for (int k = 0; k < L.count; k++) {
        if (k + 6 < L.count) {                             // (a definition is 1.5 KB: the destination's two lines that matter, a few operations ahead)
            const int* ahead = L.ops + (size_t)(k + 6) * L.tuple;
            const char* a = reinterpret_cast<const char*>(&virt_[key(ahead[0], L.tuple > 7 ? ahead[7] : 0)]);
            __builtin_prefetch(a, 1); __builtin_prefetch(a + 64, 1);
        }
        defineOp(L, k);
    }
}

// The signature of a definition — the op that made it, as far as it decides what the definition is: children, matrices, scale buffer,
// which children are leaves and which of those are read from memory, and the version of a child that is a definition itself.
// definitionStands reads what signDefinition wrote: the steady state — the same op on the same buffers as when `dest` was last defined,
// its virtual children unchanged (same definition version) and re-confirmed in this list exactly as they were fresh then -> the
// definition stands; only its matrix snapshots are refreshed.  Anything else rebuilds it.  (stored: the child is a stored internal node
// read as a leaf — a memory definition, which is rebuilt every time.)
bool WalkPlanner::definitionStands(const VirtDef& ev, const OpInfo& o, int ownScale, const bool stored[2]) const {
    const Operand &a = o.ch[0], &b = o.ch[1];
    auto childSame = [&](const Operand& c, bool sigTip, int ver, bool fresh) {
        if (c.leaf != sigTip) return false;
        if (c.leaf) return true;
        const VirtDef& cv = virt_[key(c.buf, o.part)];
        return fresh && cv.stamp == stamp_ && cv.version == ver;
    };
    return ev.on && ev.memKey < 0 && !stored[0] && !stored[1] && ev.nSteps <= stepCap() &&
           ev.sigC1 == a.buf && ev.sigM1 == a.mat && ev.sigC2 == b.buf && ev.sigM2 == b.mat && ev.sigScale == ownScale &&
           ev.sigMem1 == (a.leaf && !a.tip) && ev.sigMem2 == (b.leaf && !b.tip) &&
           childSame(a, ev.sigTip1, ev.childVer1, ev.fresh1) && childSame(b, ev.sigTip2, ev.childVer2, ev.fresh2);
}

void WalkPlanner::signDefinition(VirtDef& nv, const OpInfo& o, int ownScale, const bool stored[2]) {
    const Operand &a = o.ch[0], &b = o.ch[1];
    const VirtDef &va = virt_[key(a.buf, o.part)], &vb = virt_[key(b.buf, o.part)];
    nv.version = ++virtVersion_;
    nv.sigC1 = a.buf; nv.sigM1 = a.mat; nv.sigC2 = b.buf; nv.sigM2 = b.mat; nv.sigScale = ownScale;
    nv.sigTip1 = a.leaf || stored[0]; nv.sigTip2 = b.leaf || stored[1];
    nv.sigMem1 = (a.leaf && !a.tip) || stored[0]; nv.sigMem2 = (b.leaf && !b.tip) || stored[1];
    nv.fresh1 = !nv.sigTip1 && va.stamp == stamp_; nv.fresh2 = !nv.sigTip2 && vb.stamp == stamp_;
    nv.childVer1 = nv.sigTip1 ? -1 : va.version; nv.childVer2 = nv.sigTip2 ? -1 : vb.version;
}

// Pass 1 for op k (its children are earlier ops of the list, or come from outside it): fills info_[k], marks the ops that produce its
// children as consumed, and decides whether its destination is a definition (re-confirmed, or built) or real data; a real one gets its
// hold need and size.
void WalkPlanner::defineOp(ListState& L, int k) {
    const int* op = L.ops + (size_t)k * L.tuple;
    Plan& out = *L.out;
    OpInfo& o = info_[k];
    o.dest = op[0]; o.wS = op[1]; o.rS = op[2];
    o.part = L.tuple > 7 ? op[7] : 0;
    o.virtDest = false; o.emitted = false; o.need = 0; o.size = 1;
    const int kd = key(o.dest, o.part);
    int kc[2];
    for (int w = 0; w < 2; w++) {
        Operand& c = o.ch[w];
        c.buf = op[3 + 2 * w]; c.mat = op[4 + 2 * w];
        c.tip = compactTip[c.buf] != 0; c.leaf = c.tip || leafPartials[c.buf] != 0;
        kc[w] = key(c.buf, o.part);
        c.prod = -1;
        if (!c.tip && wStamp_[kc[w]] == stamp_) { c.prod = wOp_[kc[w]]; L.consumed[c.prod] = 1; }
    }
    if (o.wS != OP_NONE) sWStamp_[scaleKey(o.wS, o.part)] = stamp_;

    const int ownScale = o.wS != OP_NONE ? o.wS : o.rS;
    bool makeVirtual = false;
    // (memory definitions: ONE child may be a stored internal node, or a definition that reads one — planner.h memStepCap)
    bool virt[2], stored[2], asLeaf[2];
    for (int w = 0; w < 2; w++) {
        virt[w] = !o.ch[w].leaf && virt_[kc[w]].on;
        stored[w] = L.memDefs && !o.ch[w].leaf && !virt[w];
        asLeaf[w] = o.ch[w].leaf || stored[w];
    }
    if (L.allowVirtual && (asLeaf[0] || virt[0]) && (asLeaf[1] || virt[1]) && !(stored[0] && stored[1]) && o.ch[0].buf != o.dest && o.ch[1].buf != o.dest) {
        VirtDef& ev = virt_[kd];
        if (definitionStands(ev, o, ownScale, stored)) {
            for (int st = 0; st < ev.nSteps; st++) {
                out.snapPairs.push_back(ev.steps[st].originA); out.snapPairs.push_back(snapSlot(kd, st, 0));
                out.snapPairs.push_back(ev.steps[st].originB); out.snapPairs.push_back(snapSlot(kd, st, 1));
            }
            ev.stamp = stamp_;
            makeVirtual = true;
        } else {
            VirtDef saved = ev;
            if (saved.on) clearVirtualKey(kd);
            const Operand &a = o.ch[0], &b = o.ch[1];
            makeVirtual = buildVirtual(kd, asLeaf[0] ? a.buf : kc[0], asLeaf[0], (a.leaf && !a.tip) || stored[0], a.mat,
                                       asLeaf[1] ? b.buf : kc[1], asLeaf[1], (b.leaf && !b.tip) || stored[1], b.mat, ownScale, out.snapPairs, stored[0], stored[1]);
            if (!makeVirtual && saved.on) { virt_[kd] = saved; tagOf_[kd] = saved.cacheTag; tagEpoch_++; registerVirtual(kd); }
            if (makeVirtual) signDefinition(virt_[kd], o, ownScale, stored);
        }
    }
    if (!makeVirtual && virt_[kd].on) clearVirtualKey(kd);      // whatever it was, this op replaces it
    o.virtDest = makeVirtual;
    wStamp_[kd] = stamp_; wOp_[kd] = k;

    if (makeVirtual && virt_[kd].memKey >= 0) L.anyMem = true;
    if (!makeVirtual) {
        realInfo(k);
        // two memory definitions, each behind its own operand's program, can take a hold slot more than the walk has: store them
        if (L.memDefs && o.need > popcount2(allSlots_)) {
            for (int w = 0; w < 2; w++) {
                if (o.ch[w].tip || operandOp(kc[w]) < 0 || wStamp_[kc[w]] != stamp_) continue;
                const int x = wOp_[kc[w]];
                clearVirtualKey(kc[w]);
                info_[x].virtDest = false;
                realInfo(x);
            }
            realInfo(k);
        }
    }
}

// Backward settlement of who consumes a memory definition (only when pass 1 made one).
// Memory definitions: who consumes whom is settled backwards — a definition nothing in this list evaluates is stored after all (the
// root of a tree: whoever reads it would otherwise evaluate it from memory in a launch of its own), and a stored operand is
// consumed by a definition only where that definition is evaluated.  Reads info_ and the definitions; leaves L.consumed rebuilt,
// and the unevaluated memory definitions dropped, their ops real (need / size set).
void WalkPlanner::settleMemoryConsumers(ListState& L) {
    const int count = L.count;
    std::vector<char>& consumed = L.consumed;
    std::fill(consumed.begin(), consumed.end(), 0);
    std::vector<char> live(count, 0), absorbed(count, 0);      // evaluated by a real op of the list; its steps stand in a longer definition
    for (int k = count - 1; k >= 0; k--) {
        OpInfo& o = info_[k];
        const int kd = key(o.dest, o.part);
        if (o.virtDest && virt_[kd].memKey >= 0 && !live[k] && !absorbed[k]) { clearVirtualKey(kd); o.virtDest = false; realInfo(k); }
        if (o.virtDest) {
            const int a = live[k] ? operandOp(kd) : -1;
            if (a >= 0) consumed[a] = 1;
            for (int w = 0; w < 2; w++) {
                const int prod = o.ch[w].prod;
                if (prod >= 0 && info_[prod].virtDest) absorbed[prod] = 1;
            }
            continue;
        }
        for (int w = 0; w < 2; w++) {
            const int prod = o.ch[w].prod;
            if (prod < 0) continue;
            if (info_[prod].virtDest) live[prod] = 1; else consumed[prod] = 1;
        }
    }
}

// The partitions the list names, in the order of their first operation: L.partsSeen.
void WalkPlanner::listPartitions(ListState& L) {
    L.partsSeen.clear();
    std::vector<char> seen(L.parts, 0);
    for (int k = 0; k < L.count; k++) if (!seen[info_[k].part]) { seen[info_[k].part] = 1; L.partsSeen.push_back(info_[k].part); }
}

// Pass 2 for one partition: wave after wave peeled off while what is left weighs more than a chunk and a half, then the remainder as
// one slice.  Reads info_, L.consumed and the cut (L.cutOps / cutTop / ruled); appends the partition's slices (progStart, progCount,
// partition, wave) and their micro-operations to the plan, marks the ops emitted, and returns the number of waves.  The first weighing
// of a list that is weighed for compression settles lastWeighed and the cut (planner.h repeatChunkRule).
int WalkPlanner::emitPartition(ListState& L, int part) {
    int wave = 0;
    for (;;) {
        int chunk = (wave == 0 || L.cutTop <= 0) ? L.cutOps : std::min(L.cutOps, L.cutTop);
        if (chunk > 0 || !L.ruled) {
            const long total = weighPartition(L, part);
            if (!L.ruled) {                              // the whole plan's weight is known: the slice sizes that go with it
                L.ruled = true;
                lastWeighed = total;
                if (repeatChunkRule) repeatChunkRule(total, L.cutOps, L.cutTop);
                chunk = L.cutOps;
            }
            if (chunk > 0 && total > chunk + chunk / 2 && peelWave(L, part, chunk, wave)) { wave++; continue; }
        }
        if (emitRemainder(L, part, wave)) wave++;
        return wave;
    }
}

// Weighs what is left of a partition: L.weight[k] = micro-operations below every op that is still to be emitted (children precede
// parents in the list; 0 for the others), under L.repeatW with definitions counted as what compression leaves of them.  Returns the sum
// over the roots (the ops nothing consumes).  Reads info_, L.consumed, the definitions.
long WalkPlanner::weighPartition(ListState& L, int part) {
    std::vector<int>& weight = L.weight;
    weight.assign(L.count, 0);
    long total = 0;
    for (int k = 0; k < L.count; k++) {
        const OpInfo& o = info_[k];
        if (o.part != part || o.virtDest || o.emitted) continue;
        int w = 1;
        for (int c = 0; c < 2; c++) {
            const int prod = o.ch[c].prod;
            if (o.ch[c].tip) continue;
            if (prod >= 0 && !info_[prod].virtDest) { if (!info_[prod].emitted) w += weight[prod]; continue; }
            const int ck = key(o.ch[c].buf, o.part);
            const VirtDef& v = virt_[ck];
            if (!v.on) continue;
            if (L.repeatW && plainDefinition(v)) { w += 1; continue; }      // (a table row gathered by this op)
            // (a memory definition under memDefTables: its path, and a gather per plain clade off it)
            w += L.repeatW && memDefTables && v.memKey >= 0 ? memDefWeight(v) : v.nSteps;
            const int a = L.anyMem ? operandOp(ck) : -1;      // (a memory definition: its operand's program comes with it)
            if (a >= 0 && !info_[a].emitted) w += weight[a];
        }
        weight[k] = w;
        if (!L.consumed[k]) total += w;
    }
    return total;
}

// Peels one wave: the maximal subtrees of at most `chunk` micro-operations (L.weight) among what is left of the partition, one slice
// each.  false, and nothing emitted: fewer than two such subtrees.  Reads info_, L.weight, L.consumed.
bool WalkPlanner::peelWave(ListState& L, int part, int chunk, int wave) {
    Plan& out = *L.out;
    std::vector<int>&chunkRoots = L.chunkRoots, &stack = L.stack;
    chunkRoots.clear(); stack.clear();
    for (int k = L.count - 1; k >= 0; k--) {
        const OpInfo& o = info_[k];
        if (o.part == part && !o.virtDest && !o.emitted && !L.consumed[k]) stack.push_back(k);
    }
    while (!stack.empty()) {
        const int k = stack.back(); stack.pop_back();
        if (L.weight[k] <= chunk) { chunkRoots.push_back(k); continue; }
        bool descended = false;
        for (int c = 1; c >= 0; c--) {
            const Operand& ch = info_[k].ch[c];
            int prod = ch.prod;
            if (L.anyMem && !ch.tip && (prod < 0 || info_[prod].virtDest)) prod = operandOp(key(ch.buf, part));
            if (prod >= 0 && !info_[prod].virtDest && !info_[prod].emitted) { stack.push_back(prod); descended = true; }
        }
        if (!descended) chunkRoots.push_back(k);      // heavier than a chunk but nothing below is left to peel
    }
    // a DAG may reach the same op twice: emit once
    std::sort(chunkRoots.begin(), chunkRoots.end());
    chunkRoots.erase(std::unique(chunkRoots.begin(), chunkRoots.end()), chunkRoots.end());
    // only worth a wave of its own when it really runs side by side
    if (chunkRoots.size() < 2) return false;
    for (int k : chunkRoots) {
        if (info_[k].emitted) continue;
        PlanSeg seg; seg.progStart = (int)out.prog.size(); seg.partition = part; seg.wave = wave;
        emitReal(k, allSlots_, out);
        seg.progCount = (int)out.prog.size() - seg.progStart;
        out.segs.push_back(seg);
    }
    return true;
}

// Emits what is left of the partition as one slice of wave `wave`: every root, and the write-mode leftovers.  false: nothing was left
// (no slice is added).  Reads info_, L.consumed, sDone_.
bool WalkPlanner::emitRemainder(ListState& L, int part, int wave) {
    Plan& out = *L.out;
    PlanSeg seg; seg.progStart = (int)out.prog.size(); seg.partition = part; seg.wave = wave;
    for (int k = 0; k < L.count; k++) {
        const OpInfo& o = info_[k];
        if (o.part != part || o.virtDest || o.emitted) continue;
        if (!L.consumed[k]) emitReal(k, allSlots_, out);
    }
    // virtual nodes of a rescaling evaluation still owe their scale factors if nothing above evaluated them
    for (int k = 0; k < L.count; k++) {
        const OpInfo& o = info_[k];
        if (o.part != part || !o.virtDest || o.wS == OP_NONE) continue;
        if (sDone_[scaleKey(o.wS, o.part)] != stamp_) emitVirtual(key(o.dest, o.part), allSlots_, true, out);
    }
    seg.progCount = (int)out.prog.size() - seg.progStart;
    if (seg.progCount > 0) out.segs.push_back(seg);
    return seg.progCount > 0;
}

// The cache fill: the finished plan goes into L.fill.
// (the entry TAKES the program — `out` is left with whatever the entry held — and `planned` names the entry's copy, as on
// a hit; the definitions of unstored destinations are copied, steps in use only, over whatever the way held before)
void WalkPlanner::fillCache(ListState& L) {
    CacheEntry* fill = L.fill;
    Plan& out = *L.out;
    const int count = L.count;
    fill->plan.clear();
    fill->plan.prog.swap(out.prog); fill->plan.segs.swap(out.segs); fill->plan.deps.swap(out.deps);
    fill->plan.launchOrder.swap(out.launchOrder); fill->plan.snapPairs.swap(out.snapPairs); fill->plan.runs.swap(out.runs); fill->plan.leaves = out.leaves;
    planned = &fill->plan;
    if ((int)fill->defs.size() < count) fill->defs.resize(count);
    fill->defOn.assign(count, 0);
    for (int k = 0; k < count; k++)
        if (info_[k].virtDest) { const int kk = key(info_[k].dest, info_[k].part); virt_[kk].cacheTag = fill->tag; tagOf_[kk] = fill->tag; tagEpoch_++; fill->defs[k] = virt_[kk]; fill->defOn[k] = 1; }
    plannedTag = fill->tag;
    fill->stored = lastStored; fill->memReads = lastMemReads; fill->holds = lastHolds; fill->waves = lastWaves; fill->weighed = lastWeighed;
    fill->valid = true;
}

bool WalkPlanner::plainDefinition(const VirtDef& v) const {
    if (v.memKey >= 0) return false;
    for (int s = 0; s < v.nSteps; s++) if (v.steps[s].memA || v.steps[s].memB) return false;
    return v.nSteps > 0;
}

// (planner.h memDefTables) what compression leaves of a memory definition: the steps from memStep up to the last one, and off that path a
// clade of compact tips as the one gather it becomes, anything else — a clade over uploaded tip partials — as its steps
int WalkPlanner::memDefWeight(const VirtDef& v) const {
    int size[PLAN_MAX_STEPS]; bool plain[PLAN_MAX_STEPS];       // per step: its subtree (operands are earlier steps)
    for (int t = 0; t < v.nSteps; t++) {
        const VirtStep& s = v.steps[t];
        if (s.type == VT_CHERRY) { size[t] = 1; plain[t] = !s.memA && !s.memB; }
        else if (s.type == VT_EXTEND) { size[t] = 1 + size[s.subA]; plain[t] = plain[s.subA] && !s.memB; }
        else { size[t] = 1 + size[s.subA] + size[s.subB]; plain[t] = plain[s.subA] && plain[s.subB]; }
    }
    auto off = [&](int sub) { return plain[sub] ? 1 : size[sub]; };
    int w = 0;
    walkMemPath(v, v.nSteps - 1, [&](int, int sub) { w += 1 + (sub >= 0 ? off(sub) : 0); });
    return w;
}

namespace {
// The maximal plain sub-clades of micro-operations [start, start + count) of one run (planner.h RepeatRun): ranges [first, root] in which
// every micro-operation stores nothing, pays nothing (`pays`) and reads tips, the ACC of its predecessor in the range or a hold slot parked
// in the range, and whose result is read by a micro-operation of the run that is not such a one itself.  In program order.
template <class Pays> void plainSubRanges(const std::vector<MicroOp>& prog, int start, int count, Pays pays, std::vector<PlanRun>& out) {
    std::vector<int> first((size_t)count, -1);            // per micro-operation: where its plain sub-clade begins, -1: it heads none
    int parked[3] = {-1, -1, -1};
    auto at = [&](int i) -> int& { return first[(size_t)(i - start)]; };
    for (int i = start; i < start + count; i++) {
        const MicroOp& m = prog[(size_t)i];
        bool ok = m.storeBuf < 0 && !pays(i);
        int f = i, h = -1;
        if (isHoldKind(m.k1)) { h = parked[m.k1 - PK_H0]; parked[m.k1 - PK_H0] = -1; if (h < 0 || at(h) < 0) ok = false; }
        else if (m.k1 != PK_TIPS) ok = false;
        if (m.k2 == PK_ACC) {
            // (post-order: the operand in ACC ends right before this one, a parked operand right before that one's range)
            if (i == start || at(i - 1) < 0 || prog[(size_t)i - 1].hold) ok = false;
            else if (h >= 0 && ok && at(i - 1) != h + 1) ok = false;
            else f = h >= 0 && ok ? at(h) : at(i - 1);
        } else if (m.k2 != PK_TIPS || h >= 0) ok = false;
        at(i) = ok ? f : -1;
        if (m.hold) parked[m.hold - 1] = i;
    }
    for (int i = start; i < start + count; i++) {
        if (at(i) < 0) continue;
        const MicroOp& m = prog[(size_t)i];
        int j = -1;
        if (m.hold) { for (int q = i + 1; q < start + count; q++) if (prog[(size_t)q].k1 == PK_H0 + m.hold - 1) { j = q; break; } }
        else if (i + 1 < start + count && prog[(size_t)i + 1].k2 == PK_ACC) j = i + 1;
        if (j >= 0 && at(j) < 0) out.push_back(PlanRun{at(i), i - at(i) + 1});
    }
}
}  // namespace

// Which slices read what other slices of the same plan store (planner.h PlanSeg): a slice reads a stored result only as a
// PK_MEM operand, and only of a slice of an EARLIER wave of the same partition (tests/native/plan_check.cpp checks both).
// Reads prog and the slices' ranges; leaves every slice's depStart / depCount and Plan::deps.
void WalkPlanner::linkDependencies(Plan& out) {
    const size_t nKeys = (size_t)partialsCount_ * keyParts_;
    if (storedBy_.size() < nKeys) { storedBy_.assign(nKeys, -1); storedStamp_.assign(nKeys, 0); }
    linkStamp_++;
    const int n = (int)out.segs.size();
    for (int s = 0; s < n; s++) {
        const PlanSeg& sg = out.segs[s];
        for (int k = sg.progStart; k < sg.progStart + sg.progCount; k++) {
            const int st = out.prog[k].storeBuf;
            if (st >= 0) { const size_t kk = (size_t)key(st, sg.partition); storedBy_[kk] = s; storedStamp_[kk] = linkStamp_; }
        }
    }
    out.deps.clear();
    std::vector<int> mark(n, -1);
    for (int s = 0; s < n; s++) {
        PlanSeg& sg = out.segs[s];
        sg.depStart = (int)out.deps.size();
        auto reads = [&](int kind, int buf) {
            if (kind != PK_MEM) return;
            const size_t kk = (size_t)key(buf, sg.partition);
            if (kk >= nKeys || storedStamp_[kk] != linkStamp_) return;
            const int by = storedBy_[kk];
            if (by == s || mark[by] == s) return;
            mark[by] = s;
            out.deps.push_back(by);
        };
        for (int k = sg.progStart; k < sg.progStart + sg.progCount; k++) { reads(out.prog[k].k1, out.prog[k].a1); reads(out.prog[k].k2, out.prog[k].a2); }
        sg.depCount = (int)out.deps.size() - sg.depStart;
    }
}

namespace {
// tickets (planner.h PlanSeg::next): does every slice have at most one dependant?  Reads the dependencies; leaves every slice's
// `next` and Plan::leaves (0: no forest, or an empty slice).
void ticketForest(Plan& out) {
    const int n = (int)out.segs.size();
    std::vector<int> dependants(n, 0);
    for (int s = 0; s < n; s++) out.segs[s].next = -1;
    for (int s = 0; s < n; s++)
        for (int d = out.segs[s].depStart; d < out.segs[s].depStart + out.segs[s].depCount; d++) { dependants[out.deps[d]]++; out.segs[out.deps[d]].next = s; }
    bool forest = n > 0;
    int leaves = 0;
    for (int s = 0; s < n; s++) {
        if (dependants[s] > 1 || out.segs[s].progCount <= 0) forest = false;
        if (out.segs[s].depCount == 0) leaves++;
    }
    out.leaves = forest ? leaves : 0;
}

// tail: own length + the longest tail among the slices that wait for this one.  Slices are sorted by wave and read only
// earlier waves, so one backward sweep settles every slice before the ones it reads.  Leaves every slice's tail and the plain launch
// order: descending tail.
void sliceTails(Plan& out) {
    const int n = (int)out.segs.size();
    for (int s = 0; s < n; s++) out.segs[s].tail = 0;
    for (int s = n - 1; s >= 0; s--) {
        PlanSeg& sg = out.segs[s];
        sg.tail += sg.progCount;
        for (int d = sg.depStart; d < sg.depStart + sg.depCount; d++) {
            PlanSeg& child = out.segs[out.deps[d]];
            child.tail = std::max(child.tail, sg.tail);
        }
    }
    out.launchOrder.resize(n);
    for (int s = 0; s < n; s++) out.launchOrder[s] = s;
    std::stable_sort(out.launchOrder.begin(), out.launchOrder.end(), [&](int a, int b) { return out.segs[a].tail > out.segs[b].tail; });
}

// A run that the slice DURATIONS count as one gather: more than one micro-operation, none of which stores or reads memory.  Not
// tableCandidate of findRepeatRuns, which decides what the engine really takes from a class table: that one also asks that no
// micro-operation of the range PAYS reciprocals, that every tip is a compact one the index knows, that the result has a consumer in the
// slice and that the clade is within the class limit.  Who pays is known only once the engine has folded the plan (foldScaleFactors runs
// on the finished plan, engine_walk.cpp), the index only with the alignment — the schedule is simulated before either, so the
// durations ignore them: an estimate that can count a run the engine then leaves in the walk.  Do not merge the two.
bool gatherRun(const std::vector<MicroOp>& prog, const PlanRun& run) {
    bool plain = run.count > 1;
    for (int i = run.start; plain && i < run.start + run.count; i++) {
        const MicroOp& m = prog[(size_t)i];
        plain = m.storeBuf < 0 && m.k1 != PK_MEM && m.k2 != PK_MEM;
    }
    return plain;
}

// how long a slice runs: its micro-operations — under planner.h repeatWeights with every run that reads tips only counted as the one
// gather it becomes, and (2: planner.h memDefTables) inside any other run every plain sub-clade the same way
std::vector<int> sliceDurations(const Plan& out, int repeatDurations) {
    const int n = (int)out.segs.size();
    std::vector<int> duration(n);
    for (int s = 0; s < n; s++) duration[s] = out.segs[s].progCount;
    if (!repeatDurations) return duration;
    std::vector<PlanRun> sub;
    for (const PlanRun& run : out.runs) {
        const bool plain = gatherRun(out.prog, run);
        int saved = plain ? run.count - 1 : 0;
        if (!plain && repeatDurations > 1 && run.count > 1) {
            sub.clear();
            plainSubRanges(out.prog, run.start, run.count, [](int) { return false; }, sub);
            for (const PlanRun& q : sub) saved += q.count - 1;
        }
        if (saved <= 0) continue;
        const int s = sliceHolding(out, run.start);
        if (s >= 0) duration[s] -= saved;
    }
    return duration;
}

// List scheduling on `machines` identical machines, a slice taking its duration: whenever a machine is free, the ready slice
// (all of its dependencies finished) with the longest tail starts; the order of the starts is the launch order.  Reads the
// dependencies, tails and the descending-tail order; replaces Plan::launchOrder.
void scheduleLaunchOrder(Plan& out, const std::vector<int>& duration, int machines) {
    const int n = (int)out.segs.size();
    std::vector<int> waiting(n, 0);                       // unfinished dependencies
    std::vector<std::vector<int>> dependants(n);
    for (int s = 0; s < n; s++) {
        waiting[s] = out.segs[s].depCount;
        for (int d = out.segs[s].depStart; d < out.segs[s].depStart + out.segs[s].depCount; d++) dependants[out.deps[d]].push_back(s);
    }
    std::vector<long> freeAt(machines, 0);
    std::vector<std::pair<long, int>> running;            // (finish time, slice)
    std::vector<int> ready;
    for (int s : out.launchOrder) if (waiting[s] == 0) ready.push_back(s);      // (kept in descending-tail order)
    std::vector<int> order;
    order.reserve(n);
    auto retire = [&](long now) {
        for (size_t i = 0; i < running.size();) {
            if (running[i].first > now) { i++; continue; }
            for (int c : dependants[running[i].second])
                if (--waiting[c] == 0) {
                    const auto at = std::upper_bound(ready.begin(), ready.end(), c, [&](int a, int b) { return out.segs[a].tail > out.segs[b].tail; });
                    ready.insert(at, c);
                }
            running[i] = running.back(); running.pop_back();
        }
    };
    while ((int)order.size() < n) {
        const size_t m = std::min_element(freeAt.begin(), freeAt.end()) - freeAt.begin();
        long now = freeAt[m];
        retire(now);
        if (ready.empty()) {                              // nothing can start: the machine idles until the next slice finishes
            if (running.empty()) break;                   // (cannot happen: the dependencies are acyclic)
            now = std::min_element(running.begin(), running.end())->first;
            retire(now);
            for (long& f : freeAt) f = std::max(f, now);
            continue;
        }
        const int s = ready.front();
        ready.erase(ready.begin());
        order.push_back(s);
        freeAt[m] = now + duration[s];
        running.emplace_back(freeAt[m], s);
    }
    if ((int)order.size() == n) out.launchOrder = order;
}
}  // namespace

void WalkPlanner::linkSlices(Plan& out, int repeatDurations) {
    linkDependencies(out);
    ticketForest(out);
    sliceTails(out);
    if (launchMachines <= 0.0 || out.segs.size() < 3) return;
    scheduleLaunchOrder(out, sliceDurations(out, repeatDurations), std::max(1, (int)(launchMachines + 0.5)));
}

// a kept plan made under the first-sight cap while lists that come again have a longer one
bool WalkPlanner::promotable(const CacheEntry& e, bool allowVirtual) const {
    return allowVirtual && e.parts == 1 && e.stepLimit == 0 && e.memStepCap > 0 && e.memStepCap < memCapSeen();
}

WalkPlanner::CacheEntry* WalkPlanner::findCached(const int* ops, int count, int tuple, int parts, bool allowVirtual, int chunkOps) {
    for (CacheEntry& e : cache_)
        if (e.valid && e.count == count && e.tuple == tuple && e.parts == parts && e.chunkOps == chunkOps && e.allowVirtual == allowVirtual && e.repeatWeights == repeatWeights && e.memDefTables == memDefTables &&
            e.stepLimit == (allowVirtual ? stepLimit : 0) && (e.memStepCap == (allowVirtual ? memStepCap : 0) || e.memStepCap == (allowVirtual ? memCapSeen() : 0)) &&
            e.tipEpoch == compactEpoch && memcmp(e.ops.data(), ops, (size_t)count * tuple * sizeof(int)) == 0)
            return &e;
    return nullptr;
}

bool WalkPlanner::replayCached(const int* ops, int count, int tuple, int parts, bool allowVirtual, int chunkOps, bool* simple) {
    if (!cacheEnabled || count < 16 || parts != keyParts_) return false;
    allowVirtual = allowVirtual && enabled_;
    CacheEntry* e = findCached(ops, count, tuple, parts, allowVirtual, chunkOps);
    if (!e || (simple && !e->simple)) return false;    // (asked for a simple list only: nothing has been touched)
    if (promotable(*e, allowVirtual)) return false;    // (plan() plans it again: planner.h memStepCapSeen)
    // memory definitions: a simple list skips mustMaterializeBefore, so nothing but this entry's own definitions may read what the list
    // overwrites (a branch move in between leaves such readers behind: that evaluation takes the long way) — looked at only when a
    // definition has changed hands since this entry's last replay
    if (simple && memStepCap > 0 && parts == 1 && e->cleanAtEpoch != tagEpoch_)
        for (int k = 0; k < count; k++)
            for (int u : tipUsers_[ops[(size_t)k * tuple]])
                if (tagOf_[u] != e->tag) return false;
    parts_ = parts;
    stamp_ += 2;                                       // a list of its own, as in plan()
    replay(*e, ops);
    cacheHits++;
    if (simple) *simple = e->simple;
    return true;
}

// Put the planner into the state planning the (closed) list again would leave it in; the kept program is handed out
// through `planned`.  A definition still tagged with this entry is the one the entry wrote (every other writer of a
// definition resets the tag), so the steady state costs one comparison per operation.
void WalkPlanner::replay(const CacheEntry& e, const int* ops) {
    // (nobody has written a tag since this entry was last replayed: every key is as that replay left it)
    for (int k = 0; e.cleanAtEpoch != tagEpoch_ && k < e.count; k++) {
        const int part = e.tuple > 7 ? ops[(size_t)k * e.tuple + 7] : 0;
        const int dest = key(ops[(size_t)k * e.tuple], part);
        if (e.defOn[k] ? tagOf_[dest] == e.tag : tagOf_[dest] < 0) continue;        // already what the entry leaves behind
        if (k + 6 < e.count) {                                   // (a definition is 1.5 KB: both sides of the copy below miss the caches otherwise)
            const int aheadPart = e.tuple > 7 ? ops[(size_t)(k + 6) * e.tuple + 7] : 0;
            const char* a = reinterpret_cast<const char*>(&e.defs[(size_t)k + 6]);
            const char* b = reinterpret_cast<const char*>(&virt_[key(ops[(size_t)(k + 6) * e.tuple], aheadPart)]);
            __builtin_prefetch(a); __builtin_prefetch(a + 64); __builtin_prefetch(a + 128); __builtin_prefetch(a + 192);
            __builtin_prefetch(b, 1); __builtin_prefetch(b + 64, 1); __builtin_prefetch(b + 128, 1); __builtin_prefetch(b + 192, 1);
        }
        const VirtDef& want = e.defs[k];
        VirtDef& cur = virt_[dest];
        // The usual reason to be here: the same node over the same tips, defined by the entry of the OTHER scale-buffer set (the evaluations
        // right behind a rescaling one) — the definition's leaves stand in the tips' user lists already, only its scale buffers change.
        // Taking the key out of every list and putting it back cost more than planning the list from scratch (tests/native/plan_check.cpp
        // bench-replay: 303 us against 218 for a 1000-taxon list on the build container).
        bool sameLeaves = cur.on && e.defOn[k] && cur.nSteps == want.nSteps;
        for (int st = 0; sameLeaves && st < want.nSteps; st++)
            sameLeaves = cur.steps[st].tipA == want.steps[st].tipA && cur.steps[st].tipB == want.steps[st].tipB;
        if (sameLeaves) {
            replayInPlace++;
            for (int st = 0; st < want.nSteps; st++) {
                const int was = cur.steps[st].scaleIdx;
                if (was < 0 || was == want.steps[st].scaleIdx) continue;
                bool still = false;
                for (int q = 0; q < want.nSteps && !still; q++) still = want.steps[q].scaleIdx == was;
                if (!still) { std::vector<int>& u = scaleUsers_[was]; u.erase(std::remove(u.begin(), u.end(), dest), u.end()); }
            }
        } else {
            if (cur.on) clearVirtualKey(dest);
            if (!e.defOn[k]) continue;                            // (defs[k] may be a leftover of an earlier list in this way)
        }
        cur = want;                                               // (tagged with e.tag when the entry was filled)
        tagOf_[dest] = e.tag; tagEpoch_++;
        cur.stamp = stamp_;
        cur.version = ++virtVersion_;
        cur.childVer1 = cur.sigTip1 ? -1 : virt_[key(cur.sigC1, part)].version;
        cur.childVer2 = cur.sigTip2 ? -1 : virt_[key(cur.sigC2, part)].version;
        if (sameLeaves) {
            for (int st = 0; st < cur.nSteps; st++) {
                const int sc = cur.steps[st].scaleIdx;
                if (sc < 0) continue;
                std::vector<int>& u = scaleUsers_[sc];
                if (std::find(u.begin(), u.end(), dest) == u.end()) u.push_back(dest);
            }
        } else registerVirtual(dest);
    }
    e.cleanAtEpoch = tagEpoch_;
    planned = &e.plan; plannedTag = e.tag;
    lastStored = e.stored; lastMemReads = e.memReads; lastHolds = e.holds; lastWaves = e.waves; lastWeighed = e.weighed;
}

void WalkPlanner::planMaterialize(const std::vector<int>& keys, Plan& out) {
    out.clear();
    parts_ = keyParts_;
    for (int part = 0; part < keyParts_; part++) {      // one slice per partition that has something to materialise
        PlanSeg seg; seg.progStart = (int)out.prog.size(); seg.partition = part; seg.wave = 0;
        for (int X : keys) {
            if (partitionOf(X) != part || !virt_[X].on) continue;
            emitVirtual(X, allSlots_, false, out);
            out.prog.back().storeBuf = bufferOf(X);
            clearVirtualKey(X);
        }
        seg.progCount = (int)out.prog.size() - seg.progStart;
        if (seg.progCount > 0) out.segs.push_back(seg);
    }
    linkSlices(out);
}

bool foldScaleFactors(const Plan& plan, int maxMembers, FoldMap& out) {
    const size_t n = plan.prog.size();
    out.payStart.assign(n + 1, 0);
    out.members.clear();
    for (const MicroOp& m : plan.prog) if (m.smode == PS_WRITE) return false;
    // first the count of members every micro-operation pays for (slices tile plan.prog in any order), then the lists themselves
    std::vector<std::vector<int>> pays(n);
    std::vector<int> acc, hold[3], cur;
    for (const PlanSeg& sg : plan.segs) {
        acc.clear();
        for (std::vector<int>& h : hold) h.clear();          // (no hold slot is in use at the start of a slice)
        for (int i = sg.progStart; i < sg.progStart + sg.progCount; i++) {
            const MicroOp& m = plan.prog[(size_t)i];
            cur.clear();
            if (isHoldKind(m.k1)) { const std::vector<int>& h = hold[m.k1 - PK_H0]; cur.insert(cur.end(), h.begin(), h.end()); }
            if (m.k2 == PK_ACC) cur.insert(cur.end(), acc.begin(), acc.end());
            if (m.smode == PS_READ) cur.push_back(m.scaleIdx);
            if (m.storeBuf >= 0 || i == sg.progStart + sg.progCount - 1 || (int)cur.size() >= maxMembers) { pays[(size_t)i] = cur; cur.clear(); }
            if (m.hold) hold[m.hold - 1] = cur;
            acc.swap(cur);
        }
    }
    // (a list is paid in the order of its buffer indices, not in the order its members were met: where a slice ends does not change
    // the product's rounding — a memory definition evaluated behind its operand's program meets them in another order than one that reads
    // the operand from memory)
    for (size_t i = 0; i < n; i++) {
        std::sort(pays[i].begin(), pays[i].end());
        out.payStart[i] = (int)out.members.size();
        out.members.insert(out.members.end(), pays[i].begin(), pays[i].end());
    }
    out.payStart[n] = (int)out.members.size();
    return true;
}

// ---- repeated sub-patterns (planner.h RepeatIndex) ---------------------------------------------------------------------
void RepeatIndex::init(int tipCount, int patterns, int maxClasses) {
    tipCount_ = tipCount; P_ = patterns; maxClasses_ = std::max(1, std::min(maxClasses, 65535));      // (classes are kept as 16-bit numbers)
    tip_.assign((size_t)tipCount, nullptr);
    capacity_ = (size_t)8 * (size_t)std::max(0, tipCount) + 1024;
    clear();
}

void RepeatIndex::clear() { clades_.clear(); memo_.clear(); }

std::size_t RepeatIndex::bytes() const {
    size_t b = clades_.capacity() * sizeof(Clade) + memo_.size() * 32;
    for (const Clade& c : clades_) b += c.cls.capacity() * sizeof(std::uint16_t) + (c.rep.capacity() + c.tips.capacity()) * sizeof(int);
    return b;
}

int RepeatIndex::find(int a, int b) const {
    if (a > b) std::swap(a, b);
    const auto it = memo_.find(((std::uint64_t)(unsigned)a << 32) | (unsigned)b);
    return it == memo_.end() ? -1 : it->second;
}

int RepeatIndex::intern(int a, int b) {
    if (a > b) std::swap(a, b);
    const std::uint64_t k = ((std::uint64_t)(unsigned)a << 32) | (unsigned)b;
    const auto it = memo_.find(k);
    if (it != memo_.end()) return it->second;
    Clade c; c.a = a; c.b = b;
    clades_.push_back(c);
    const int id = tipCount_ + (int)clades_.size() - 1;
    memo_.emplace(k, id);
    return id;
}

bool RepeatIndex::build(int id, int* budget) {
    if (isTip(id)) return tip_[(size_t)id] != nullptr;
    // children first, without recursion (a ladder clade is as deep as it has tips)
    std::vector<int> todo(1, id);
    while (!todo.empty()) {
        const int x = todo.back();
        Clade& c = clades_[(size_t)(x - tipCount_)];
        if (c.built) { todo.pop_back(); continue; }
        bool wait = false, none = false;
        for (int ch : {c.a, c.b}) {
            if (isTip(ch)) { if (!tip_[(size_t)ch]) none = true; continue; }
            const Clade& k = clades_[(size_t)(ch - tipCount_)];
            if (!k.built) { todo.push_back(ch); wait = true; } else if (k.over) none = true;
        }
        if (wait) continue;
        if (budget && (*budget)-- <= 0) return false;
        todo.pop_back();
        c.built = true; c.over = none; c.D = 0; c.cls.clear(); c.rep.clear(); c.tips.clear();
        builds++;
        if (none) continue;
        const std::uint8_t* ta = isTip(c.a) ? tip_[(size_t)c.a] : nullptr;
        const std::uint8_t* tb = isTip(c.b) ? tip_[(size_t)c.b] : nullptr;
        const Clade* ka = ta ? nullptr : &clades_[(size_t)(c.a - tipCount_)];
        const Clade* kb = tb ? nullptr : &clades_[(size_t)(c.b - tipCount_)];
        const std::uint32_t Db = tb ? 5u : (std::uint32_t)kb->D, Da = ta ? 5u : (std::uint32_t)ka->D;
        const std::uint64_t space = (std::uint64_t)Da * Db;                // (< 2^32: both counts are at most 65 535)
        c.cls.resize((size_t)P_);
        const bool direct = space <= ((std::uint64_t)1 << 16);     // (a table of 256 KB at most to clear per clade)
        std::unordered_map<std::uint32_t, int> sparse;
        if (direct) table_.assign((size_t)space, -1);
        bool over = false;
        for (int p = 0; p < P_; p++) {
            const std::uint32_t ca = ta ? (ta[p] < 4 ? ta[p] : 4u) : ka->cls[(size_t)p], cb = tb ? (tb[p] < 4 ? tb[p] : 4u) : kb->cls[(size_t)p];
            const std::uint32_t key = ca * Db + cb;
            int d;
            if (direct) { int& slot = table_[key]; if (slot < 0) { slot = c.D++; c.rep.push_back(p); } d = slot; }
            else { const auto ins = sparse.emplace(key, c.D); if (ins.second) { c.D++; c.rep.push_back(p); } d = ins.first->second; }
            if (c.D > maxClasses_) { over = true; break; }
            c.cls[(size_t)p] = (std::uint16_t)d;
        }
        if (over) { c.over = true; c.D = 0; std::vector<std::uint16_t>().swap(c.cls); std::vector<int>().swap(c.rep); continue; }
        for (int ch : {c.a, c.b}) {
            if (isTip(ch)) c.tips.push_back(ch);
            else { const Clade& k = clades_[(size_t)(ch - tipCount_)]; c.tips.insert(c.tips.end(), k.tips.begin(), k.tips.end()); }
        }
    }
    const Clade& c = clades_[(size_t)(id - tipCount_)];
    return c.built && !c.over;
}

void findRepeatRuns(const Plan& plan, const FoldMap* fold, RepeatIndex& idx, bool build, std::vector<RepeatRun>& out, std::vector<int>* missing, bool subRuns) {
    out.clear();
    if (plan.runs.empty()) return;
    for (const MicroOp& m : plan.prog) if (m.smode == PS_WRITE) return;
    auto pays = [&](int i) { return fold ? fold->payStart[(size_t)i + 1] > fold->payStart[(size_t)i] : plan.prog[(size_t)i].smode == PS_READ; };
    // micro-operations [start, last], whose slice ends at `end`, as a candidate (a whole run, or a sub-run of one).  false: the range itself
    // does not qualify — it stores, pays or reads something else than tips and its own results.  (Stricter than gatherRun of the slice
    // durations, which cannot know who pays: see there.)
    auto tableCandidate = [&](int start, int last, int end, bool sub) {
        bool ok = true;
        int acc = -1, hold[3] = {-1, -1, -1};
        for (int i = start; i <= last && ok; i++) {
            const MicroOp& m = plan.prog[(size_t)i];
            if (m.storeBuf >= 0 || pays(i)) ok = false;
            int a, b;
            if (m.k1 == PK_TIPS) a = m.a1; else if (isHoldKind(m.k1)) a = hold[m.k1 - PK_H0]; else a = -1;
            if (m.k2 == PK_TIPS) b = m.a2; else if (m.k2 == PK_ACC) b = acc; else b = -1;
            if (a < 0 || b < 0 || (m.k1 == PK_TIPS && a >= idx.tipCount()) || (m.k2 == PK_TIPS && b >= idx.tipCount())) { ok = false; break; }
            acc = idx.intern(a, b);
            if (m.hold && i < last) hold[m.hold - 1] = acc;
        }
        if (!ok) return false;
        RepeatRun rr; rr.start = start; rr.count = last - start + 1; rr.clade = acc; rr.viaHold = plan.prog[(size_t)last].hold != 0; rr.consumer = -1; rr.sub = sub;
        if (rr.viaHold) {
            const int k = PK_H0 + plan.prog[(size_t)last].hold - 1;
            for (int j = last + 1; j < end; j++) if (plan.prog[(size_t)j].k1 == k) { rr.consumer = j; break; }
        } else if (last + 1 < end && plan.prog[(size_t)last + 1].k2 == PK_ACC) rr.consumer = last + 1;
        if (rr.consumer < 0) return true;
        const RepeatIndex::Clade& c = idx.clade(rr.clade);
        if (!c.built) {
            if (build) idx.build(rr.clade);
            else { if (missing) missing->push_back(rr.clade); return true; }
        }
        if (idx.clade(rr.clade).over) return true;
        out.push_back(rr);
        return true;
    };
    std::vector<PlanRun> sub;
    for (size_t r = 0; r < plan.runs.size(); r++) {
        const PlanRun& run = plan.runs[r];
        // the slice of every run (runs are in program order, slices tile the program in any order)
        const int s = sliceHolding(plan, run.start);
        const int last = run.start + run.count - 1, end = s < 0 ? -1 : plan.segs[(size_t)s].progStart + plan.segs[(size_t)s].progCount;
        if (run.count <= 0 || end < 0 || last >= end) continue;
        if (tableCandidate(run.start, last, end, false) || !subRuns) continue;
        // not as a whole — a memory definition evaluated from memory, mostly: the plain clades inside it (planner.h RepeatRun), their
        // consumers inside the run
        sub.clear();
        plainSubRanges(plan.prog, run.start, run.count, pays, sub);
        for (const PlanRun& q : sub) tableCandidate(q.start, q.start + q.count - 1, last + 1, true);
    }
}

void emitRepeatPlan(const Plan& plan, const std::vector<RepeatRun>& take, RepeatPlan& out) {
    out.plan.clear(); out.lower.clear(); out.origin.clear(); out.tableReads = 0; out.twoTables = 0; out.unstoredConsumers = 0; out.subRuns = 0; out.subRunOps = 0;
    const size_t n = plan.prog.size();
    std::vector<MicroOp> mod(plan.prog);
    std::vector<char> gone(n, 0);
    auto sliceStart = [&](int at) { const int s = sliceHolding(plan, at); return s < 0 ? 0 : plan.segs[(size_t)s].progStart; };
    for (const RepeatRun& rr : take) {                   // (in program order: a consumer's first operand is settled before its second)
        const PlanRun run{rr.start, rr.count};
        for (int i = run.start; i < run.start + run.count; i++) gone[(size_t)i] = 1;
        if (rr.sub) { out.subRuns++; out.subRunOps += run.count; }
        MicroOp& c = mod[(size_t)rr.consumer];
        out.tableReads++;
        if (rr.viaHold) { c.k1 = PK_TAB; c.a1 = rr.clade; continue; }
        const int prev = run.start - 1;
        if (c.k1 == PK_TIPS || c.k1 == PK_MEM) {          // the other child is a leaf: the table goes first (the kernels prefetch a first child)
            const int k = c.k1, a = c.a1, mt = c.mat1;
            c.k1 = PK_TAB; c.a1 = rr.clade; c.mat1 = c.mat2;
            c.k2 = k; c.a2 = a; c.mat2 = mt;
        } else if (isHoldKind(c.k1) && prev >= sliceStart(run.start) && !gone[(size_t)prev] && mod[(size_t)prev].hold == c.k1 - PK_H0 + 1) {
            // the other child was parked while the run was evaluated; with the run gone it is still in ACC: nothing is parked
            mod[(size_t)prev].hold = 0;
            const int mt = c.mat1;
            c.k1 = PK_TAB; c.a1 = rr.clade; c.mat1 = c.mat2;
            c.k2 = PK_ACC; c.a2 = 0; c.mat2 = mt;
        } else { c.k2 = PK_TAB; c.a2 = rr.clade; }
    }
    {
        std::vector<char> counted(n, 0);
        for (const RepeatRun& rr : take) {
            if (counted[(size_t)rr.consumer]) continue;
            counted[(size_t)rr.consumer] = 1;
            const MicroOp& c = mod[(size_t)rr.consumer];
            if (c.k1 == PK_TAB && c.k2 == PK_TAB) out.twoTables++;
            if (c.storeBuf < 0) out.unstoredConsumers++;
        }
    }
    out.plan.segs = plan.segs; out.plan.deps = plan.deps; out.plan.launchOrder = plan.launchOrder; out.plan.snapPairs = plan.snapPairs; out.plan.leaves = plan.leaves;
    for (PlanSeg& sg : out.plan.segs) {
        const int s0 = sg.progStart, cnt = sg.progCount;
        sg.progStart = (int)out.plan.prog.size();
        for (int i = s0; i < s0 + cnt; i++) if (!gone[(size_t)i]) { out.plan.prog.push_back(mod[(size_t)i]); out.origin.push_back(i); }
        sg.progCount = (int)out.plan.prog.size() - sg.progStart;
    }
    for (const RepeatRun& rr : take) {
        const PlanRun run{rr.start, rr.count};
        PlanSeg sg; sg.progStart = (int)out.plan.prog.size(); sg.progCount = run.count; sg.partition = rr.clade; sg.wave = 0;
        sg.depStart = 0; sg.depCount = 0; sg.tail = run.count; sg.next = -1;
        for (int i = run.start; i < run.start + run.count; i++) {
            MicroOp m = plan.prog[(size_t)i];
            m.smode = PS_NONE; m.scaleIdx = PLAN_NONE;
            if (i == run.start + run.count - 1) m.hold = 0;
            out.plan.prog.push_back(m); out.origin.push_back(i);
        }
        out.lower.push_back(sg);
    }
}

}  // namespace mi355
