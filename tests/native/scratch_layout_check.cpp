// scratch_layout_check.cpp — every layout of beast-mcmc_amd/csrc/scratch_layout.h over a grid of shapes (tests/test_scratch_layout.py):
// (a) each section's offset and the total equal the formulas the samplers carved their buffers by before the carver existed, written
//     out here from those sources, not from the header;
// (b) the sections are disjoint, in ascending order, and end within the total;
// (c) each offset is a multiple of its element type's alignment (row structs: 8, they hold doubles or pointers);
// (d) a section the call does not ask for resolves to null, every other one to base + offset.
// Host only: g++ -fsanitize=address,undefined, no HIP.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../beast-mcmc_amd/csrc/scratch_layout.h"

using namespace mi355::scratch;

namespace {

int failures = 0;
long checked = 0;

struct Seen { const char* name; size_t offset, bytes, align; const void* resolved; size_t wantOffset; bool wantAbsent; };

size_t up(size_t b) { return (b + 255) & ~(size_t)255; }
size_t D(size_t n) { return n * sizeof(double); }

struct Check {
    std::string what;
    std::vector<Seen> seen;
    char* base;
    Check(const std::string& w, size_t total) : what(w), base((char*)aligned_alloc(256, up(total) + 256)) {}
    ~Check() { free(base); }
    template <class T>
    void add(const char* name, const Section<T>& s, size_t wantOffset, bool wantAbsent = false, size_t align = alignof(T)) {
        seen.push_back({name, s.offset, s.bytes(), align, s.at(base), wantOffset, wantAbsent});
    }
    void fail(const char* name, const char* why, size_t got, size_t want) {
        if (failures++ < 20) printf("FAIL %s: %s %s (got %zu, want %zu)\n", what.c_str(), name, why, got, want);
    }
    void done(size_t total, size_t wantTotal) {
        checked++;
        if (total != wantTotal) fail("total", "differs from the parent's formula", total, wantTotal);
        size_t end = 0;
        for (const Seen& s : seen) {
            if (s.offset != s.wantOffset) fail(s.name, "offset differs from the parent's formula", s.offset, s.wantOffset);
            if (s.offset < end) fail(s.name, "overlaps the section before it", s.offset, end);
            end = s.offset + s.bytes;
            if (s.offset % s.align) fail(s.name, "is misaligned", s.offset % s.align, 0);
            const bool absent = s.bytes == 0;
            if (absent != s.wantAbsent) fail(s.name, "presence", absent, s.wantAbsent);
            if (absent ? s.resolved != nullptr : s.resolved != base + s.offset) fail(s.name, "resolves to the wrong pointer", 0, 0);
        }
        if (end > total) fail("total", "is smaller than the last section's end", total, end);
    }
};

std::string shape(const char* name, std::initializer_list<size_t> v) {
    std::string s = name;
    for (size_t x : v) s += " " + std::to_string(x);
    return s;
}

const size_t Ps[] = {1, 7, 300}, Rs[] = {1, 3, 5}, Ks[] = {1, 3, FLAG_SLOTS}, stages[] = {0, 1, 2}, rowSizes[] = {16, 12, 40, 44};

void ancestral() {
    for (size_t R : Rs) for (size_t P : Ps) {
        const AncestralLayout l(R, P);
        const size_t stateBytes = (R * P + 255) & ~(size_t)255, tailBytes = P * sizeof(int) + sizeof(unsigned);
        Check c(shape("ancestral", {R, P}), l.bytes());
        c.add("states", l.states, 0);
        c.add("cats", l.cats, stateBytes);
        c.add("error", l.error, stateBytes + P * sizeof(int));
        c.done(l.bytes(), stateBytes + tailBytes);
    }
}

void jump() {
    for (size_t S : {2, 4}) for (size_t C : {1, 3}) for (size_t P : Ps) for (size_t K : Ks) for (size_t R : Rs) for (size_t stageRows : stages) {
        const size_t blocks = (P + 255) / 256, SS = S * S;
        const JumpLayout l(S, C, P, K, R, blocks, stageRows);
        const size_t nReg = K * SS, nCond = K * R * C * SS, nPart = blocks * K * R, nRow = K * R, nPat = K * P, nStage = K * stageRows * P;
        const size_t doubles = 4 * nReg + nCond + nPart + nRow + nPat + nStage;
        Check c(shape("jump", {S, C, P, K, R, stageRows}), l.bytes());
        c.add("reg", l.reg, 0);
        c.add("rateReg", l.rateReg, D(nReg));
        c.add("tmp", l.tmp, D(2 * nReg));
        c.add("M", l.M, D(3 * nReg));
        c.add("cond", l.cond, D(4 * nReg));
        c.add("part", l.part, D(4 * nReg + nCond));
        c.add("row", l.row, D(4 * nReg + nCond + nPart));
        c.add("pat", l.pat, D(4 * nReg + nCond + nPart + nRow));
        c.add("stage", l.stage, D(4 * nReg + nCond + nPart + nRow + nPat), stageRows == 0);
        c.add("flags", l.flags, D(doubles));
        c.done(l.bytes(), doubles * sizeof(double) + 8 * sizeof(int));
    }
}

void uniform() {
    for (size_t S : {2, 4}) for (size_t N : {2, 41}) for (size_t P : Ps) for (size_t K : Ks) for (size_t R : Rs) for (size_t stageRows : stages)
    for (size_t rowBytes : rowSizes) for (bool history : {false, true}) {
        const size_t blocks = (P + 255) / 256, SS = S * S;
        const UniformLayout l(S, P, K, R, blocks, stageRows, N, rowBytes, history);
        const size_t nTable = N * SS, nReg = K * SS, nPart = blocks * K * R, nRow = K * R, nPat = K * P, nStage = K * stageRows * P;
        const size_t oRows = up((nTable + nReg + nPart + nRow + nPat + nStage) * sizeof(double));
        const size_t oFlags = oRows + up(R * rowBytes);
        const size_t oLong = oFlags + up(8 * sizeof(int));
        const size_t oCounts = oLong + up((P + 2) * sizeof(long long));
        Check c(shape("uniform", {S, N, P, K, R, stageRows, rowBytes, history}), l.bytes());
        c.add("table", l.table, 0);
        c.add("reg", l.reg, D(nTable));
        c.add("part", l.part, D(nTable + nReg));
        c.add("row", l.row, D(nTable + nReg + nPart));
        c.add("pat", l.pat, D(nTable + nReg + nPart + nRow));
        c.add("stage", l.stage, D(nTable + nReg + nPart + nRow + nPat), stageRows == 0);
        c.add("rows", l.rows, oRows, false, 8);
        c.add("flags", l.flags, oFlags);
        c.add("longs", l.longs, oLong);
        c.add("counts", l.counts, oCounts, !history);
        c.done(l.bytes(), oCounts + (history ? R * P * sizeof(int) : 0));
    }
}

void event() {
    for (size_t n : {1, 127, 128, 129, 1000}) {
        const EventLayout l(n);
        const size_t stBytes = (2 * n + 255) & ~(size_t)255;
        Check c(shape("event", {n}), l.bytes());
        c.add("states", l.states, 0);
        c.add("heights", l.heights, stBytes);
        c.done(l.bytes(), stBytes + n * sizeof(double));
    }
}

void simulate() {
    for (size_t slots : {1, 3, 9}) for (size_t chunk : {4, 64, 300}) for (size_t nRows : {1, 4}) for (size_t S : {2, 4}) for (size_t C : {1, 3}) {
        const size_t tableDoubles = (nRows - 1) * C * S * S + S + C, metaInts = (nRows - 1) * C * S + 2;
        const SimulateLayout l(slots, chunk, tableDoubles, metaInts);
        const size_t oCats = up(slots * chunk), oErr = oCats + chunk * sizeof(int), oTable = up(oErr + sizeof(unsigned));
        const size_t oMeta = oTable + tableDoubles * sizeof(double);
        Check c(shape("simulate", {slots, chunk, nRows, S, C}), l.bytes());
        c.add("states", l.states, 0);
        c.add("cats", l.cats, oCats);
        c.add("error", l.error, oErr);
        c.add("table", l.table, oTable);
        c.add("meta", l.meta, oMeta);
        c.done(l.bytes(), oMeta + metaInts * sizeof(int));
    }
}

void robust() {
    for (size_t P : Ps) for (size_t K : Ks) for (size_t R : Rs) for (size_t stageRows : stages) for (size_t rowBytes : rowSizes) {
        const size_t blocks = (P + 255) / 256, SS64 = 64 * 64;
        const RobustLayout l(64, P, K, R, blocks, stageRows, rowBytes);
        const size_t nEig = 2 * SS64 + 64, nReg = K * SS64, nCond = K * R * SS64, nPart = blocks * K * R, nRow = K * R, nSite = K * P,
                     nStage = K * stageRows * P;
        const size_t doubles = nEig + SS64 + 4 * nReg + nCond + nPart + nRow + nSite + nStage;
        Check c(shape("robust", {P, K, R, stageRows, rowBytes}), l.bytes());
        size_t o = 0;
        c.add("eig", l.eig, o); o += D(nEig);
        c.add("Q", l.Q, o); o += D(SS64);
        c.add("reg", l.reg, o); o += D(nReg);
        c.add("rateReg", l.rateReg, o); o += D(nReg);
        c.add("tmp", l.tmp, o); o += D(nReg);
        c.add("M", l.M, o); o += D(nReg);
        c.add("cond", l.cond, o); o += D(nCond);
        c.add("part", l.part, o); o += D(nPart);
        c.add("row", l.row, o); o += D(nRow);
        c.add("site", l.site, o); o += D(nSite);
        c.add("stage", l.stage, o, stageRows == 0);
        c.add("rows", l.rows, D(doubles), false, 8);
        c.add("error", l.error, D(doubles) + R * rowBytes);
        c.done(l.bytes(), doubles * sizeof(double) + R * rowBytes + sizeof(unsigned));
    }
}

void unconditioned() {
    for (size_t S : {2, 5, 64}) for (size_t L : Rs) for (size_t sites : Ps) for (size_t K : Ks) for (size_t stageRows : stages) {
        const size_t blocks = (sites + 255) / 256, SS = S * S;
        const UnconditionedLayout l(S, L, sites, K, blocks, stageRows);
        const size_t nReg = K * SS, nPart = blocks * K * L, nTot = K * L, nStage = K * stageRows * sites;
        const size_t doubles = SS + S + L + nReg + nPart + nTot + nStage;
        Check c(shape("unconditioned", {S, L, sites, K, stageRows}), l.bytes());
        c.add("Q", l.Q, 0);
        c.add("freq", l.freq, D(SS));
        c.add("len", l.len, D(SS + S));
        c.add("reg", l.reg, D(SS + S + L));
        c.add("part", l.part, D(SS + S + L + nReg));
        c.add("tot", l.tot, D(SS + S + L + nReg + nPart));
        c.add("stage", l.stage, D(SS + S + L + nReg + nPart + nTot), stageRows == 0);
        c.add("error", l.error, D(doubles));
        c.done(l.bytes(), doubles * sizeof(double) + sizeof(unsigned));
    }
}

void history() {
    const size_t C = 2;
    for (size_t slots : {1, 5}) for (size_t chunk : {256, 512}) for (size_t sites : {1, 300, 700}) for (size_t qCount : {1, 2}) for (size_t S : {2, 5})
    for (size_t K : {1, FLAG_SLOTS}) for (size_t R : {1, 3}) for (size_t rowBytes : {40, 44}) for (bool values : {false, true})
    for (bool rowTotals : {false, true}) for (bool hist : {false, true}) {
        const size_t SS = S * S, lines = qCount * S + 2, nTable = qCount * SS + S + C, waves = chunk / 64, nChunks = (sites + chunk - 1) / chunk;
        const HistoryLayout l(slots, chunk, sites, qCount, S, K, R, lines, nTable, waves, rowBytes, values, rowTotals, hist);
        const size_t oCats = up(slots * chunk), oErr = oCats + chunk * sizeof(int), oQ = up(oErr + sizeof(unsigned));
        const size_t nQ = qCount * SS, nReg = K * SS, nSite = K * chunk, nRow = K * R, nWave = rowTotals ? waves * K * R : 0,
                     nStage = values ? K * R * chunk : 0;
        const size_t oLast = oQ + (nQ + nReg + nTable + 2 * lines + nSite + nRow + nWave + nStage) * sizeof(double);
        const size_t oRows = up(oLast + lines * sizeof(int));
        const size_t oCounts = up(oRows + R * rowBytes);
        const size_t oOffsets = up(oCounts + (hist ? R * chunk * sizeof(int) : 0));
        Check c(shape("history", {slots, chunk, sites, qCount, S, K, R, rowBytes, values, rowTotals, hist}), l.bytes());
        c.add("states", l.states, 0);
        c.add("cats", l.cats, oCats);
        c.add("error", l.error, oErr);
        size_t o = oQ;
        c.add("Q", l.Q, o); o += D(nQ);
        c.add("reg", l.reg, o); o += D(nReg);
        c.add("table", l.table, o); o += D(nTable);
        c.add("total", l.total, o); o += D(lines);
        c.add("rate", l.rate, o); o += D(lines);
        c.add("site", l.site, o); o += D(nSite);
        c.add("row", l.row, o); o += D(nRow);
        c.add("wave", l.wave, o, !rowTotals); o += D(nWave);
        c.add("stage", l.stage, o, !values);
        c.add("last", l.last, oLast);
        c.add("rows", l.rows, oRows, false, 8);
        c.add("counts", l.counts, oCounts, !hist);
        c.add("offsets", l.offsets, oOffsets, !hist);
        c.done(l.bytes(), oOffsets + (hist ? (sites + nChunks) * sizeof(long long) : 0));
    }
}

}  // namespace

int main() {
    if (up256(0) != 0 || up256(1) != 256 || up256(256) != 256 || up256(257) != 512) { printf("FAIL up256\n"); failures++; }
    ancestral(); jump(); uniform(); event(); simulate(); robust(); unconditioned(); history();
    if (failures) { printf("scratch_layout_check: %d failure(s) in %ld layouts\n", failures, checked); return 1; }
    printf("scratch_layout_check: OK (%ld layouts)\n", checked);
    return 0;
}
