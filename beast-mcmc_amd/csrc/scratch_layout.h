// scratch_layout.h — what is inside the samplers' grow-on-demand device buffers (engine_internal.h Instance::ancestralDev, jumpDev,
// uniformDev, nodePatternDev, nodePosteriorDev, placementDev, regraftDev, eventDev, simulateDev, robustDev, historyDev): a carver that lays sections out one after another, and per
// buffer a layout that names its sections from plain integers.  Host only, plain C++17, no HIP: tests/native/scratch_layout_check.cpp
// (NodePatternLayout: node_pattern_layout_check.cpp) compiles it alone and checks every layout's offsets, order and alignment.  The .cpp files resolve sections to pointers (at / as) and grow the
// buffer to bytes(); they keep no offset arithmetic.
#pragma once
#include <cstddef>
#include <cstdint>

namespace mi355 {
namespace scratch {

inline size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }

// `count` elements of T at byte `offset` of a buffer; an empty section (what a call did not ask for) resolves to nullptr
template <class T>
struct Section {
    size_t offset = 0, count = 0;
    size_t bytes() const { return count * sizeof(T); }
    T* at(char* base) const { return as<T>(base); }
    template <class U> U* as(char* base) const { return count ? reinterpret_cast<U*>(base + offset) : nullptr; }      // (row structs: Section<char>)
};

// A layout derives from this and takes its sections in its constructor, in buffer order; align(256) stands wherever the next
// section starts on a 256-byte boundary — "(256)" in the comments below
class Carver {
    size_t off_ = 0;
protected:
    template <class T> Section<T> take(size_t count) { Section<T> s{off_, count}; off_ += s.bytes(); return s; }
    void align(size_t a) { off_ = (off_ + a - 1) / a * a; }
public:
    size_t bytes() const { return off_; }
};
using Doubles = Section<double>;
using Ints = Section<int>;

constexpr int FLAG_SLOTS = 8;                // ints kept for the register flags whatever K is (kernels.h MAX_JUMP_REGISTERS)

// ancestralDev: states [R][P] | (256) categories [P] | error word
struct AncestralLayout : Carver {
    Section<uint8_t> states; Ints cats; Section<unsigned> error;
    AncestralLayout(size_t R, size_t P) { states = take<uint8_t>(R * P); align(256); cats = take<int>(P); error = take<unsigned>(1); }
};

// jumpDev: registers | rateReg | tmp | M (each [K][S][S]) | cond [K][R][C][S][S] | blockPartials [blocks][K][R] | rowTotals [K][R]
//          | patternTotals [K][P] | outJumps stage [K][stageRows][P] | register flags
struct JumpLayout : Carver {
    Doubles reg, rateReg, tmp, M, cond, part, row, pat, stage; Ints flags;
    JumpLayout(size_t S, size_t C, size_t P, size_t K, size_t R, size_t blocks, size_t stageRows) {
        for (Doubles* d : {&reg, &rateReg, &tmp, &M}) *d = take<double>(K * S * S);
        cond = take<double>(K * R * C * S * S); part = take<double>(blocks * K * R); row = take<double>(K * R); pat = take<double>(K * P);
        stage = take<double>(K * stageRows * P); flags = take<int>(FLAG_SLOTS);
    }
};

// uniformDev: R^n table [N][S][S] | registers [K][S][S] | blockPartials [blocks][K][R] | rowTotals [K][R] | patternTotals [K][P]
//             | stage [K][stageRows][P] | (256) rows [R] | (256) register flags | (256) pattern offsets [P], total, fallbacks
//             | (256) event counts [R][P] (histories)
struct UniformLayout : Carver {
    Doubles table, reg, part, row, pat, stage; Section<char> rows; Ints flags; Section<long long> longs; Ints counts;
    UniformLayout(size_t S, size_t P, size_t K, size_t R, size_t blocks, size_t stageRows, size_t N, size_t rowBytes, bool history) {
        table = take<double>(N * S * S); reg = take<double>(K * S * S); part = take<double>(blocks * K * R); row = take<double>(K * R);
        pat = take<double>(K * P); stage = take<double>(K * stageRows * P); align(256);
        rows = take<char>(R * rowBytes); align(256);
        flags = take<int>(FLAG_SLOTS); align(256);
        longs = take<long long>(P + 2); align(256);
        counts = take<int>(history ? R * P : 0);
    }
};

// nodePatternDev: log pattern values [P] | block sums [blocks] | the sum | Lambda [slots][chunk] | term stage [R][chunk]
//                 (outNodeLogTerms) | (256) extant tips below [slots][chunk]
struct NodePatternLayout : Carver {
    Doubles logPattern, blockSums, sum, lambda, terms; Ints below;
    NodePatternLayout(size_t slots, size_t R, size_t P, size_t chunk, size_t blocks, bool wantTerms) {
        logPattern = take<double>(P); blockSums = take<double>(blocks); sum = take<double>(1); lambda = take<double>(slots * chunk);
        terms = take<double>(wantTerms ? R * chunk : 0); align(256);
        below = take<int>(slots * chunk);
    }
};

// nodePosteriorDev: posteriors stage [rows][P][S] (outPosteriors) | MAP probabilities [rows][P] | block sums [blocks][rows][S] and
//                   totals [rows][S] (outStateTotals) | category posteriors [P][C] | (256) MAP states [rows][P] | (256) error word
//                   — rows: those of one launch; a section the call did not ask for is empty
struct NodePosteriorLayout : Carver {
    Doubles posteriors, mapProb, blockSums, totals, categories; Section<uint8_t> mapStates; Section<unsigned> error;
    NodePosteriorLayout(size_t rows, size_t P, size_t S, size_t C, size_t blocks, bool full, bool map, bool wantTotals, bool cats) {
        posteriors = take<double>(full ? rows * P * S : 0); mapProb = take<double>(map ? rows * P : 0);
        blockSums = take<double>(wantTotals ? blocks * rows * S : 0); totals = take<double>(wantTotals ? rows * S : 0);
        categories = take<double>(cats ? P * C : 0); align(256);
        mapStates = take<uint8_t>(map ? rows * P : 0); align(256);
        error = take<unsigned>(1);
    }
};

// placementDev: pendant tables [pendants][C][S][X] | code table [X][S] | log table [candidates][P][X] (outLogTable) | segment sums
//               [segments][queries][candidates] | scores [queries][candidates] | (256) counts [queries][P][X] | (256) site patterns
//               [sites] | pendant matrix slots [pendants] | (256) query codes [queries][sites] | (256) error word
//               — candidates, queries: those of one launch
struct PlacementLayout : Carver {
    Doubles pendant, codeTable, table, partial, scores; Ints counts, sitePatterns, slots; Section<uint8_t> codes; Section<unsigned> error;
    PlacementLayout(size_t candidates, size_t queries, size_t pendants, size_t sites, size_t segments, size_t P, size_t S, size_t C, size_t X) {
        pendant = take<double>(pendants * C * S * X); codeTable = take<double>(X * S); table = take<double>(candidates * P * X);
        partial = take<double>(segments * queries * candidates); scores = take<double>(queries * candidates); align(256);
        counts = take<int>(queries * P * X); align(256);
        sitePatterns = take<int>(sites); slots = take<int>(pendants); align(256);
        codes = take<uint8_t>(queries * sites); align(256);
        error = take<unsigned>(1);
    }
};

// regraftDev: pendant vectors [pendants][perVector] | log ratios [candidates][P] (outPatternLogRatios) | segment sums
//             [segments][candidates] | scores [candidates] | (256) pendant matrix slots [pendants] | (256) error word
//             — candidates: those of one launch; perVector: kernels.h regraftPendantDoubles, a multiple of 4 doubles
struct RegraftLayout : Carver {
    Doubles pendants, ratios, partial, scores; Ints slots; Section<unsigned> error;
    RegraftLayout(size_t candidates, size_t pendantCount, size_t perVector, size_t segments, size_t P) {
        pendants = take<double>(pendantCount * perVector); align(256);
        ratios = take<double>(candidates * P); partial = take<double>(segments * candidates); scores = take<double>(candidates); align(256);
        slots = take<int>(pendantCount); align(256);
        error = take<unsigned>(1);
    }
};

// eventDev: event states [n][2] | (256) event heights [n]
struct EventLayout : Carver {
    Section<uint8_t> states; Doubles heights;
    explicit EventLayout(size_t n) { states = take<uint8_t>(2 * n); align(256); heights = take<double>(n); }
};

// simulateDev: states [slots][chunk] | (256) categories [chunk] | error word | (256) cumulative tables | their meta words
struct SimulateLayout : Carver {
    Section<uint8_t> states; Ints cats; Section<unsigned> error; Doubles table; Ints meta;
    SimulateLayout(size_t slots, size_t chunk, size_t tableDoubles, size_t metaInts) {
        states = take<uint8_t>(slots * chunk); align(256);
        cats = take<int>(chunk); error = take<unsigned>(1); align(256);
        table = take<double>(tableDoubles); meta = take<int>(metaInts);
    }
};

// robustDev, conditional counts (S = 64): U, U^-1, lambda [2 S S + S] | Q [S][S] | registers | rateReg | tmp | M (each [K][S][S])
//            | cond [K][R][S][S] | blockPartials [blocks][K][R] | branchTotals [K][R] | siteTotals [K][P]
//            | outCounts stage [K][stageRows][P] | rows [R] | error word
struct RobustLayout : Carver {
    Doubles eig, Q, reg, rateReg, tmp, M, cond, part, row, site, stage; Section<char> rows; Section<unsigned> error;
    RobustLayout(size_t S, size_t P, size_t K, size_t R, size_t blocks, size_t stageRows, size_t rowBytes) {
        eig = take<double>(2 * S * S + S); Q = take<double>(S * S);
        for (Doubles* d : {&reg, &rateReg, &tmp, &M}) *d = take<double>(K * S * S);
        cond = take<double>(K * R * S * S); part = take<double>(blocks * K * R); row = take<double>(K * R); site = take<double>(K * P);
        stage = take<double>(K * stageRows * P); rows = take<char>(R * rowBytes); error = take<unsigned>(1);
    }
};

// robustDev, unconditioned counts: Q [S][S] | frequencies [S] | lengths [L] | registers [K][S][S] | blockPartials [blocks][K][L]
//            | totals [K][L] | outCounts stage [K][stageRows][sites] | error word
struct UnconditionedLayout : Carver {
    Doubles Q, freq, len, reg, part, tot, stage; Section<unsigned> error;
    UnconditionedLayout(size_t S, size_t L, size_t sites, size_t K, size_t blocks, size_t stageRows) {
        Q = take<double>(S * S); freq = take<double>(S); len = take<double>(L); reg = take<double>(K * S * S);
        part = take<double>(blocks * K * L); tot = take<double>(K * L); stage = take<double>(K * stageRows * sites);
        error = take<unsigned>(1);
    }
};

// historyDev: states [slots][chunk] | (256) categories [chunk] | error word | (256) Q [qCount][S][S] | registers [K][S][S] | jump
//             tables | line totals | line rates | site totals [K][chunk] | row totals [K][R] | wave sums [waves][K][R] (row totals)
//             | values [K][R][chunk] (outValues) | line last indices | (256) rows [R] | (256) event counts [R][chunk] (histories)
//             | (256) site offsets [sites + chunks] (histories)
struct HistoryLayout : Carver {
    Section<uint8_t> states; Ints cats; Section<unsigned> error; Doubles Q, reg, table, total, rate, site, row, wave, stage; Ints last;
    Section<char> rows; Ints counts; Section<long long> offsets;
    HistoryLayout(size_t slots, size_t chunk, size_t sites, size_t qCount, size_t S, size_t K, size_t R, size_t lines, size_t tableDoubles,
                  size_t waves, size_t rowBytes, bool values, bool rowTotals, bool history) {
        states = take<uint8_t>(slots * chunk); align(256);
        cats = take<int>(chunk); error = take<unsigned>(1); align(256);
        Q = take<double>(qCount * S * S); reg = take<double>(K * S * S); table = take<double>(tableDoubles);
        total = take<double>(lines); rate = take<double>(lines); site = take<double>(K * chunk); row = take<double>(K * R);
        wave = take<double>(rowTotals ? waves * K * R : 0); stage = take<double>(values ? K * R * chunk : 0);
        last = take<int>(lines); align(256);
        rows = take<char>(R * rowBytes); align(256);
        counts = take<int>(history ? R * chunk : 0); align(256);
        offsets = take<long long>(history ? sites + (sites + chunk - 1) / chunk : 0);
    }
};

// BASTA lineage demes (engine_basta.cpp Basta::statesDev): states [vectors][chunk] | (256) outStates stage [chunk][vectors]
//             | (256) occupancy [intervals][S] | changes [S][S] (64-bit counters) | error word
struct BastaStatesLayout : Carver {
    Section<uint8_t> states, stage; Section<unsigned long long> occupancy, changes; Section<unsigned> error;
    BastaStatesLayout(size_t vectors, size_t chunk, size_t intervals, size_t S, bool copyOut) {
        states = take<uint8_t>(vectors * chunk); align(256);
        stage = take<uint8_t>(copyOut ? chunk * vectors : 0); align(256);
        occupancy = take<unsigned long long>(intervals * S); changes = take<unsigned long long>(S * S); error = take<unsigned>(1);
    }
};

// BASTA gradient (engine_basta.cpp Basta::gradientDev): adjoints [vectors][S] | w [vectors][S] | (256) per-interval shares
//             [intervals][S * S + S] | (256) out [S * S + S]
struct BastaGradientLayout : Carver {
    Doubles adjoints, w, parts, out;
    BastaGradientLayout(size_t vectors, size_t intervals, size_t S) {
        adjoints = take<double>(vectors * S); w = take<double>(vectors * S); align(256);
        parts = take<double>(intervals * (S * S + S)); align(256);
        out = take<double>(S * S + S);
    }
};

}  // namespace scratch
}  // namespace mi355
