// node_pattern_layout_check.cpp — the scratch of beagleMi355NodePatternLikelihoods (beast-mcmc_amd/csrc/scratch_layout.h
// NodePatternLayout) over a grid of shapes: every section's offset and the total against the formulas written out here, sections
// disjoint and ascending, each aligned for its element type, the term stage null when the call does not ask for it.  Plain C++17
// (tests/test_stochastic_dollo_host.py).
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

#include "../../beast-mcmc_amd/csrc/scratch_layout.h"

using namespace mi355::scratch;

static void expect(bool ok, const char* what, size_t slots, size_t R, size_t P, size_t chunk, bool terms) {
    if (ok) return;
    std::printf("node_pattern_layout_check: %s fails at slots %zu rows %zu patterns %zu chunk %zu terms %d\n", what, slots, R, P, chunk,
                (int)terms);
    std::exit(1);
}

int main() {
    const size_t slotCounts[] = {1, 2, 15, 1999}, rows[] = {1, 3, 79, 1999}, patterns[] = {1, 33, 257, 100000}, chunks[] = {256, 512, 100096};
    char base[1];
    for (size_t slots : slotCounts) for (size_t R : rows) for (size_t P : patterns) for (size_t chunk : chunks) for (bool terms : {false, true}) {
        if (slots > R) continue;
        const size_t blocks = (P + 255) / 256;
        const NodePatternLayout L(slots, R, P, chunk, blocks, terms);
        expect(L.logPattern.offset == 0 && L.logPattern.count == P, "log pattern values", slots, R, P, chunk, terms);
        expect(L.blockSums.offset == P * 8 && L.blockSums.count == blocks, "block sums", slots, R, P, chunk, terms);
        expect(L.sum.offset == (P + blocks) * 8 && L.sum.count == 1, "the sum", slots, R, P, chunk, terms);       // (one copy takes all three)
        expect(L.lambda.offset == (P + blocks + 1) * 8 && L.lambda.count == slots * chunk, "lambda", slots, R, P, chunk, terms);
        expect(L.terms.offset == L.lambda.offset + slots * chunk * 8 && L.terms.count == (terms ? R * chunk : 0), "terms", slots, R, P, chunk, terms);
        expect(L.below.offset == up256(L.terms.offset + L.terms.count * 8) && L.below.count == slots * chunk, "below", slots, R, P, chunk, terms);
        expect(L.bytes() == L.below.offset + slots * chunk * 4, "bytes", slots, R, P, chunk, terms);
        expect(L.lambda.offset % 8 == 0 && L.terms.offset % 8 == 0 && L.below.offset % 256 == 0, "alignment", slots, R, P, chunk, terms);
        expect((L.terms.at(base) != nullptr) == terms, "null stage", slots, R, P, chunk, terms);
    }
    std::printf("node_pattern_layout_check: OK\n");
    return 0;
}
