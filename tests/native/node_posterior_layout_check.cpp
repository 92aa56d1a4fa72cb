// node_posterior_layout_check.cpp — the scratch of beagleMi355NodePosteriors (beast-mcmc_amd/csrc/scratch_layout.h
// NodePosteriorLayout) over a grid of shapes: every section's offset and the total against the formulas written out here, sections
// ascending, each aligned for its element type, a section the call does not ask for null.  Plain C++17
// (tests/test_node_posteriors_host.py).
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

#include "../../beast-mcmc_amd/csrc/scratch_layout.h"

using namespace mi355::scratch;

static void expect(bool ok, const char* what, size_t rows, size_t P, size_t S, size_t C, int wanted) {
    if (ok) return;
    std::printf("node_posterior_layout_check: %s fails at rows %zu patterns %zu states %zu categories %zu outputs %d\n", what, rows, P, S, C, wanted);
    std::exit(1);
}

int main() {
    const size_t rowCounts[] = {1, 3, 80, 3219}, patterns[] = {1, 33, 65, 257, 100000}, states[] = {2, 4, 61, 255}, categories[] = {1, 4, 17};
    char base[1];
    for (size_t rows : rowCounts) for (size_t P : patterns) for (size_t S : states) for (size_t C : categories) for (int wanted = 1; wanted < 16; wanted++) {
        const bool full = wanted & 1, map = wanted & 2, totals = wanted & 4, cats = wanted & 8;
        const size_t blocks = (P + 63) / 64;
        const NodePosteriorLayout L(rows, P, S, C, blocks, full, map, totals, cats);
        size_t at = 0;
        expect(L.posteriors.offset == at && L.posteriors.count == (full ? rows * P * S : 0), "posteriors", rows, P, S, C, wanted);
        at += L.posteriors.count * 8;
        expect(L.mapProb.offset == at && L.mapProb.count == (map ? rows * P : 0), "MAP probabilities", rows, P, S, C, wanted);
        at += L.mapProb.count * 8;
        expect(L.blockSums.offset == at && L.blockSums.count == (totals ? blocks * rows * S : 0), "block sums", rows, P, S, C, wanted);
        at += L.blockSums.count * 8;
        expect(L.totals.offset == at && L.totals.count == (totals ? rows * S : 0), "totals", rows, P, S, C, wanted);      // (right behind the block sums)
        at += L.totals.count * 8;
        expect(L.categories.offset == at && L.categories.count == (cats ? P * C : 0), "categories", rows, P, S, C, wanted);
        at = up256(at + L.categories.count * 8);
        expect(L.mapStates.offset == at && L.mapStates.count == (map ? rows * P : 0), "MAP states", rows, P, S, C, wanted);
        at = up256(at + L.mapStates.count);
        expect(L.error.offset == at && L.error.count == 1 && L.bytes() == at + 4, "error word and bytes", rows, P, S, C, wanted);
        expect(L.mapStates.offset % 256 == 0 && L.error.offset % 256 == 0, "alignment", rows, P, S, C, wanted);
        expect((L.posteriors.at(base) != nullptr) == full && (L.mapProb.at(base) != nullptr) == map && (L.mapStates.at(base) != nullptr) == map &&
               (L.blockSums.at(base) != nullptr) == totals && (L.totals.at(base) != nullptr) == totals && (L.categories.at(base) != nullptr) == cats &&
               L.error.at(base) != nullptr, "null sections", rows, P, S, C, wanted);
    }
    std::printf("node_posterior_layout_check: OK\n");
    return 0;
}
