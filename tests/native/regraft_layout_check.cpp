// regraft_layout_check.cpp — the scratch of beagleMi355RegraftScores (beast-mcmc_amd/csrc/scratch_layout.h RegraftLayout) over a grid
// of shapes: every section's offset and the total against the formulas written out here, sections ascending, each aligned for its
// element type (the pendant vectors and the log ratios for the 32-byte loads of the 4-state kernel).  Plain C++17
// (tests/test_regraft_host.py).
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

#include "../../beast-mcmc_amd/csrc/scratch_layout.h"

using namespace mi355::scratch;

static void expect(bool ok, const char* what, size_t K, size_t M, size_t P, size_t S, size_t C) {
    if (ok) return;
    std::printf("regraft_layout_check: %s fails at candidates %zu pendants %zu patterns %zu states %zu categories %zu\n", what, K, M, P, S, C);
    std::exit(1);
}

int main() {
    const size_t candidates[] = {1, 7, 335, 1998}, patterns[] = {1, 33, 65, 100000}, states[] = {2, 4, 61, 255};
    const size_t categories[] = {1, 4, 9}, pendants[] = {1, 3};
    for (size_t K : candidates) for (size_t P : patterns) for (size_t S : states) for (size_t C : categories) for (size_t M : pendants)
    for (bool tiled : {false, true}) {
        const size_t segments = (P + 63) / 64, perVector = C * S * (tiled ? (P + 31) / 32 * 32 : P);
        const RegraftLayout L(K, M, perVector, segments, P);
        size_t at = 0;
        expect(L.pendants.offset == at && L.pendants.count == M * perVector, "pendant vectors", K, M, P, S, C);
        at = up256(at + L.pendants.count * 8);
        expect(L.ratios.offset == at && L.ratios.count == K * P, "log ratios", K, M, P, S, C);
        at += L.ratios.count * 8;
        expect(L.partial.offset == at && L.partial.count == segments * K, "segment sums", K, M, P, S, C);
        at += L.partial.count * 8;
        expect(L.scores.offset == at && L.scores.count == K, "scores", K, M, P, S, C);
        at = up256(at + L.scores.count * 8);
        expect(L.slots.offset == at && L.slots.count == M, "pendant slots", K, M, P, S, C);
        at = up256(at + L.slots.count * 4);
        expect(L.error.offset == at && L.error.count == 1 && L.bytes() == at + 4, "error word and bytes", K, M, P, S, C);
        expect(L.pendants.offset % 256 == 0 && L.ratios.offset % 256 == 0 && L.slots.offset % 256 == 0 && L.error.offset % 256 == 0 &&
               (S != 4 || perVector * 8 % 32 == 0), "alignment", K, M, P, S, C);
    }
    std::printf("regraft_layout_check: OK\n");
    return 0;
}
