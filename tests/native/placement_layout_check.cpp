// placement_layout_check.cpp — the scratch of beagleMi355PlacementScores (beast-mcmc_amd/csrc/scratch_layout.h PlacementLayout) over
// a grid of shapes: every section's offset and the total against the formulas written out here, sections ascending, each aligned for
// its element type.  Plain C++17 (tests/test_placement_host.py).
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

#include "../../beast-mcmc_amd/csrc/scratch_layout.h"

using namespace mi355::scratch;

static void expect(bool ok, const char* what, size_t K, size_t Q, size_t P, size_t S, size_t X) {
    if (ok) return;
    std::printf("placement_layout_check: %s fails at candidates %zu queries %zu patterns %zu states %zu codes %zu\n", what, K, Q, P, S, X);
    std::exit(1);
}

int main() {
    const size_t candidates[] = {1, 7, 70, 1998}, queries[] = {1, 17, 100}, patterns[] = {1, 33, 65, 100000}, states[] = {2, 4, 61, 255};
    const size_t categories[] = {1, 4, 9}, sites[] = {1, 257, 100001}, pendants[] = {1, 3};
    for (size_t K : candidates) for (size_t Q : queries) for (size_t P : patterns) for (size_t S : states) for (size_t C : categories)
    for (size_t n : sites) for (size_t M : pendants) for (size_t X : {S + 1, (size_t)255}) {
        const size_t segments = (P * X + 8191) / 8192;
        const PlacementLayout L(K, Q, M, n, segments, P, S, C, X);
        size_t at = 0;
        expect(L.pendant.offset == at && L.pendant.count == M * C * S * X, "pendant tables", K, Q, P, S, X);
        at += L.pendant.count * 8;
        expect(L.codeTable.offset == at && L.codeTable.count == X * S, "code table", K, Q, P, S, X);
        at += L.codeTable.count * 8;
        expect(L.table.offset == at && L.table.count == K * P * X, "log table", K, Q, P, S, X);
        at += L.table.count * 8;
        expect(L.partial.offset == at && L.partial.count == segments * Q * K, "segment sums", K, Q, P, S, X);
        at += L.partial.count * 8;
        expect(L.scores.offset == at && L.scores.count == Q * K, "scores", K, Q, P, S, X);
        at = up256(at + L.scores.count * 8);
        expect(L.counts.offset == at && L.counts.count == Q * P * X, "counts", K, Q, P, S, X);
        at = up256(at + L.counts.count * 4);
        expect(L.sitePatterns.offset == at && L.sitePatterns.count == n, "site patterns", K, Q, P, S, X);
        at += L.sitePatterns.count * 4;
        expect(L.slots.offset == at && L.slots.count == M, "pendant slots", K, Q, P, S, X);
        at = up256(at + L.slots.count * 4);
        expect(L.codes.offset == at && L.codes.count == Q * n, "query codes", K, Q, P, S, X);
        at = up256(at + L.codes.count);
        expect(L.error.offset == at && L.error.count == 1 && L.bytes() == at + 4, "error word and bytes", K, Q, P, S, X);
        expect(L.pendant.offset % 8 == 0 && L.counts.offset % 256 == 0 && L.sitePatterns.offset % 256 == 0 && L.codes.offset % 256 == 0 &&
               L.error.offset % 256 == 0, "alignment", K, Q, P, S, X);
    }
    std::printf("placement_layout_check: OK\n");
    return 0;
}
