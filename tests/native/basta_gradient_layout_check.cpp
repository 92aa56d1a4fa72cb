// basta_gradient_layout_check.cpp — the scratch of beagleBastaGradient (beast-mcmc_amd/csrc/scratch_layout.h BastaGradientLayout)
// over a grid of shapes: every section's offset and the total against the formulas written out here, sections disjoint and
// ascending, 256-byte boundaries where the comment in the header says so.  Plain C++17 (tests/test_basta_gradient_host.py).
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

#include "../../beast-mcmc_amd/csrc/scratch_layout.h"

using namespace mi355::scratch;

static void expect(bool ok, const char* what, size_t v, size_t k, size_t s) {
    if (ok) return;
    std::printf("basta_gradient_layout_check: %s fails at vectors %zu intervals %zu states %zu\n", what, v, k, s);
    std::exit(1);
}

int main() {
    const size_t vectors[] = {1, 7, 358, 401407}, intervals[] = {1, 3, 66, 1998}, states[] = {2, 4, 9, 61, 64, 65, 256};
    for (size_t v : vectors) for (size_t k : intervals) for (size_t s : states) {
        const BastaGradientLayout L(v, k, s);
        const size_t entries = s * s + s;
        expect(L.adjoints.offset == 0 && L.adjoints.count == v * s, "adjoints", v, k, s);
        expect(L.w.offset == v * s * 8 && L.w.count == v * s, "w", v, k, s);
        expect(L.parts.offset == up256(2 * v * s * 8) && L.parts.count == k * entries, "parts", v, k, s);
        expect(L.out.offset == up256(L.parts.offset + k * entries * 8) && L.out.count == entries, "out", v, k, s);
        expect(L.bytes() == L.out.offset + entries * 8, "bytes", v, k, s);
        expect(L.parts.offset % 256 == 0 && L.out.offset % 256 == 0, "alignment", v, k, s);
        expect(L.w.offset >= L.adjoints.offset + L.adjoints.bytes() && L.parts.offset >= L.w.offset + L.w.bytes() &&
               L.out.offset >= L.parts.offset + L.parts.bytes(), "order", v, k, s);
    }
    std::printf("basta_gradient_layout_check: OK\n");
    return 0;
}
