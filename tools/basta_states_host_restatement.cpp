// basta_states_host_restatement.cpp — beagleBastaSampleStates (include/beagle_mi355.h) restated in single-threaded C++, as the host
// side of tools/basta_states_bench.py: the root from p f, then every operation from the last to the first, each input from the row of
// the operation's matrix its dest state selects (BastaLikelihood.java:889-943), fixed vectors without a draw (:846-867), the engine's
// stateless SplitMix64 numbers and drawChoice.  Compiled with -ffp-contract=off it gives the device's states bit for bit.
#include <cfloat>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace {

inline unsigned long long mix64(unsigned long long state, unsigned long long key) {
    unsigned long long z = state + (key + 1ull) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

inline double uniform(unsigned long long stream, unsigned long long ctr) { return (double)(mix64(stream, ctr) >> 11) * 0x1.0p-53; }

template <class W>
inline int drawChoice(const W& w, int n, double u, bool map, bool& bad) {
    double total = 0.0, best = 0.0;
    int lastPositive = 0, choice = 0;
    for (int i = 0; i < n; i++) {
        const double v = w(i);
        total = total + v;
        if (v > 0.0) lastPositive = i;
        if (i == 0 || v > best) { best = v; choice = i; }
    }
    if (!(total > 0.0) || !(total <= DBL_MAX)) { bad = true; return 0; }
    if (map) return choice;
    double U = u * total;
    for (int i = 0; i < n; i++) {
        U = U - w(i);
        if (U < 0.0) return i;
    }
    return lastPositive;
}

}  // namespace

// outStates [replicates][vectors] (or null), outOccupancy [intervalCount - 1][S] (or null), outChanges [S][S] (or null); returns 1 when
// a draw met a total that is not finite and positive
extern "C" int basta_sample_states(int S, const int* ops, int n, const int* intervals, int intervalCount, const double* partials,
                                   int vectors, const double* matrices, const double* frequencies, int replicates,
                                   unsigned long long seed, int flags, unsigned char* outStates, double* outOccupancy, double* outChanges) {
    const bool map = flags & 1, asWritten = flags & 2;
    std::vector<int> intervalOf(n);
    for (int t = 0; t + 1 < intervalCount; t++) for (int k = intervals[t]; k < intervals[t + 1]; k++) intervalOf[k] = t;
    std::vector<int> fixedAt(vectors, -1);                   // the state of a vector with exactly one positive entry
    for (int v = 0; v < vectors; v++) {
        int positives = 0, at = 0;
        for (int i = 0; i < S; i++) if (partials[(size_t)v * S + i] > 0.0) { positives++; at = i; }
        if (positives == 1) fixedAt[v] = at;
    }
    std::vector<long long> occupancy((size_t)(intervalCount - 1) * S, 0), changes((size_t)S * S, 0);
    std::vector<uint8_t> states(vectors);
    bool bad = false;
    for (int r = 0; r < replicates; r++) {
        const unsigned long long stream = mix64(seed, (unsigned long long)r);
        states.assign(vectors, 255);
        for (int k = n - 1; k >= 0; k--) {
            const int* op = ops + (size_t)k * 8;
            const int dest = op[0];
            if (states[dest] == 255) {
                const double* p = partials + (size_t)dest * S;
                states[dest] = (uint8_t)drawChoice([&](int i) { return p[i] * frequencies[i]; }, S, uniform(stream, dest), map, bad);
            }
            const int s = states[dest];
            for (int side = 0; side < 2; side++) {
                const int in = op[side ? 3 : 1];
                if (in < 0) continue;
                int t = fixedAt[in];
                if (t < 0) {
                    const double* p = partials + (size_t)in * S;
                    const double* M = matrices + (size_t)op[side ? 4 : 2] * S * S;
                    const double* row = asWritten ? M + s : M + (size_t)s * S;
                    const int step = asWritten ? S : 1;
                    t = drawChoice([&](int j) { return row[(size_t)j * step] * p[j]; }, S, uniform(stream, in), map, bad);
                }
                states[in] = (uint8_t)t;
                if (op[3] >= 0) states[op[side ? 6 : 5]] = (uint8_t)t;
                occupancy[(size_t)intervalOf[k] * S + t]++;
                changes[(size_t)s * S + t]++;
            }
        }
        if (outStates) for (int v = 0; v < vectors; v++) outStates[(size_t)r * vectors + v] = states[v];
    }
    if (outOccupancy) for (size_t i = 0; i < occupancy.size(); i++) outOccupancy[i] = (double)occupancy[i];
    if (outChanges) for (size_t i = 0; i < changes.size(); i++) outChanges[i] = (double)changes[i];
    return bad ? 1 : 0;
}
