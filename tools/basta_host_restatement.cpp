// basta_host_restatement.cpp — the three functions of the reference's pure-Java BASTA delegate (peelPartials,
// reduceWithinInterval, reduceAcrossIntervals: GenericBastaLikelihoodDelegate.java:813-877, 970-1006, 935-968) restated in
// single-threaded C++, as the host side of tools/basta_bench.py (the reference's generic delegate is single-threaded too).
// Same operation list, same matrices, same order of every sum as the device path.
#include <cmath>
#include <vector>

extern "C" double basta_evaluate(int S, const int* ops, const int* intervals, int intervalCount, const double* lengths,
                                 const double* matrices, const double* sizes, double* partials, double* coalescent, int maxIntervals) {
    for (int k = 0; k < maxIntervals; k++) coalescent[k] = 0.0;
    for (int t = 0; t + 1 < intervalCount; t++)
        for (int o = intervals[t]; o < intervals[t + 1]; o++) {
            const int* op = ops + (size_t)o * 8;
            double* dest = partials + (size_t)op[0] * S;
            const double* p1 = partials + (size_t)op[1] * S;
            const double* m1 = matrices + (size_t)op[2] * S * S;
            for (int i = 0; i < S; i++) {
                double sum = 0.0;
                for (int j = 0; j < S; j++) sum += m1[i * S + j] * p1[j];
                dest[i] = sum;
            }
            if (op[3] < 0) continue;
            const double* p2 = partials + (size_t)op[3] * S;
            const double* m2 = matrices + (size_t)op[4] * S * S;
            double* acc1 = partials + (size_t)op[5] * S;
            double* acc2 = partials + (size_t)op[6] * S;
            double prob = 0.0;
            for (int i = 0; i < S; i++) {
                double right = 0.0;
                for (int j = 0; j < S; j++) right += m2[i * S + j] * p2[j];
                const double left = dest[i];
                const double entry = left * right / sizes[i];
                dest[i] = entry; acc1[i] = left; acc2[i] = right;
                prob += entry;
            }
            for (int i = 0; i < S; i++) dest[i] /= prob;
            coalescent[op[7]] = prob;
        }
    std::vector<double> e((size_t)maxIntervals * S, 0.0), f(e), g(e), h(e);
    for (int t = 0; t + 1 < intervalCount; t++)
        for (int o = intervals[t]; o < intervals[t + 1]; o++) {
            const int* op = ops + (size_t)o * 8;
            const size_t at = (size_t)op[7] * S;
            for (int side = 0; side < 2; side++) {
                const int start = op[side ? 3 : 1], end = op[side ? 6 : 5];
                if (start < 0) continue;
                for (int i = 0; i < S; i++) {
                    const double a = partials[(size_t)start * S + i], b = partials[(size_t)end * S + i];
                    e[at + i] += a; f[at + i] += a * a; g[at + i] += b; h[at + i] += b * b;
                }
            }
        }
    double logL = 0.0;
    for (int t = 0; t + 1 < intervalCount; t++) {
        if (intervals[t + 1] <= intervals[t]) continue;
        const int number = ops[(size_t)intervals[t] * 8 + 7];
        const size_t at = (size_t)number * S;
        double sum = 0.0;
        for (int i = 0; i < S; i++) sum += (e[at + i] * e[at + i] - f[at + i] + g[at + i] * g[at + i] - h[at + i]) / sizes[i];
        double term = -lengths[t] * sum / 4;
        if (coalescent[number] != 0.0) term += std::log(coalescent[number]);
        logL += term;
    }
    return logL;
}
