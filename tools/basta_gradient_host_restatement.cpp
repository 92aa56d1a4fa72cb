// basta_gradient_host_restatement.cpp — the BASTA gradient in single-threaded C++, as the host side of tools/basta_gradient_bench.py:
//   basta_gradient          the reverse sweep of beagleBastaGradient (include/beagle_mi355.h states the rule), every sum in the
//                           device's order: handed the device's vectors and matrices it returns the device's bits
//   basta_gradient_forward  the reference's forward mode on zeroed storage (GenericBastaLikelihoodDelegate.java peelPartialsGrad
//                           :443-534, peelPopSizeSGrad :536-603, reduceWithinIntervalGrad :680-753, reduceAcrossIntervalsGrad /
//                           ...GradPopSize :622-678; the reference's generic delegate is single-threaded too): S^2 tangent vectors
//                           per buffer, O(N S^4), for a list small enough to finish
// Both take the vectors and coalescent probabilities of an evaluation (tools/basta_host_restatement.cpp basta_evaluate).
// Compile with -ffp-contract=off.
#include <cstddef>
#include <vector>

namespace {

struct Sums { std::vector<double> e, f, g, h; };

// e, f, g, h per interval number, operations in list order (reduceWithinInterval)
Sums within(int S, const int* ops, const int* intervals, int intervalCount, const double* partials, int maxIntervals) {
    Sums s;
    s.e.assign((size_t)maxIntervals * S, 0.0); s.f = s.e; s.g = s.e; s.h = s.e;
    for (int t = 0; t + 1 < intervalCount; t++)
        for (int o = intervals[t]; o < intervals[t + 1]; o++) {
            const int* op = ops + (size_t)o * 8;
            const size_t at = (size_t)ops[(size_t)intervals[t] * 8 + 7] * S;
            for (int side = 0; side < 2; side++) {
                const int start = op[side ? 3 : 1], end = op[side ? 6 : 5];
                if (start < 0) continue;
                for (int i = 0; i < S; i++) {
                    const double a = partials[(size_t)start * S + i], b = partials[(size_t)end * S + i];
                    s.e[at + i] += a; s.f[at + i] += a * a; s.g[at + i] += b; s.h[at + i] += b * b;
                }
            }
        }
    return s;
}

// out_j = sum_i M[i][j] x_i, i in index order
void columns(int S, const double* M, const double* x, double* out) {
    for (int j = 0; j < S; j++) out[j] = 0.0;
    for (int i = 0; i < S; i++) for (int j = 0; j < S; j++) out[j] += M[(size_t)i * S + j] * x[i];
}

}  // namespace

extern "C" void basta_gradient(int S, const int* ops, int n, const int* intervals, int intervalCount, const double* lengths,
                               const double* distances, const double* matrices, const double* sizes, const double* partials,
                               int buffers, const double* coalescent, int maxIntervals, double* adjoints, double* outTheta, double* outW) {
    const Sums s = within(S, ops, intervals, intervalCount, partials, maxIntervals);
    std::vector<double> theta(S), c(S), w((size_t)buffers * S, 0.0), sum(S);
    for (int i = 0; i < S; i++) theta[i] = 1.0 / sizes[i];
    for (size_t i = 0; i < (size_t)buffers * S; i++) adjoints[i] = 0.0;
    auto V = [&](int x) { return partials + (size_t)x * S; };
    auto L = [&](int x) { return adjoints + (size_t)x * S; };
    for (int t = intervalCount - 2; t >= 0; t--) {
        if (intervals[t + 1] <= intervals[t]) continue;
        const size_t at = (size_t)ops[(size_t)intervals[t] * 8 + 7] * S;
        const double half = -lengths[t] * 0.5;
        for (int i = 0; i < S; i++) c[i] = half * theta[i];
        for (int o = intervals[t + 1] - 1; o >= intervals[t]; o--) {
            const int* op = ops + (size_t)o * 8;
            const int dest = op[0];
            if (op[3] < 0) {
                for (int i = 0; i < S; i++) L(dest)[i] = L(dest)[i] + c[i] * (s.g[at + i] - V(dest)[i]);
            } else {
                double dot = 0.0;
                for (int i = 0; i < S; i++) dot += L(dest)[i] * V(dest)[i];
                const double J = coalescent[op[7]];
                for (int i = 0; i < S; i++) {
                    const double wi = ((L(dest)[i] - dot) + 1.0) / J;
                    w[(size_t)dest * S + i] = wi;
                    L(op[5])[i] = (wi * V(op[6])[i]) * theta[i] + c[i] * (s.g[at + i] - V(op[5])[i]);
                    L(op[6])[i] = (wi * V(op[5])[i]) * theta[i] + c[i] * (s.g[at + i] - V(op[6])[i]);
                }
            }
            for (int side = 0; side < (op[3] >= 0 ? 2 : 1); side++) {
                const int in = op[side ? 3 : 1], acc = op[side ? 6 : 5];
                columns(S, matrices + (size_t)op[side ? 4 : 2] * S * S, L(acc), sum.data());
                for (int i = 0; i < S; i++) L(in)[i] = sum[i] + c[i] * (s.e[at + i] - V(in)[i]);
            }
        }
    }
    // per interval its operations in list order, then the intervals in index order
    std::vector<double> partW((size_t)S * S), partG(S);
    for (int i = 0; i < S * S; i++) outW[i] = 0.0;
    for (int i = 0; i < S; i++) outTheta[i] = 0.0;
    for (int t = 0; t + 1 < intervalCount; t++) {
        for (int i = 0; i < S * S; i++) partW[i] = 0.0;
        for (int i = 0; i < S; i++) partG[i] = 0.0;
        if (intervals[t + 1] > intervals[t]) {
            const size_t at = (size_t)ops[(size_t)intervals[t] * 8 + 7] * S;
            const double quarter = -lengths[t] * 0.25;
            for (int i = 0; i < S; i++) partG[i] = quarter * (((s.e[at + i] * s.e[at + i] - s.f[at + i]) + s.g[at + i] * s.g[at + i]) - s.h[at + i]);
            for (int o = intervals[t]; o < intervals[t + 1]; o++) {
                const int* op = ops + (size_t)o * 8;
                for (int side = 0; side < (op[3] >= 0 ? 2 : 1); side++) {
                    const int acc = op[side ? 6 : 5];
                    if (distances)
                        for (int a = 0; a < S; a++) {
                            const double tv = distances[t] * V(acc)[a];
                            for (int b = 0; b < S; b++) partW[(size_t)a * S + b] += tv * L(acc)[b];
                        }
                }
                if (op[3] >= 0) for (int i = 0; i < S; i++) partG[i] += (w[(size_t)op[0] * S + i] * V(op[5])[i]) * V(op[6])[i];
            }
        }
        for (int i = 0; i < S * S; i++) outW[i] += partW[i];
        for (int i = 0; i < S; i++) outTheta[i] += partG[i];
    }
}

extern "C" void basta_gradient_forward(int S, const int* ops, int n, const int* intervals, int intervalCount, const double* lengths,
                                       const double* distances, const double* matrices, const double* sizes, const double* partials,
                                       int buffers, const double* coalescent, int maxIntervals, double* outTheta, double* outW) {
    const Sums s = within(S, ops, intervals, intervalCount, partials, maxIntervals);
    const size_t VS = (size_t)buffers * S, NS = (size_t)maxIntervals * S, SS = (size_t)S * S;
    std::vector<double> grad(SS * VS, 0.0), pop((size_t)S * VS, 0.0), gradJ(SS * maxIntervals, 0.0), popJ((size_t)S * maxIntervals, 0.0);
    for (int t = 0; t + 1 < intervalCount; t++)
        for (int o = intervals[t]; o < intervals[t + 1]; o++) {
            const int* op = ops + (size_t)o * 8;
            const size_t dest = (size_t)op[0] * S, in1 = (size_t)op[1] * S, acc1 = (size_t)op[5] * S;
            const double* m1 = matrices + (size_t)op[2] * SS;
            const double distance = distances[t];
            for (size_t ab = 0; ab < SS; ab++) {                             // peelPartialsGrad :476-488
                double* gp = grad.data() + ab * VS;
                const int a = (int)(ab / S), b = (int)(ab % S);
                for (int i = 0; i < S; i++) {
                    double sum = 0.0;
                    for (int j = 0; j < S; j++) sum += m1[(size_t)i * S + j] * gp[in1 + j];
                    gp[dest + i] = sum;
                }
                gp[dest + b] += partials[acc1 + a] * distance;
            }
            for (int a = 0; a < S; a++) {                                    // peelPopSizeSGrad :553-561
                double* pp = pop.data() + (size_t)a * VS;
                for (int i = 0; i < S; i++) {
                    double sum = 0.0;
                    for (int j = 0; j < S; j++) sum += m1[(size_t)i * S + j] * pp[in1 + j];
                    pp[dest + i] = sum;
                }
            }
            if (op[3] < 0) continue;
            const size_t in2 = (size_t)op[3] * S, acc2 = (size_t)op[6] * S;
            const double* m2 = matrices + (size_t)op[4] * SS;
            const double J = coalescent[op[7]];
            for (size_t ab = 0; ab < SS; ab++) {                             // :498-531
                double* gp = grad.data() + ab * VS;
                const int a = (int)(ab / S), b = (int)(ab % S);
                double partialJ = 0.0;
                for (int i = 0; i < S; i++) {
                    for (int j = 0; j < S; j++) gp[acc2 + i] += m2[(size_t)i * S + j] * gp[in2 + j];
                    if (i == b) gp[acc2 + i] += partials[acc2 + a] * distance;
                    const double rightGrad = gp[acc2 + i], leftGrad = gp[dest + i];
                    const double entry = (leftGrad * partials[acc2 + i] + rightGrad * partials[acc1 + i]) / sizes[i];
                    partialJ += entry;
                    gp[dest + i] = entry / J;
                    gp[acc1 + i] = leftGrad;
                }
                for (int i = 0; i < S; i++) gp[dest + i] -= partialJ * partials[dest + i] / J;
                gradJ[ab * maxIntervals + op[7]] = partialJ;
            }
            for (int a = 0; a < S; a++) {                                    // :572-601
                double* pp = pop.data() + (size_t)a * VS;
                double partialJ = 0.0;
                for (int i = 0; i < S; i++) {
                    double rightGrad = 0.0;
                    for (int j = 0; j < S; j++) rightGrad += m2[(size_t)i * S + j] * pp[in2 + j];
                    const double leftGrad = pp[dest + i];
                    double entry = (leftGrad * partials[acc2 + i] + rightGrad * partials[acc1 + i]) / sizes[i];
                    if (i == a) entry += partials[acc1 + i] * partials[acc2 + i];
                    partialJ += entry;
                    pp[dest + i] = entry / J;
                    pp[acc1 + i] = leftGrad;
                    pp[acc2 + i] = rightGrad;
                }
                for (int i = 0; i < S; i++) pp[dest + i] -= partialJ * partials[dest + i] / J;
                popJ[(size_t)a * maxIntervals + op[7]] = partialJ;
            }
        }
    // reduceWithinIntervalGrad
    std::vector<double> ge(SS * NS, 0.0), gf(ge), gg(ge), gh(ge), pe((size_t)S * NS, 0.0), pf(pe), pg(pe), ph(pe);
    for (int o = 0; o < n; o++) {
        const int* op = ops + (size_t)o * 8;
        const size_t at = (size_t)op[7] * S;
        for (int side = 0; side < (op[3] >= 0 ? 2 : 1); side++) {
            const size_t start = (size_t)op[side ? 3 : 1] * S, end = (size_t)op[side ? 6 : 5] * S;
            for (size_t ab = 0; ab < SS + S; ab++) {
                const bool isPop = ab >= SS;
                const double* gp = isPop ? pop.data() + (ab - SS) * VS : grad.data() + ab * VS;
                const size_t to = (isPop ? ab - SS : ab) * NS + at;
                double* E = (isPop ? pe : ge).data() + to; double* F = (isPop ? pf : gf).data() + to;
                double* G = (isPop ? pg : gg).data() + to; double* H = (isPop ? ph : gh).data() + to;
                for (int i = 0; i < S; i++) {
                    E[i] += gp[start + i]; F[i] += 2 * partials[start + i] * gp[start + i];
                    G[i] += gp[end + i]; H[i] += 2 * partials[end + i] * gp[end + i];
                }
            }
        }
    }
    // reduceAcrossIntervalsGrad / ...GradPopSize
    for (size_t i = 0; i < SS; i++) outW[i] = 0.0;
    for (int i = 0; i < S; i++) outTheta[i] = 0.0;
    for (int t = 0; t + 1 < intervalCount; t++) {
        if (intervals[t + 1] <= intervals[t]) continue;
        const int number = ops[(size_t)intervals[t] * 8 + 7];
        const size_t at = (size_t)number * S;
        const double J = coalescent[number];
        for (size_t ab = 0; ab < SS + S; ab++) {
            const bool isPop = ab >= SS;
            const size_t from = (isPop ? ab - SS : ab) * NS + at;
            const double* E = (isPop ? pe : ge).data() + from; const double* F = (isPop ? pf : gf).data() + from;
            const double* G = (isPop ? pg : gg).data() + from; const double* H = (isPop ? ph : gh).data() + from;
            double sum = 0.0;
            for (int k = 0; k < S; k++) {
                sum += (2 * s.e[at + k] * E[k] - F[k] + 2 * s.g[at + k] * G[k] - H[k]) / sizes[k];
                if (isPop && k == (int)(ab - SS)) sum += s.e[at + k] * s.e[at + k] - s.f[at + k] + s.g[at + k] * s.g[at + k] - s.h[at + k];
            }
            double element = -lengths[t] * sum / 4;
            if (J != 0.0) element += (isPop ? popJ[(ab - SS) * maxIntervals + number] : gradJ[ab * maxIntervals + number]) / J;
            (isPop ? outTheta[ab - SS] : outW[ab]) += element;
        }
    }
}
