// mds_host_restatement.cpp — the multidimensional-scaling likelihood on one host thread, for tools/mds_bench.py: the same work as
// the device library's three calls, organised the way the reference's pure-Java core organises it (an N x N table of increments
// filled over both triangles and halved; a row update that reads the old row from the table), plus the gradient of
// include/mds_mi355.h, which that core does not have.  Compiled by the tool with g++ -O3; a yardstick, not part of the library.
#include <math.h>
#include <stdint.h>

#include <vector>

namespace {
struct State {
    int n = 0, d = 0, truncated = 0;
    double tau = 1.0;
    const double* y = nullptr;       // borrowed, n * n
    std::vector<double> x, table;
    double sum = 0.0;
};
State g;

inline double logPhi(double z) { return log1p(-0.5 * erfc(z * 0.70710678118654752440)); }

inline double dist(const double* a, const double* b, int d) {
    double s = 0.0;
    for (int c = 0; c < d; ++c) {
        const double t = a[c] - b[c];
        s += t * t;
    }
    return sqrt(s);
}

inline double increment(int i, int j) {
    const double obs = g.y[(int64_t)i * g.n + j];
    if (obs != obs) return 0.0;
    const double dd = dist(&g.x[(int64_t)i * g.d], &g.x[(int64_t)j * g.d], g.d), r = dd - obs;
    double inc = r * r;
    if (g.truncated) {
        inc *= 0.5 * g.tau;
        if (i != j) inc += logPhi(dd * sqrt(g.tau));
    }
    return inc;
}
}  // namespace

// seeded inputs made here (numpy needs several N x N temporaries for the same): locations uniform in a box of side 8,
// observations |distance + noise|, noise uniform in +-0.5, symmetric, zero diagonal, about 5 % of the pairs NaN
extern "C" void mds_host_synthesize(int n, int d, uint64_t seed, double* x, double* y) {
    uint64_t s = seed * 0x9E3779B97F4A7C15ull + 1;
    auto next = [&s]() {
        s += 0x9E3779B97F4A7C15ull;
        uint64_t z = s;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        z ^= z >> 31;
        return (double)(z >> 11) * (1.0 / 9007199254740992.0);
    };
    for (int64_t e = 0; e < (int64_t)n * d; ++e) x[e] = 8.0 * next() - 4.0;
    for (int i = 0; i < n; ++i) {
        y[(int64_t)i * n + i] = 0.0;
        for (int j = i + 1; j < n; ++j) {
            const double u = next();
            const double v = u < 0.05 ? NAN : fabs(dist(x + (int64_t)i * d, x + (int64_t)j * d, d) + (next() - 0.5));
            y[(int64_t)i * n + j] = y[(int64_t)j * n + i] = v;
        }
    }
}

extern "C" void mds_host_setup(int n, int d, int truncated, double tau, const double* x, const double* y) {
    g.n = n;
    g.d = d;
    g.truncated = truncated;
    g.tau = tau;
    g.y = y;
    g.x.assign(x, x + (int64_t)n * d);
    g.table.assign((size_t)n * (size_t)n, 0.0);
}

extern "C" double mds_host_full() {
    double sum = 0.0;
    for (int i = 0; i < g.n; ++i)
        for (int j = 0; j < g.n; ++j) {
            const double inc = increment(i, j);
            g.table[(int64_t)i * g.n + j] = inc;
            sum += inc;
        }
    g.sum = sum / 2;
    return g.truncated ? g.sum : 0.5 * g.tau * g.sum;
}

extern "C" double mds_host_row(int k, const double* moved) {
    for (int c = 0; c < g.d; ++c) g.x[(int64_t)k * g.d + c] = moved[c];
    double delta = 0.0;
    for (int j = 0; j < g.n; ++j) {
        const double inc = increment(k, j);
        delta += inc - g.table[(int64_t)k * g.n + j];
        g.table[(int64_t)k * g.n + j] = inc;
    }
    for (int j = 0; j < g.n; ++j) g.table[(int64_t)j * g.n + k] = g.table[(int64_t)k * g.n + j];      // acceptState
    g.sum += delta;
    return g.truncated ? g.sum : 0.5 * g.tau * g.sum;
}

extern "C" void mds_host_gradient(double* out) {
    const double st = sqrt(g.tau);
    for (int i = 0; i < g.n; ++i) {
        double acc[16] = {0};
        const double* xi = &g.x[(int64_t)i * g.d];
        for (int j = 0; j < g.n; ++j) {
            const double obs = g.y[(int64_t)i * g.n + j];
            if (j == i || obs != obs) continue;
            const double* xj = &g.x[(int64_t)j * g.d];
            const double dd = dist(xi, xj, g.d);
            if (!(dd > 0.0)) continue;
            double coef = g.tau * (dd - obs);
            if (g.truncated) {
                const double z = dd * st;
                coef += st * 0.39894228040143267794 * exp(-0.5 * z * z) / (1.0 - 0.5 * erfc(z * 0.70710678118654752440));
            }
            coef /= dd;
            for (int c = 0; c < g.d; ++c) acc[c] -= coef * (xi[c] - xj[c]);
        }
        for (int c = 0; c < g.d; ++c) out[(int64_t)i * g.d + c] = acc[c];
    }
}
