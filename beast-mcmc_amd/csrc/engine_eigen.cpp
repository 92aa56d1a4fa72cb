// engine_eigen.cpp — eigen systems of time-reversible models formed on the device (include/beagle_mi355.h
// beagleMi355SetReversibleModels, beagleMi355GetEigenDecomposition, beagleMi355EigenStats; kernels_eigen.hip): argument checks, the
// packed upload of the models' rates and frequencies, one launch per chunk of models, and the way back out of an eigen slot.
#include "engine_internal.h"

using namespace mi355::eng;

// models of one launch: what half the staging ring holds (BEAGLE_MI355_EIGEN_CHUNK=<n>, read at the call: fewer — tests of the split)
static size_t eigenChunk(size_t perModelBytes) {
    size_t n = std::max<size_t>(1, (RING_BYTES / 2) / perModelBytes);
    if (const char* e = getenv("BEAGLE_MI355_EIGEN_CHUNK")) { const long v = atol(e); if (v > 0) n = std::min(n, (size_t)v); }
    return n;
}

// What SubstitutionModelDelegate.updateSubstitutionModels does with a decomposition on the host and a setEigenDecomposition per model
// (SubstitutionModelDelegate.java:272-288), for reversible models, into the slots every later call reads.  Queued behind everything
// queued; nothing comes back.  No list held back reads an eigen slot (a held pre-order list reads branch matrices and partials).
static int setReversibleModels(Instance* in, const int* idx, int count, const double* rates, const double* freqs, int flags) {
    if (in->S > 64) return BEAGLE_ERROR_NO_IMPLEMENTATION;
    if (count < 0 || flags != 0) return BEAGLE_ERROR_OUT_OF_RANGE;
    if (count == 0) return BEAGLE_SUCCESS;
    if (!idx || !rates || !freqs) return BEAGLE_ERROR_OUT_OF_RANGE;
    const size_t S = (size_t)in->S, R = S * (S - 1) / 2, per = R + S;
    std::vector<char> named((size_t)in->eigenCount, 0);                  // (two workgroups into one slot would race)
    for (int k = 0; k < count; k++) {
        if (badIndex(idx[k], in->eigenCount) || named[(size_t)idx[k]]) return BEAGLE_ERROR_OUT_OF_RANGE;
        named[(size_t)idx[k]] = 1;
    }
    for (int k = 0; k < count; k++) {
        const double* r = rates + (size_t)k * R;
        const double* pi = freqs + (size_t)k * S;
        for (size_t i = 0; i < S; i++) if (!(std::isfinite(pi[i]) && pi[i] > 0.0)) return BEAGLE_ERROR_OUT_OF_RANGE;
        for (size_t e = 0; e < R; e++) if (!(std::isfinite(r[e]) && r[e] >= 0.0)) return BEAGLE_ERROR_OUT_OF_RANGE;
        double n = 0.0;                                                  // n = -sum_i pi_i Q_ii = 2 sum_{i<j} pi_i r_ij pi_j
        size_t e = 0;
        for (size_t i = 0; i < S; i++) for (size_t j = i + 1; j < S; j++, e++) n += 2.0 * pi[i] * r[e] * pi[j];
        if (!(std::isfinite(n) && n > 0.0)) return BEAGLE_ERROR_OUT_OF_RANGE;
    }
    // per model of the call the sweeps it took (beagleMi355EigenStats reads them): work in flight may still write the old block
    const size_t need = (size_t)count * sizeof(int);
    if (need > in->eigenSweepsDev.bytes) {
        const int rcg = growDevice(in, in->eigenSweepsDev, need, std::max<size_t>(2 * need, 4096), Grow::KeepOld); if (rcg) return rcg;
    }
    const size_t chunk = eigenChunk(per * sizeof(double) + sizeof(int));
    std::vector<char> pack;
    for (size_t first = 0; first < (size_t)count; first += chunk) {
        const size_t n = std::min(chunk, (size_t)count - first);
        // one packed upload per launch: [{rates, frequencies} double[n][R + S] | slot int[n]]
        const size_t modelBytes = n * per * sizeof(double), bytes = modelBytes + n * sizeof(int);
        pack.resize(bytes);
        double* pm = (double*)pack.data();
        for (size_t k = 0; k < n; k++) {
            memcpy(pm + k * per, rates + (first + k) * R, R * sizeof(double));
            memcpy(pm + k * per + R, freqs + (first + k) * S, S * sizeof(double));
        }
        memcpy(pack.data() + modelBytes, idx + first, n * sizeof(int));
        void* dPack = nullptr;
        const int rc = uploadTransient(in, pack.data(), bytes, &dPack); if (rc) return rc;
        // (from here on the slots change: the host's copy of what they held is no longer what they hold)
        if (!in->okEigen.empty()) for (size_t k = 0; k < n; k++) in->okEigen[(size_t)idx[first + k]] = 0;
        if (!mi355::launchEigenReversible(live(in), in->eigen, (const double*)dPack, (const int*)((const char*)dPack + modelBytes),
                                          in->eigenSweepsDev.as<int>() + first, (int)n, in->S, in->eigenComplex)) return BEAGLE_ERROR_GENERAL;
        HIP_TRY(hipGetLastError());
    }
    in->statEigenCalls++; in->statEigenModels += count; in->eigenLastCount = count;
    return BEAGLE_SUCCESS;
}

extern "C" {

int beagleMi355SetReversibleModels(int instance, const int* eigenIndices, int count, const double* relativeRates,
                                   const double* frequencies, int flags) {
    if (mi355::isShardedHandle(instance)) {                 // eigen systems are replicated: every shard decomposes its own copy (the same bits)
        return mi355::shardedBroadcast(instance, [&](int h) {
            return beagleMi355SetReversibleModels(h, eigenIndices, count, relativeRates, frequencies, flags); });
    }
    GET_INSTANCE_KEEP_PENDING(instance);                      // (a held-back pre-order list reads no eigen slot: it stays held)
    return setReversibleModels(in, eigenIndices, count, relativeRates, frequencies, flags);
}

int beagleMi355GetEigenDecomposition(int instance, int eigenIndex, double* outEigenVectors, double* outInverseEigenVectors,
                                     double* outEigenValues) {
    if (mi355::isShardedHandle(instance)) {
        return mi355::shardedFirst(instance, [&](int h) {
            return beagleMi355GetEigenDecomposition(h, eigenIndex, outEigenVectors, outInverseEigenVectors, outEigenValues); });
    }
    GET_INSTANCE_KEEP_PENDING(instance);
    if (badIndex(eigenIndex, in->eigenCount) || !outEigenVectors || !outInverseEigenVectors || !outEigenValues) return BEAGLE_ERROR_OUT_OF_RANGE;
    const size_t S = (size_t)in->S, nLambda = in->eigenComplex ? 2 * S : S, stride = 2 * S * S + nLambda;
    std::vector<double> slot(stride);
    const int rc = download(in, slot.data(), in->eigen + stride * (size_t)eigenIndex, stride * sizeof(double)); if (rc) return rc;
    memcpy(outEigenVectors, &slot[0], S * S * sizeof(double));
    memcpy(outInverseEigenVectors, &slot[S * S], S * S * sizeof(double));
    memcpy(outEigenValues, &slot[2 * S * S], nLambda * sizeof(double));
    return BEAGLE_SUCCESS;
}

int beagleMi355EigenStats(int instance, long long* out4) {
    if (mi355::isShardedHandle(instance)) { return mi355::shardedFirst(instance, [&](int h) { return beagleMi355EigenStats(h, out4); }); }
    GET_INSTANCE_KEEP_PENDING(instance);
    if (!out4) return BEAGLE_ERROR_OUT_OF_RANGE;
    out4[0] = in->statEigenCalls; out4[1] = in->statEigenModels; out4[2] = out4[3] = 0;
    if (in->eigenLastCount > 0) {
        std::vector<int> sweeps((size_t)in->eigenLastCount);
        const int rc = download(in, sweeps.data(), in->eigenSweepsDev.p, sweeps.size() * sizeof(int)); if (rc) return rc;
        for (int s : sweeps) { out4[2] = std::max<long long>(out4[2], s < 0 ? -s : s); if (s < 0) out4[3]++; }
    }
    return BEAGLE_SUCCESS;
}

}  // extern "C"
