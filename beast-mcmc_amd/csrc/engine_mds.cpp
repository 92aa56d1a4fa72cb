// engine_mds.cpp — host side of libmds2_jni.so: the instance table and the C ABI of include/mds_mi355.h over the launchers of
// kernels_mds.h.
//
// State per instance, restating MultiDimensionalScalingCoreImpl (src/dr/inference/multidimensionalscaling/
// MultiDimensionalScalingCoreImpl.java) without its N x N table of increments:
//   host (pinned)  cur, stored [N][D]: the caller's locations and the stored copy (restore swaps the two pointers)
//   device         obs [N][ld], loc [N][D] = the locations the sums below were computed at, saved[D] = loc[k] before the last row
//                  update, slab, out[2]
//   sums           ssq = sum (d - y)^2 and tr = sum log Phi(d sqrt tau) (truncated instances), and their stored copies
//   flags          sumKnown, incrementsKnown, updatedLocation, rowSaved (the Java core's `storedIncrements != null`) as there;
//                  deviceStale / deviceStaleAt / movedSinceStore say where loc differs from cur, which the Java core's table
//                  cannot tell — a row update is taken only when loc differs from cur in the updated location alone.
// A row update needs no upload: the new location travels in the kernel arguments; the old one is still in loc.
#include <math.h>
#include <string.h>

#include <memory>
#include <mutex>
#include <new>
#include <vector>

#include "../../include/mds_mi355.h"
#include "kernels_mds.h"

#define MDS_EXPORT extern "C" __attribute__((visibility("default")))

namespace {

struct HipFailure { hipError_t err; };
inline void check(hipError_t err) {
    if (err != hipSuccess) throw HipFailure{err};
}

struct Instance {
    int dim = 0, n = 0, device = 0;
    int64_t ld = 0;
    bool truncated = false;
    hipStream_t stream = nullptr;
    double *obs = nullptr, *loc = nullptr, *saved = nullptr, *slab = nullptr, *out = nullptr, *grad = nullptr;
    double *cur = nullptr, *stored = nullptr, *hostOut = nullptr;          // pinned
    double tau = 0.0, storedTau = 0.0;
    double ssq = 0.0, tr = 0.0, storedSsq = 0.0, storedTr = 0.0;
    bool sumKnown = false, incrementsKnown = false, rowSaved = false;
    int updatedLocation = -1;
    bool deviceStale = true;         // loc differs from cur in more than one location (or nothing is known about it)
    int deviceStaleAt = -1;          // ... in this location alone
    bool movedSinceStore = false;    // an all-location update or a second single update since the last store
    long long stats[MDS_STATS_COUNT] = {0, 0, 0, 0, 0, 0};
    std::mutex mutex;

    ~Instance() {
        if (hipSetDevice(device) != hipSuccess) return;
        if (stream) (void)hipStreamSynchronize(stream);
        for (double* p : {obs, loc, saved, slab, out, grad})
            if (p) (void)hipFree(p);
        for (double* p : {cur, stored, hostOut})
            if (p) (void)hipHostFree(p);
        if (stream) (void)hipStreamDestroy(stream);
    }

    size_t points() const { return (size_t)n * (size_t)dim; }

    void uploadLocations() {
        check(hipMemcpyAsync(loc, cur, points() * sizeof(double), hipMemcpyHostToDevice, stream));
        deviceStale = false;
        deviceStaleAt = -1;
    }
    void readSums() {
        check(hipMemcpyAsync(hostOut, out, 2 * sizeof(double), hipMemcpyDeviceToHost, stream));
        check(hipStreamSynchronize(stream));
        ssq = hostOut[0];
        tr = hostOut[1];
    }
    void evaluateAll() {
        uploadLocations();
        check(mds::launchSum(stream, dim, n, obs, loc, tau, truncated, slab, out));
        readSums();
        stats[0] += 1;
        stats[3] += 2;
        stats[4] = 2;
        stats[5] = 2;
    }
    void evaluateRow(int k) {
        mds::Point x;
        for (int c = 0; c < mds::MAX_DIM; ++c) x.v[c] = c < dim ? cur[(size_t)k * dim + c] : 0.0;
        check(mds::launchRow(stream, dim, n, obs, loc, k, x, tau, truncated, ssq, tr, saved, out));
        readSums();
        deviceStaleAt = -1;
        rowSaved = true;
        stats[1] += 1;
        stats[3] += 1;
        stats[4] = 1;
        stats[5] = 1;
    }
    // calculateLogLikelihood's first half (MultiDimensionalScalingCoreImpl.java:154-163)
    void evaluate() {
        stats[4] = stats[5] = 0;
        if (sumKnown) return;
        const bool rowOnly = incrementsKnown && updatedLocation >= 0 && !deviceStale && deviceStaleAt == updatedLocation;
        try {
            if (rowOnly) {
                evaluateRow(updatedLocation);
            } else {
                evaluateAll();
                incrementsKnown = true;
            }
        } catch (...) {                                          // a failed launch or copy: nothing on the device is trusted
            deviceStale = true;
            incrementsKnown = rowSaved = false;
            throw;
        }
        sumKnown = true;
    }
    double sum() const { return 0.5 * tau * ssq + (truncated ? tr : 0.0); }
};

std::mutex g_tableMutex;
std::vector<std::shared_ptr<Instance>> g_table;

std::shared_ptr<Instance> find(int instance) {
    std::lock_guard<std::mutex> lock(g_tableMutex);
    if (instance < 0 || (size_t)instance >= g_table.size()) return nullptr;
    return g_table[(size_t)instance];
}

int codeOf(hipError_t err) { return err == hipErrorOutOfMemory ? MDS_ERROR_OUT_OF_MEMORY : MDS_ERROR_GENERAL; }

// the body of every call on an instance: look it up, take its lock, select its device, contain what is thrown
template <typename Body>
int onInstance(int instance, Body body) {
    try {
        std::shared_ptr<Instance> p = find(instance);
        if (!p) return MDS_ERROR_UNINITIALIZED_INSTANCE;
        std::lock_guard<std::mutex> lock(p->mutex);
        check(hipSetDevice(p->device));
        return body(*p);
    } catch (const HipFailure& f) {
        return codeOf(f.err);
    } catch (const std::bad_alloc&) {
        return MDS_ERROR_OUT_OF_MEMORY;
    } catch (...) {
        return MDS_ERROR_UNIDENTIFIED_EXCEPTION;
    }
}

}  // namespace

MDS_EXPORT int mdsInitialize(int dimension, int locationCount, long long flags, int deviceNumber, int /*threads*/) {
    try {
        if (dimension < 1 || locationCount < 1 || deviceNumber < -1) return MDS_ERROR_OUT_OF_RANGE;
        if (dimension > MDS_MAX_DIMENSION) return MDS_ERROR_NO_IMPLEMENTATION;
        const int device = deviceNumber < 0 ? 0 : deviceNumber;
        int count = 0;
        if (hipGetDeviceCount(&count) != hipSuccess || count < 1) {
            (void)hipGetLastError();
            return MDS_ERROR_NO_RESOURCE;
        }
        if (device >= count) return MDS_ERROR_OUT_OF_RANGE;
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, device) != hipSuccess || strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
            (void)hipGetLastError();
            return MDS_ERROR_NO_RESOURCE;                        // the kernels exist for gfx950 only
        }
        check(hipSetDevice(device));
        auto p = std::make_shared<Instance>();
        p->dim = dimension;
        p->n = locationCount;
        p->device = device;
        p->ld = mds::leadingDimension(locationCount);
        p->truncated = (flags & MDS_FLAG_LEFT_TRUNCATION) != 0;
        const size_t table = (size_t)locationCount * (size_t)p->ld, points = p->points();
        check(hipStreamCreateWithFlags(&p->stream, hipStreamNonBlocking));
        check(hipMalloc((void**)&p->obs, table * sizeof(double)));
        check(hipMalloc((void**)&p->loc, points * sizeof(double)));
        check(hipMalloc((void**)&p->grad, points * sizeof(double)));
        check(hipMalloc((void**)&p->saved, mds::MAX_DIM * sizeof(double)));
        check(hipMalloc((void**)&p->slab, 2 * mds::MAX_SUM_BLOCKS * sizeof(double)));
        check(hipMalloc((void**)&p->out, 2 * sizeof(double)));
        check(hipHostMalloc((void**)&p->cur, points * sizeof(double), hipHostMallocDefault));
        check(hipHostMalloc((void**)&p->stored, points * sizeof(double), hipHostMallocDefault));
        check(hipHostMalloc((void**)&p->hostOut, 2 * sizeof(double), hipHostMallocDefault));
        memset(p->cur, 0, points * sizeof(double));
        memset(p->stored, 0, points * sizeof(double));
        check(hipMemsetAsync(p->obs, 0, table * sizeof(double), p->stream));
        check(hipMemsetAsync(p->loc, 0, points * sizeof(double), p->stream));
        check(hipStreamSynchronize(p->stream));
        std::lock_guard<std::mutex> lock(g_tableMutex);
        g_table.push_back(p);
        return (int)g_table.size() - 1;
    } catch (const HipFailure& f) {
        return codeOf(f.err);
    } catch (const std::bad_alloc&) {
        return MDS_ERROR_OUT_OF_MEMORY;
    } catch (...) {
        return MDS_ERROR_UNIDENTIFIED_EXCEPTION;
    }
}

MDS_EXPORT int mdsInitializeLayout(int, int, int, long long, int, int) { return MDS_ERROR_NO_IMPLEMENTATION; }

MDS_EXPORT int mdsFinalize(int instance) {
    try {
        std::shared_ptr<Instance> p;
        {
            std::lock_guard<std::mutex> lock(g_tableMutex);
            if (instance < 0 || (size_t)instance >= g_table.size() || !g_table[(size_t)instance]) return MDS_ERROR_UNINITIALIZED_INSTANCE;
            p.swap(g_table[(size_t)instance]);
        }
        std::lock_guard<std::mutex> lock(p->mutex);              // a call in flight on another thread finishes first
        return MDS_SUCCESS;
    } catch (...) {
        return MDS_ERROR_UNIDENTIFIED_EXCEPTION;
    }
}

// updateLocation (MultiDimensionalScalingCoreImpl.java:122-151)
MDS_EXPORT int mdsUpdateLocations(int instance, int index, const double* values, long long length) {
    return onInstance(instance, [&](Instance& m) {
        if (index < -1 || index >= m.n) return MDS_ERROR_OUT_OF_RANGE;
        const long long need = index < 0 ? (long long)m.points() : m.dim;
        if (!values || length < need) return MDS_ERROR_OUT_OF_RANGE;
        if (m.updatedLocation != -1 || index == -1) {
            m.incrementsKnown = false;
            m.rowSaved = false;
            m.movedSinceStore = true;
        }
        if (index >= 0) {
            m.updatedLocation = index;
            memcpy(m.cur + (size_t)index * m.dim, values, (size_t)m.dim * sizeof(double));
            if (m.deviceStaleAt < 0) m.deviceStaleAt = index;
            else if (m.deviceStaleAt != index) m.deviceStale = true;
        } else {
            memcpy(m.cur, values, m.points() * sizeof(double));
            m.deviceStale = true;
        }
        m.sumKnown = false;
        return MDS_SUCCESS;
    });
}

MDS_EXPORT int mdsGetSumOfIncrements(int instance, double* outSum) {
    return onInstance(instance, [&](Instance& m) {
        if (!outSum) return MDS_ERROR_OUT_OF_RANGE;
        m.evaluate();
        *outSum = m.sum();
        return MDS_SUCCESS;
    });
}

// storeState (:176-190)
MDS_EXPORT int mdsStoreState(int instance) {
    return onInstance(instance, [&](Instance& m) {
        m.storedSsq = m.ssq;
        m.storedTr = m.tr;
        m.rowSaved = false;
        memcpy(m.stored, m.cur, m.points() * sizeof(double));
        m.updatedLocation = -1;
        m.movedSinceStore = false;
        m.storedTau = m.tau;
        return MDS_SUCCESS;
    });
}

// restoreState (:192-212): the sum and tau come back, the location pointers change places; the device gets its one moved
// location back where a row update is all that happened since the store, and is marked stale otherwise
MDS_EXPORT int mdsRestoreState(int instance) {
    return onInstance(instance, [&](Instance& m) {
        m.ssq = m.storedSsq;
        m.tr = m.storedTr;
        m.sumKnown = true;
        if (m.rowSaved && !m.movedSinceStore && !m.deviceStale && m.deviceStaleAt < 0) {
            check(hipMemcpyAsync(m.loc + (size_t)m.updatedLocation * m.dim, m.saved, (size_t)m.dim * sizeof(double), hipMemcpyDeviceToDevice,
                                 m.stream));
            m.incrementsKnown = true;
        } else {
            m.incrementsKnown = false;
            m.deviceStale = true;
        }
        m.rowSaved = false;
        std::swap(m.cur, m.stored);
        m.tau = m.storedTau;
        return MDS_SUCCESS;
    });
}

// acceptState (:214-221) copies the new row into the table's column; there is no table here
MDS_EXPORT int mdsAcceptState(int instance) {
    return onInstance(instance, [&](Instance&) { return MDS_SUCCESS; });
}

MDS_EXPORT int mdsMakeDirty(int instance) {
    return onInstance(instance, [&](Instance& m) {
        m.sumKnown = false;
        m.incrementsKnown = false;
        return MDS_SUCCESS;
    });
}

MDS_EXPORT int mdsSetPairwiseData(int instance, const double* observations, long long length) {
    return onInstance(instance, [&](Instance& m) {
        if (!observations || length < (long long)m.n * m.n) return MDS_ERROR_OUT_OF_RANGE;
        check(hipMemcpy2DAsync(m.obs, (size_t)m.ld * sizeof(double), observations, (size_t)m.n * sizeof(double), (size_t)m.n * sizeof(double),
                               (size_t)m.n, hipMemcpyHostToDevice, m.stream));
        check(hipStreamSynchronize(m.stream));
        m.sumKnown = false;
        m.incrementsKnown = false;
        return MDS_SUCCESS;
    });
}

MDS_EXPORT int mdsGetPairwiseData(int instance, double* outObservations, long long length) {
    return onInstance(instance, [&](Instance& m) {
        if (!outObservations || length < (long long)m.n * m.n) return MDS_ERROR_OUT_OF_RANGE;
        check(hipMemcpy2DAsync(outObservations, (size_t)m.n * sizeof(double), m.obs, (size_t)m.ld * sizeof(double), (size_t)m.n * sizeof(double),
                               (size_t)m.n, hipMemcpyDeviceToHost, m.stream));
        check(hipStreamSynchronize(m.stream));
        return MDS_SUCCESS;
    });
}

// setParameters (:111-119)
MDS_EXPORT int mdsSetParameters(int instance, const double* parameters, long long length) {
    return onInstance(instance, [&](Instance& m) {
        if (!parameters || length < 1) return MDS_ERROR_OUT_OF_RANGE;
        m.tau = parameters[0];
        if (m.truncated) {
            m.incrementsKnown = false;
            m.sumKnown = false;
        }
        return MDS_SUCCESS;
    });
}

MDS_EXPORT int mdsGetLocationGradient(int instance, double* outGradient, long long length) {
    return onInstance(instance, [&](Instance& m) {
        if (!outGradient || length < (long long)m.points()) return MDS_ERROR_OUT_OF_RANGE;
        // the kernel reads the device's locations: bring them up to date the way the next evaluation would
        if (!m.sumKnown) m.evaluate();
        if (m.deviceStale || m.deviceStaleAt >= 0) {
            m.uploadLocations();
            m.incrementsKnown = true;                            // the device now holds the locations the known sum belongs to
        }
        check(mds::launchGradient(m.stream, m.dim, m.n, m.obs, m.loc, m.tau, m.truncated, m.grad));
        check(hipMemcpyAsync(outGradient, m.grad, m.points() * sizeof(double), hipMemcpyDeviceToHost, m.stream));
        check(hipStreamSynchronize(m.stream));
        m.stats[2] += 1;
        m.stats[3] += 1;
        return MDS_SUCCESS;
    });
}

MDS_EXPORT int mdsGetObservationGradient(int instance, double*, long long) {
    return onInstance(instance, [&](Instance&) { return MDS_ERROR_NO_IMPLEMENTATION; });
}

MDS_EXPORT int mdsGetInternalDimension(int instance) {
    return onInstance(instance, [&](Instance& m) { return m.dim; });
}

MDS_EXPORT int mdsGetLocationCount(int instance) {
    return onInstance(instance, [&](Instance& m) { return m.n; });
}

MDS_EXPORT int mdsStats(int instance, long long* out, int count) {
    return onInstance(instance, [&](Instance& m) {
        if (!out || count < 0 || count > MDS_STATS_COUNT) return MDS_ERROR_OUT_OF_RANGE;
        for (int k = 0; k < count; ++k) out[k] = m.stats[k];
        return MDS_SUCCESS;
    });
}
