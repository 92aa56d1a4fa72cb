"""Multidimensional scaling on the device: the caller's side of ``libmds2_jni.so`` (include/mds_mi355.h).

``NativeMDS`` has the method set of ``dr.inference.multidimensionalscaling.NativeMDSSingleton`` (NativeMDSSingleton.java:134-161)
over the library's C ABI; a negative code becomes an ``MDSError`` the way the natives raise a RuntimeException.

``MultiDimensionalScalingLikelihood`` makes the calls ``MultiDimensionalScalingLikelihood`` makes through
``MassivelyParallelMDSImpl``, in its order (MultiDimensionalScalingLikelihood.java:254-268 at construction, :317-370 afterwards):
setParameters, setPairwiseData, updateLocations(-1), makeDirty; then per change one updateLocations or setParameters, and
``getLogLikelihood`` = (log tau - log 2 pi) n / 2 - getSumOfIncrements() only when something changed
(MassivelyParallelMDSImpl.java:122-127), n counted over the pairs i < j whose observation is not NaN.
"""
import ctypes as C
import math
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
MDS_LIB = os.path.join(HERE, "lib", "libmds2_jni.so")

USE_NATIVE_MDS, SINGLE_PRECISION, MULTI_CORE, OPENCL_VECTORIZATION, LEFT_TRUNCATION = 1, 4, 8, 16, 32
ERROR_OUT_OF_MEMORY, ERROR_UNINITIALIZED_INSTANCE, ERROR_OUT_OF_RANGE, ERROR_NO_RESOURCE, ERROR_NO_IMPLEMENTATION = -2, -4, -5, -6, -7
STATS = ("full_evaluations", "row_updates", "gradients", "launches", "last_launches", "last_path")
PATH_KNOWN, PATH_ROW, PATH_ALL = 0, 1, 2

_D, _LL = C.POINTER(C.c_double), C.c_longlong
ABI = {
    "mdsInitialize": [C.c_int, C.c_int, _LL, C.c_int, C.c_int],
    "mdsInitializeLayout": [C.c_int, C.c_int, C.c_int, _LL, C.c_int, C.c_int],
    "mdsFinalize": [C.c_int],
    "mdsUpdateLocations": [C.c_int, C.c_int, _D, _LL],
    "mdsGetSumOfIncrements": [C.c_int, _D],
    "mdsStoreState": [C.c_int],
    "mdsRestoreState": [C.c_int],
    "mdsAcceptState": [C.c_int],
    "mdsMakeDirty": [C.c_int],
    "mdsSetPairwiseData": [C.c_int, _D, _LL],
    "mdsGetPairwiseData": [C.c_int, _D, _LL],
    "mdsSetParameters": [C.c_int, _D, _LL],
    "mdsGetLocationGradient": [C.c_int, _D, _LL],
    "mdsGetObservationGradient": [C.c_int, _D, _LL],
    "mdsGetInternalDimension": [C.c_int],
    "mdsGetLocationCount": [C.c_int],
    "mdsStats": [C.c_int, C.POINTER(_LL), C.c_int],
}


class MDSError(RuntimeError):
    def __init__(self, function, code):
        RuntimeError.__init__(self, "%s: %d" % (function, code))
        self.function, self.code = function, code


_library = {}


def library(path=None):
    """The loaded libmds2_jni.so with every function of the C ABI typed.  A missing library is an error: there is no other
    implementation behind this module."""
    path = path or os.environ.get("MDS_MI355_LIB", MDS_LIB)
    if path not in _library:
        lib = C.CDLL(path)
        for name, argtypes in ABI.items():
            fn = getattr(lib, name)
            fn.argtypes, fn.restype = argtypes, C.c_int
        _library[path] = lib
    return _library[path]


def _doubles(values):
    a = np.ascontiguousarray(values, dtype=np.float64).reshape(-1)
    return a, a.ctypes.data_as(_D), a.size


class NativeMDS:
    """The natives' method set.  ``raw`` is the ctypes library for callers that want the codes themselves."""

    def __init__(self, path=None):
        self.raw = library(path)

    def _check(self, function, code):
        if code < 0:
            raise MDSError(function, code)
        return code

    def initialize(self, dimensionCount, locationCount, flags, deviceNumber=-1, threads=0, columnLocationCount=None):
        if columnLocationCount is not None:
            return self._check("mdsInitializeLayout", self.raw.mdsInitializeLayout(dimensionCount, locationCount, columnLocationCount, flags,
                                                                                  deviceNumber, threads))
        return self._check("mdsInitialize", self.raw.mdsInitialize(dimensionCount, locationCount, flags, deviceNumber, threads))

    def finalize(self, instance):
        self._check("mdsFinalize", self.raw.mdsFinalize(instance))

    def updateLocations(self, instance, index, locations):
        a, p, n = _doubles(locations)
        self._check("mdsUpdateLocations", self.raw.mdsUpdateLocations(instance, index, p, n))

    def getSumOfIncrements(self, instance):
        out = C.c_double(float("nan"))
        self._check("mdsGetSumOfIncrements", self.raw.mdsGetSumOfIncrements(instance, C.byref(out)))
        return out.value

    def storeState(self, instance):
        self._check("mdsStoreState", self.raw.mdsStoreState(instance))

    def restoreState(self, instance):
        self._check("mdsRestoreState", self.raw.mdsRestoreState(instance))

    def acceptState(self, instance):
        self._check("mdsAcceptState", self.raw.mdsAcceptState(instance))

    def makeDirty(self, instance):
        self._check("mdsMakeDirty", self.raw.mdsMakeDirty(instance))

    def setPairwiseData(self, instance, observations):
        a, p, n = _doubles(observations)
        self._check("mdsSetPairwiseData", self.raw.mdsSetPairwiseData(instance, p, n))

    def setParameters(self, instance, parameters):
        a, p, n = _doubles(parameters)
        self._check("mdsSetParameters", self.raw.mdsSetParameters(instance, p, n))

    def getPairwiseData(self, instance):
        n = self._check("mdsGetLocationCount", self.raw.mdsGetLocationCount(instance))
        out = np.empty(n * n, dtype=np.float64)
        self._check("mdsGetPairwiseData", self.raw.mdsGetPairwiseData(instance, out.ctypes.data_as(_D), out.size))
        return out

    def getLocationGradient(self, instance, gradient):
        """Fills `gradient` (float64, C-contiguous, at least N * D entries), as the native fills the Java array."""
        if not (isinstance(gradient, np.ndarray) and gradient.dtype == np.float64 and gradient.flags.c_contiguous):
            raise TypeError("gradient: a C-contiguous float64 array")
        self._check("mdsGetLocationGradient", self.raw.mdsGetLocationGradient(instance, gradient.ctypes.data_as(_D), gradient.size))

    def getObservationGradient(self, instance, gradient):
        self._check("mdsGetObservationGradient", self.raw.mdsGetObservationGradient(instance, gradient.ctypes.data_as(_D), gradient.size))

    def getInternalDimension(self, instance):
        return self._check("mdsGetInternalDimension", self.raw.mdsGetInternalDimension(instance))

    def stats(self, instance):
        out = (_LL * len(STATS))()
        self._check("mdsStats", self.raw.mdsStats(instance, out, len(STATS)))
        return dict(zip(STATS, (int(v) for v in out)))


def observation_count(observations):
    """Pairs i < j whose observation is not NaN."""
    y = np.asarray(observations, dtype=np.float64)
    return int(np.count_nonzero(~np.isnan(y[np.triu_indices(y.shape[0], 1)])))


class MultiDimensionalScalingLikelihood:
    def __init__(self, dimension, observations, locations, precision, left_truncated=False, flags=USE_NATIVE_MDS, device=-1,
                 native=None):
        y = np.ascontiguousarray(observations, dtype=np.float64)
        x = np.ascontiguousarray(locations, dtype=np.float64)
        if y.ndim != 2 or y.shape[0] != y.shape[1] or x.shape != (y.shape[0], dimension):
            raise ValueError("observations [N][N] and locations [N][dimension] are wanted")
        self.native = native or NativeMDS()
        self.dimension, self.location_count = dimension, y.shape[0]
        self.observation_count = observation_count(y)
        self.precision = self.stored_precision = float(precision)
        self.instance = self.native.initialize(dimension, self.location_count, flags | (LEFT_TRUNCATION if left_truncated else 0), device, 0)
        self.internal_dimension = self.native.getInternalDimension(self.instance)
        self.native.setParameters(self.instance, [self.precision])
        self.native.setPairwiseData(self.instance, y)
        self.native.updateLocations(self.instance, -1, x)
        self.log_likelihood = self.stored_log_likelihood = 0.0
        self.makeDirty()

    # -- changes (handleVariableChangedEvent) ----------------------------------------------------------------------
    def setLocation(self, k, x):
        self.native.updateLocations(self.instance, int(k), np.asarray(x, dtype=np.float64).reshape(self.dimension))
        self.likelihood_known = False

    def setLocations(self, locations):
        self.native.updateLocations(self.instance, -1, np.asarray(locations, dtype=np.float64).reshape(self.location_count, self.dimension))
        self.likelihood_known = False

    def setPrecision(self, precision):
        self.precision = float(precision)
        self.native.setParameters(self.instance, [self.precision])
        self.likelihood_known = False

    # -- the model's state ----------------------------------------------------------------------------------------
    def storeState(self):
        self.stored_log_likelihood = self.log_likelihood
        self.native.storeState(self.instance)
        self.stored_precision = self.precision

    def restoreState(self):
        self.log_likelihood = self.stored_log_likelihood
        self.likelihood_known = True
        self.native.restoreState(self.instance)
        self.precision = self.stored_precision

    def acceptState(self):
        self.native.acceptState(self.instance)

    def makeDirty(self):
        self.likelihood_known = False
        self.native.makeDirty(self.instance)

    def getLogLikelihood(self):
        if not self.likelihood_known:
            s = self.native.getSumOfIncrements(self.instance)
            self.log_likelihood = 0.5 * (math.log(self.precision) - math.log(2.0 * math.pi)) * self.observation_count - s
            self.likelihood_known = True
        return self.log_likelihood

    def getGradientLogDensity(self):
        out = np.empty(self.location_count * self.dimension, dtype=np.float64)
        self.native.getLocationGradient(self.instance, out)
        return out

    def stats(self):
        return self.native.stats(self.instance)

    def close(self):
        if self.instance is not None:
            self.native.finalize(self.instance)
            self.instance = None
