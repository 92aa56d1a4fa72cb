"""ctypes binding of the C ABI (include/beagle_mi355.h) — the Python-side stand-in for
``beagle.BeagleJNIImpl`` (lib/beagle.jar!beagle/BeagleJNIImpl.class), which wraps the JNI natives in
the ``beagle.Beagle`` interface and turns non-zero return codes into ``BeagleException``.

Method names and argument order are those of the ``beagle.Beagle`` Java interface, so test code reads
like the reference's callers (e.g. ``beagle.updatePartials(operations, operationCount, Beagle.NONE)``,
src/dr/evomodel/treelikelihood/BeagleTreeLikelihood.java:1003).

There is NO fallback: if the HIP library is missing this module raises at load time
(``BeagleFactory.loadBeagleInstance`` would fall back to a Java implementation; this engine does not).
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
ENGINE_LIB = os.path.join(_HERE, "lib", "libhmsbeagle-jni.so")
if os.environ.get("BEAGLE_MI355_ENGINE_LIB"):        # development: an A/B build of the same engine (tools/build_variant.sh)
    ENGINE_LIB = os.environ["BEAGLE_MI355_ENGINE_LIB"]
HOST_LIB = os.path.join(_HERE, "lib", "libbeast_host.so")

NONE = -1
# instance / requirement flag bits (lib/beagle.jar!beagle/BeagleFlag; include/beagle_mi355.h)
FLAG_EIGEN_REAL, FLAG_EIGEN_COMPLEX, FLAG_PROCESSOR_GPU, FLAG_FRAMEWORK_CPU = 1 << 4, 1 << 5, 1 << 16, 1 << 27
OPERATION_TUPLE_SIZE = 7

ERROR_NAMES = {0: "NO_ERROR", -1: "GENERAL_ERROR", -2: "OUT_OF_MEMORY_ERROR", -3: "UNIDENTIFIED_EXCEPTION_ERROR",
               -4: "UNINITIALIZED_INSTANCE_ERROR", -5: "OUT_OF_RANGE_ERROR", -6: "NO_RESOURCE_ERROR",
               -7: "NO_IMPLEMENTATION_ERROR", -8: "FLOATING_POINT_ERROR"}


class BeagleException(RuntimeError):
    """Mirror of beagle.BeagleException(functionName, errCode)."""

    def __init__(self, function_name, code):
        super().__init__("%s returned %d (%s)" % (function_name, code, ERROR_NAMES.get(code, "?")))
        self.function_name = function_name
        self.code = code


class InstanceDetails(C.Structure):
    _fields_ = [("resourceNumber", C.c_int), ("resourceName", C.c_char_p), ("implName", C.c_char_p),
                ("implDescription", C.c_char_p), ("flags", C.c_long)]


class _Resource(C.Structure):
    _fields_ = [("name", C.c_char_p), ("description", C.c_char_p), ("supportFlags", C.c_long),
                ("requiredFlags", C.c_long)]


class _ResourceList(C.Structure):
    _fields_ = [("list", C.POINTER(_Resource)), ("length", C.c_int)]


_DP = C.POINTER(C.c_double)
_IP = C.POINTER(C.c_int)


def _d(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.float64)


def _i(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.int32)


def _dp(a):
    return None if a is None else a.ctypes.data_as(_DP)


def _ip(a):
    return None if a is None else a.ctypes.data_as(_IP)


_PROTOS = {
    "CreateInstance": ([C.c_int] * 9 + [_IP, C.c_int, C.c_long, C.c_long, C.POINTER(InstanceDetails)], C.c_int),
    "FinalizeInstance": ([C.c_int], C.c_int),
    "SetCPUThreadCount": ([C.c_int, C.c_int], C.c_int),
    "SetPatternWeights": ([C.c_int, _DP], C.c_int),
    "SetPatternPartitions": ([C.c_int, C.c_int, _IP], C.c_int),
    "SetTipStates": ([C.c_int, C.c_int, _IP], C.c_int),
    "GetTipStates": ([C.c_int, C.c_int, _IP], C.c_int),
    "SetTipPartials": ([C.c_int, C.c_int, _DP], C.c_int),
    "SetPartials": ([C.c_int, C.c_int, _DP], C.c_int),
    "GetPartials": ([C.c_int, C.c_int, C.c_int, _DP], C.c_int),
    "GetLogScaleFactors": ([C.c_int, C.c_int, _DP], C.c_int),
    "SetEigenDecomposition": ([C.c_int, C.c_int, _DP, _DP, _DP], C.c_int),
    "SetStateFrequencies": ([C.c_int, C.c_int, _DP], C.c_int),
    "SetCategoryWeights": ([C.c_int, C.c_int, _DP], C.c_int),
    "SetCategoryRates": ([C.c_int, _DP], C.c_int),
    "SetCategoryRatesWithIndex": ([C.c_int, C.c_int, _DP], C.c_int),
    "SetTransitionMatrix": ([C.c_int, C.c_int, _DP, C.c_double], C.c_int),
    "GetTransitionMatrix": ([C.c_int, C.c_int, _DP], C.c_int),
    "ConvolveTransitionMatrices": ([C.c_int, _IP, _IP, _IP, C.c_int], C.c_int),
    "UpdateTransitionMatrices": ([C.c_int, C.c_int, _IP, _IP, _IP, _DP, C.c_int], C.c_int),
    "UpdateTransitionMatricesWithMultipleModels": ([C.c_int, _IP, _IP, _IP, _IP, _IP, _DP, C.c_int], C.c_int),
    "UpdatePartials": ([C.c_int, _IP, C.c_int, C.c_int], C.c_int),
    "UpdatePartialsByPartition": ([C.c_int, _IP, C.c_int], C.c_int),
    "WaitForPartials": ([C.c_int, _IP, C.c_int], C.c_int),
    "AccumulateScaleFactors": ([C.c_int, _IP, C.c_int, C.c_int], C.c_int),
    "AccumulateScaleFactorsByPartition": ([C.c_int, _IP, C.c_int, C.c_int, C.c_int], C.c_int),
    "RemoveScaleFactors": ([C.c_int, _IP, C.c_int, C.c_int], C.c_int),
    "RemoveScaleFactorsByPartition": ([C.c_int, _IP, C.c_int, C.c_int, C.c_int], C.c_int),
    "ResetScaleFactors": ([C.c_int, C.c_int], C.c_int),
    "ResetScaleFactorsByPartition": ([C.c_int, C.c_int, C.c_int], C.c_int),
    "CopyScaleFactors": ([C.c_int, C.c_int, C.c_int], C.c_int),
    "CalculateRootLogLikelihoods": ([C.c_int, _IP, _IP, _IP, _IP, C.c_int, _DP], C.c_int),
    "CalculateRootLogLikelihoodsByPartition": ([C.c_int, _IP, _IP, _IP, _IP, _IP, C.c_int, C.c_int, _DP, _DP], C.c_int),
    "GetSiteLogLikelihoods": ([C.c_int, _DP], C.c_int),
    "SetRootPrePartials": ([C.c_int, _IP, _IP, C.c_int], C.c_int),
    "SetDifferentialMatrix": ([C.c_int, C.c_int, _DP], C.c_int),
    "AddTransitionMatrices": ([C.c_int, _IP, _IP, _IP, C.c_int], C.c_int),
    "TransposeTransitionMatrices": ([C.c_int, _IP, _IP, C.c_int], C.c_int),
    "UpdatePrePartials": ([C.c_int, _IP, C.c_int, C.c_int], C.c_int),
    "UpdatePrePartialsByPartition": ([C.c_int, _IP, C.c_int], C.c_int),
    "CalculateEdgeDifferentials": ([C.c_int, _IP, _IP, _IP, _IP, C.c_int, _DP, _DP, _DP], C.c_int),
    "CalculateCrossProductDifferentials": ([C.c_int, _IP, _IP, _IP, _IP, _DP, C.c_int, _DP, _DP], C.c_int),
}

# symbols every engine library must export (tests assert this list against include/beagle_mi355.h)
ABI_SYMBOLS = ["beagleGetVersion", "beagleGetCitation", "beagleGetResourceList", "beagleGetBenchmarkedResourceList", "beagleGetApiTable",
               "beagleGetPartitionApiTable"] + \
              ["beagle" + k for k in _PROTOS] + \
              ["beagleMi355SetStream", "beagleMi355CalculateRootLogLikelihoodsDevice", "beagleMi355Synchronize",
               "beagleMi355KernelTimer", "beagleMi355DeviceBytes", "beagleMi355WalkStats", "beagleMi355GradientStats", "beagleMi355GetPartialsBatch", "beagleMi355SampleAncestralStates", "beagleMi355SampleMarkovJumps", "beagleMi355SampleMarkovJumpsUniformized",
               "beagleMi355SimulateSequences", "beagleMi355SimulateCompleteHistories", "beagleMi355RobustCounts", "beagleMi355SimulateUnconditionedCounts", "beagleMi355NodeHeightDerivatives", "beagleMi355UpdateDifferentialMatrices", "beagleMi355SetReversibleModels", "beagleMi355GetEigenDecomposition", "beagleMi355EigenStats", "beagleMi355UpdateTransitionMatricesFromGenerators", "beagleMi355GeneratorStats", "beagleMi355UpdateTransitionMatricesWithEpochs", "beagleMi355EpochStats", "beagleMi355NodePatternLikelihoods", "beagleMi355NodePatternStats", "beagleMi355NodePosteriors", "beagleMi355NodePosteriorStats", "beagleMi355PlacementScores", "beagleMi355PlacementStats", "beagleMi355RegraftScores", "beagleMi355RegraftStats", "beagleMi355SetTipEmission", "beagleMi355TipEmissionStats",
               "beagleMi355GetPartialsPinned", "beagleMi355GetSiteLogLikelihoodsPinned",
               "beagleMi355KernelTimerCalls", "beagleMi355WalkHealth", "beagleMi355RepeatStats", "beagleMi355RepeatSubRunStats", "beagleMi355TableOperandStats", "beagleMi355WalkLaunchInfo", "beagleMi355RootFusedCount", "beagleMi355SitePrefetchCount", "beagleMi355KernelTimerRestart", "beagleMi355GetDimensions", "beagleMi355GetCommUniqueId", "beagleMi355CommInit", "beagleMi355CommInfo", "beagleMi355CalculateRootLogLikelihoodsAllReduce"] + \
              ["beagleBasta" + k for k in ("AllocateCoalescentBuffers", "UpdatePartials", "AccumulatePartials", "GetBuffer", "GetBufferLength", "Stats", "SampleStates", "StatesStats",
                                           "Gradient", "GradientStats", "UpdatePartialsGrad", "UpdateTransitionMatricesGrad", "AccumulatePartialsGrad")]
BASTA_OPERATION_SIZE = 8


class EngineLibrary:
    """A loaded engine shared object (the HIP engine, or — in tests only — the CPU oracle, whose
    symbols carry the ``oracle_`` prefix)."""

    def __init__(self, path=ENGINE_LIB, prefix=""):
        if not os.path.exists(path):
            raise OSError("engine library %s is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(there is no CPU fallback)" % path)
        self.path = path
        self.prefix = prefix
        self.lib = C.CDLL(path, mode=C.RTLD_LOCAL)
        self.fn = {}
        for name, (argtypes, restype) in _PROTOS.items():
            f = getattr(self.lib, prefix + "beagle" + name, None)
            if f is None:
                continue
            f.argtypes = argtypes
            f.restype = restype
            self.fn[name] = f
        gv = getattr(self.lib, prefix + "beagleGetVersion")
        gv.restype = C.c_char_p
        self.version = gv().decode()
        tab = getattr(self.lib, prefix + "beagleGetApiTable")
        tab.restype = C.c_void_p
        self.api_table = tab()
        ptab = getattr(self.lib, prefix + "beagleGetPartitionApiTable", None)       # (the engine; the oracle restates no ...ByPartition call)
        self.partition_api_table = None
        if ptab is not None:
            ptab.restype = C.c_void_p
            self.partition_api_table = ptab()

    def has(self, name):
        return name in self.fn

    def resource_list(self):
        f = getattr(self.lib, self.prefix + "beagleGetResourceList")
        f.restype = C.POINTER(_ResourceList)
        rl = f().contents
        return [(rl.list[i].name.decode(), rl.list[i].description.decode(), rl.list[i].supportFlags)
                for i in range(rl.length)]


_engine = None


def engine():
    """The HIP engine library (loaded once)."""
    global _engine
    if _engine is None:
        _engine = EngineLibrary(ENGINE_LIB)
    return _engine


class Beagle:
    """One engine instance behind the ``beagle.Beagle`` method set."""

    NONE = NONE
    OPERATION_TUPLE_SIZE = OPERATION_TUPLE_SIZE

    def __init__(self, tipCount, partialsBufferCount, compactBufferCount, stateCount, patternCount,
                 eigenBufferCount, matrixBufferCount, categoryCount, scaleBufferCount,
                 resourceList=(1,), preferenceFlags=0, requirementFlags=0, library=None):
        self.lib = library or engine()
        self._f = self.lib.fn
        self.stateCount, self.patternCount, self.categoryCount = stateCount, patternCount, categoryCount
        self.eigenComplex = bool(requirementFlags & FLAG_EIGEN_COMPLEX)          # (eigenvalue arrays are [S real | S imaginary parts])
        self.details = InstanceDetails()
        rl = _i(list(resourceList)) if resourceList is not None else None
        h = self._f["CreateInstance"](tipCount, partialsBufferCount, compactBufferCount, stateCount, patternCount,
                                      eigenBufferCount, matrixBufferCount, categoryCount, scaleBufferCount,
                                      _ip(rl), 0 if rl is None else len(rl), preferenceFlags, requirementFlags,
                                      C.byref(self.details))
        if h < 0:
            raise BeagleException("create", h)
        self.instance = h

    def _check(self, name, rc):
        if rc != 0:
            raise BeagleException(name, rc)

    def finalize(self):
        if self.instance >= 0:
            self._check("finalize", self._f["FinalizeInstance"](self.instance))
            self.instance = -1

    def setCPUThreadCount(self, n):
        self._check("setCPUThreadCount", self._f["SetCPUThreadCount"](self.instance, n))

    def setPatternWeights(self, w):
        w = _d(w)
        assert w.size >= self.patternCount
        self._check("setPatternWeights", self._f["SetPatternWeights"](self.instance, _dp(w)))

    def setPatternPartitions(self, partitionCount, partitions):
        a = _i(partitions)
        self._check("setPatternPartitions", self._f["SetPatternPartitions"](self.instance, partitionCount, _ip(a)))

    def setTipStates(self, tipIndex, states):
        a = _i(states)
        assert a.size >= self.patternCount
        self._check("setTipStates", self._f["SetTipStates"](self.instance, tipIndex, _ip(a)))

    def getTipStates(self, tipIndex):
        out = np.empty(self.patternCount, dtype=np.int32)
        self._check("getTipStates", self._f["GetTipStates"](self.instance, tipIndex, _ip(out)))
        return out

    def setTipPartials(self, tipIndex, partials):
        a = _d(partials)
        assert a.size >= self.patternCount * self.stateCount
        self._check("setTipPartials", self._f["SetTipPartials"](self.instance, tipIndex, _dp(a)))

    def setPartials(self, bufferIndex, partials):
        a = _d(partials)
        assert a.size >= self.patternCount * self.stateCount * self.categoryCount
        self._check("setPartials", self._f["SetPartials"](self.instance, bufferIndex, _dp(a)))

    @classmethod
    def attach(cls, tl):
        """This binding on the instance a host driver (treelikelihood.BeagleTreeLikelihood) already owns."""
        raw = cls.__new__(cls)
        raw.lib, raw._f, raw.instance = tl.engine, tl.engine.fn, tl.instance
        raw.stateCount, raw.patternCount, raw.categoryCount = tl.state_count, tl.pattern_count, tl.category_count
        return raw

    def getPartials(self, bufferIndex, scaleIndex=NONE):
        out = np.empty(self.categoryCount * self.patternCount * self.stateCount)
        self._check("getPartials", self._f["GetPartials"](self.instance, bufferIndex, scaleIndex, _dp(out)))
        return out.reshape(self.categoryCount, self.patternCount, self.stateCount)

    def getLogScaleFactors(self, scaleIndex):
        out = np.empty(self.patternCount)
        self._check("getLogScaleFactors", self._f["GetLogScaleFactors"](self.instance, scaleIndex, _dp(out)))
        return out

    def setEigenDecomposition(self, eigenIndex, eigenVectors, inverseEigenValues, eigenValues):
        u, ui, lam = _d(eigenVectors), _d(inverseEigenValues), _d(eigenValues)
        self._check("setEigenDecomposition",
                    self._f["SetEigenDecomposition"](self.instance, eigenIndex, _dp(u), _dp(ui), _dp(lam)))

    def setStateFrequencies(self, index, freqs):
        a = _d(freqs)
        self._check("setStateFrequencies", self._f["SetStateFrequencies"](self.instance, index, _dp(a)))

    def setCategoryWeights(self, index, weights):
        a = _d(weights)
        self._check("setCategoryWeights", self._f["SetCategoryWeights"](self.instance, index, _dp(a)))

    def setCategoryRates(self, rates):
        a = _d(rates)
        self._check("setCategoryRates", self._f["SetCategoryRates"](self.instance, _dp(a)))

    def setCategoryRatesWithIndex(self, index, rates):
        a = _d(rates)
        self._check("setCategoryRatesWithIndex", self._f["SetCategoryRatesWithIndex"](self.instance, index, _dp(a)))

    def setTransitionMatrix(self, matrixIndex, matrix, paddedValue=1.0):
        a = _d(matrix)
        self._check("setTransitionMatrix", self._f["SetTransitionMatrix"](self.instance, matrixIndex, _dp(a), paddedValue))

    def getTransitionMatrix(self, matrixIndex):
        out = np.empty(self.categoryCount * self.stateCount * self.stateCount)
        self._check("getTransitionMatrix", self._f["GetTransitionMatrix"](self.instance, matrixIndex, _dp(out)))
        return out.reshape(self.categoryCount, self.stateCount, self.stateCount)

    def convolveTransitionMatrices(self, first, second, result, count):
        a, b, c = _i(first), _i(second), _i(result)
        self._check("convolveTransitionMatrices",
                    self._f["ConvolveTransitionMatrices"](self.instance, _ip(a), _ip(b), _ip(c), count))

    def updateTransitionMatrices(self, eigenIndex, probabilityIndices, firstDerivativeIndices,
                                 secondDerivativeIndices, edgeLengths, count):
        p, d1, d2, t = _i(probabilityIndices), _i(firstDerivativeIndices), _i(secondDerivativeIndices), _d(edgeLengths)
        self._check("updateTransitionMatrices",
                    self._f["UpdateTransitionMatrices"](self.instance, eigenIndex, _ip(p), _ip(d1), _ip(d2), _dp(t), count))

    def updateTransitionMatricesWithMultipleModels(self, eigenIndices, categoryRateIndices, probabilityIndices,
                                                   firstDerivativeIndices, secondDerivativeIndices, edgeLengths, count):
        e, r, p = _i(eigenIndices), _i(categoryRateIndices), _i(probabilityIndices)
        d1, d2, t = _i(firstDerivativeIndices), _i(secondDerivativeIndices), _d(edgeLengths)
        self._check("updateTransitionMatricesWithMultipleModels",
                    self._f["UpdateTransitionMatricesWithMultipleModels"](self.instance, _ip(e), _ip(r), _ip(p),
                                                                           _ip(d1), _ip(d2), _dp(t), count))

    def updatePartials(self, operations, operationCount, cumulativeScaleIndex=NONE):
        a = _i(operations)
        assert a.size >= operationCount * OPERATION_TUPLE_SIZE
        self._check("updatePartials", self._f["UpdatePartials"](self.instance, _ip(a), operationCount, cumulativeScaleIndex))

    def updatePartialsByPartition(self, operations, operationCount):
        a = _i(operations)
        assert a.size >= operationCount * 9
        self._check("updatePartialsByPartition", self._f["UpdatePartialsByPartition"](self.instance, _ip(a), operationCount))

    def waitForPartials(self, destinationPartials, destinationPartialsCount):
        a = _i(destinationPartials)
        self._check("waitForPartials", self._f["WaitForPartials"](self.instance, _ip(a), destinationPartialsCount))

    def accumulateScaleFactors(self, scaleIndices, count, cumulativeScaleIndex):
        a = _i(scaleIndices)
        self._check("accumulateScaleFactors",
                    self._f["AccumulateScaleFactors"](self.instance, _ip(a), count, cumulativeScaleIndex))

    def removeScaleFactors(self, scaleIndices, count, cumulativeScaleIndex):
        a = _i(scaleIndices)
        self._check("removeScaleFactors", self._f["RemoveScaleFactors"](self.instance, _ip(a), count, cumulativeScaleIndex))

    def resetScaleFactors(self, cumulativeScaleIndex):
        self._check("resetScaleFactors", self._f["ResetScaleFactors"](self.instance, cumulativeScaleIndex))

    def copyScaleFactors(self, dest, src):
        self._check("copyScaleFactors", self._f["CopyScaleFactors"](self.instance, dest, src))

    def accumulateScaleFactorsByPartition(self, scaleIndices, count, cumulativeScaleIndex, partitionIndex):
        a = _i(scaleIndices)
        self._check("accumulateScaleFactorsByPartition",
                    self._f["AccumulateScaleFactorsByPartition"](self.instance, _ip(a), count, cumulativeScaleIndex, partitionIndex))

    def resetScaleFactorsByPartition(self, cumulativeScaleIndex, partitionIndex):
        self._check("resetScaleFactorsByPartition",
                    self._f["ResetScaleFactorsByPartition"](self.instance, cumulativeScaleIndex, partitionIndex))

    def calculateRootLogLikelihoods(self, bufferIndices, categoryWeightsIndices, stateFrequenciesIndices,
                                    cumulativeScaleIndices, count, outSumLogLikelihood):
        """``outSumLogLikelihood``: writable sequence of length >= 1 (as the Java double[1]).
        Error -8 (FLOATING_POINT) is tolerated exactly as BeagleJNIImpl#calculateRootLogLikelihoods does."""
        b, w, f, s = _i(bufferIndices), _i(categoryWeightsIndices), _i(stateFrequenciesIndices), _i(cumulativeScaleIndices)
        out = np.zeros(1)
        rc = self._f["CalculateRootLogLikelihoods"](self.instance, _ip(b), _ip(w), _ip(f), _ip(s), count, _dp(out))
        outSumLogLikelihood[0] = out[0]
        if rc != 0 and rc != -8:
            raise BeagleException("calculateRootLogLikelihoods", rc)

    def calculateRootLogLikelihoodsByPartition(self, bufferIndices, categoryWeightsIndices, stateFrequenciesIndices,
                                               cumulativeScaleIndices, partitionIndices, partitionCount, count,
                                               outSumLogLikelihoodByPartition, outSumLogLikelihood):
        b, w, f = _i(bufferIndices), _i(categoryWeightsIndices), _i(stateFrequenciesIndices)
        s, p = _i(cumulativeScaleIndices), _i(partitionIndices)
        byp = np.zeros(partitionCount * count)
        tot = np.zeros(1)
        rc = self._f["CalculateRootLogLikelihoodsByPartition"](self.instance, _ip(b), _ip(w), _ip(f), _ip(s), _ip(p),
                                                               partitionCount, count, _dp(byp), _dp(tot))
        outSumLogLikelihoodByPartition[:len(byp)] = byp
        outSumLogLikelihood[0] = tot[0]
        if rc != 0 and rc != -8:
            raise BeagleException("calculateRootLogLikelihoodsByPartition", rc)

    # ---- pre-order partials and branch gradients (AbstractBeagleGradientDelegate / ...BranchGradientDelegate) ----
    def setRootPrePartials(self, bufferIndices, stateFrequenciesIndices, count):
        b, f = _i(bufferIndices), _i(stateFrequenciesIndices)
        self._check("setRootPrePartials", self._f["SetRootPrePartials"](self.instance, _ip(b), _ip(f), count))

    def setDifferentialMatrix(self, matrixIndex, matrix):
        m = _d(matrix)
        assert m.size == self.stateCount * self.stateCount * self.categoryCount
        self._check("setDifferentialMatrix", self._f["SetDifferentialMatrix"](self.instance, matrixIndex, _dp(m)))

    def transposeTransitionMatrices(self, inputIndices, resultIndices, count):
        a, b = _i(inputIndices), _i(resultIndices)
        self._check("transposeTransitionMatrices",
                    self._f["TransposeTransitionMatrices"](self.instance, _ip(a), _ip(b), count))

    def updatePrePartials(self, operations, operationCount, cumulativeScaleIndex=NONE):
        ops = _i(operations)
        self._check("updatePrePartials", self._f["UpdatePrePartials"](self.instance, _ip(ops), operationCount,
                                                                     cumulativeScaleIndex))

    def updatePrePartialsByPartition(self, operations, operationCount):
        """9-int tuples {pre(child), writeScale, readScale, pre(parent), matrix(child), post(sibling), matrix(sibling), partition,
        cumulativeScale}"""
        ops = _i(operations)
        self._check("updatePrePartialsByPartition", self._f["UpdatePrePartialsByPartition"](self.instance, _ip(ops), operationCount))

    def addTransitionMatrices(self, first, second, result, count):
        a, b, c = _i(first), _i(second), _i(result)
        self._check("addTransitionMatrices", self._f["AddTransitionMatrices"](self.instance, _ip(a), _ip(b), _ip(c), count))

    def calculateEdgeDifferentials(self, postBufferIndices, preBufferIndices, derivativeMatrixIndices,
                                   categoryWeightsIndices, count, want_per_pattern=False, want_squared=True):
        """-> (outSumDerivatives[count], outSumSquaredDerivatives[count] or None, outDerivatives[count, P] or None); the two
        optional outputs are passed as NULL when not wanted, as the gradient delegates do
        (AbstractBeagleBranchGradientDelegate.java:82-92)."""
        po, pr, dm, cw = _i(postBufferIndices), _i(preBufferIndices), _i(derivativeMatrixIndices), _i(categoryWeightsIndices)
        s1 = np.zeros(count)
        s2 = np.zeros(count) if want_squared else None
        per = np.zeros((count, self.patternCount)) if want_per_pattern else None
        self._check("calculateEdgeDifferentials",
                    self._f["CalculateEdgeDifferentials"](self.instance, _ip(po), _ip(pr), _ip(dm), _ip(cw), count,
                                                          _dp(per) if per is not None else None, _dp(s1),
                                                          _dp(s2) if s2 is not None else None))
        return s1, s2, per

    def calculateCrossProductDifferentials(self, postBufferIndices, preBufferIndices, categoryRateIndices,
                                           categoryWeightsIndices, edgeLengths, count, out=None):
        """-> outSumDerivatives[S*S] (accumulated into ``out`` when given, as BEAST's zero-filled array)."""
        po, pr = _i(postBufferIndices), _i(preBufferIndices)
        cr, cw, t = _i(categoryRateIndices), _i(categoryWeightsIndices), _d(edgeLengths)
        acc = np.zeros(self.stateCount * self.stateCount) if out is None else out
        self._check("calculateCrossProductDifferentials",
                    self._f["CalculateCrossProductDifferentials"](self.instance, _ip(po), _ip(pr), _ip(cr), _ip(cw), _dp(t),
                                                                  count, _dp(acc), None))
        return acc

    def getSiteLogLikelihoods(self, out=None):
        if out is None:
            out = np.empty(self.patternCount)
        self._check("getSiteLogLikelihoods", self._f["GetSiteLogLikelihoods"](self.instance, _dp(out)))
        return out

    # --- MI355X extensions -----------------------------------------------------------------
    def _ext(self, name, argtypes, restype=C.c_int):
        f = getattr(self.lib.lib, name)
        f.argtypes = argtypes
        f.restype = restype
        return f

    def setStream(self, hip_stream):
        self._check("setStream", self._ext("beagleMi355SetStream", [C.c_int, C.c_void_p])(self.instance, hip_stream))

    def calculateRootLogLikelihoodsDevice(self, bufferIndex, categoryWeightsIndex, stateFrequenciesIndex,
                                          cumulativeScaleIndex, device_ptr):
        f = self._ext("beagleMi355CalculateRootLogLikelihoodsDevice", [C.c_int] * 5 + [C.c_void_p])
        self._check("calculateRootLogLikelihoodsDevice",
                    f(self.instance, bufferIndex, categoryWeightsIndex, stateFrequenciesIndex, cumulativeScaleIndex, device_ptr))

    def synchronize(self):
        self._check("synchronize", self._ext("beagleMi355Synchronize", [C.c_int])(self.instance))

    # one process per GPU: the collective inside the engine (include/beagle_mi355.h)
    def commUniqueId(self):
        """128 bytes that identify a new communicator; produced on ONE rank and handed to all (any channel)."""
        buf = C.create_string_buffer(128)
        self._check("getCommUniqueId", self._ext("beagleMi355GetCommUniqueId", [C.c_void_p])(buf))
        return buf.raw

    def commInit(self, unique_id, rank, rank_count):
        buf = C.create_string_buffer(bytes(unique_id), 128)
        self._check("commInit", self._ext("beagleMi355CommInit", [C.c_int, C.c_void_p, C.c_int, C.c_int])(self.instance, buf, rank, rank_count))

    def commRanks(self):
        """Ranks of the instance's communicator as RCCL counts them (0: none) — include/beagle_mi355.h beagleMi355CommInfo."""
        n = C.c_int(0)
        self._check("commInfo", self._ext("beagleMi355CommInfo", [C.c_int, C.POINTER(C.c_int)])(self.instance, C.byref(n)))
        return n.value

    def calculateRootLogLikelihoodsAllReduce(self, bufferIndex, categoryWeightsIndex, stateFrequenciesIndex, cumulativeScaleIndex):
        out = C.c_double(0.0)
        f = self._ext("beagleMi355CalculateRootLogLikelihoodsAllReduce", [C.c_int] * 5 + [C.POINTER(C.c_double)])
        rc = f(self.instance, bufferIndex, categoryWeightsIndex, stateFrequenciesIndex, cumulativeScaleIndex, C.byref(out))
        if rc not in (0, -8):
            self._check("calculateRootLogLikelihoodsAllReduce", rc)
        return out.value

    def kernelTimer(self, enable):
        ms = C.c_double(0.0)
        n = C.c_long(0)
        f = self._ext("beagleMi355KernelTimer", [C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_long)])
        self._check("kernelTimer", f(self.instance, int(enable), C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def kernelTimerRestart(self):
        """Forget what the enabled kernel timer and the walk counters hold (no synchronisation: the caller has just done one)."""
        self._check("kernelTimerRestart", self._ext("beagleMi355KernelTimerRestart", [C.c_int])(self.instance))

    def kernelTimerCalls(self):
        """updatePartials calls the kernel timer bracketed since this was last asked (kernelTimer(N > 1) samples every N-th)."""
        n = C.c_long(0)
        self._check("kernelTimerCalls", self._ext("beagleMi355KernelTimerCalls", [C.c_int, C.POINTER(C.c_long)])(self.instance, C.byref(n)))
        return n.value

    def rootFusedCount(self):
        """calculateRootLogLikelihoods calls answered inside the walk's launch (include/beagle_mi355.h beagleMi355RootFusedCount)."""
        n = C.c_long(0)
        self._check("rootFusedCount", self._ext("beagleMi355RootFusedCount", [C.c_int, C.POINTER(C.c_long)])(self.instance, C.byref(n)))
        return n.value

    def sitePrefetchCount(self):
        """getSiteLogLikelihoods calls that found the values already on the host (include/beagle_mi355.h beagleMi355SitePrefetchCount)."""
        n = C.c_long(0)
        self._check("sitePrefetchCount", self._ext("beagleMi355SitePrefetchCount", [C.c_int, C.POINTER(C.c_long)])(self.instance, C.byref(n)))
        return n.value

    def getPartialsBatch(self, bufferIndices, scaleIndices=None):
        """-> [count][C][P][S]: several buffers in one call (include/beagle_mi355.h beagleMi355GetPartialsBatch)."""
        b = _i(list(bufferIndices))
        sc = None if scaleIndices is None else _i(list(scaleIndices))
        out = np.empty(len(b) * self.categoryCount * self.patternCount * self.stateCount)
        f = self._ext("beagleMi355GetPartialsBatch", [C.c_int, _IP, _IP, C.c_int, _DP])
        self._check("getPartialsBatch", f(self.instance, _ip(b), _ip(sc), len(b), _dp(out)))
        return out.reshape(len(b), self.categoryCount, self.patternCount, self.stateCount)

    def sampleAncestralStates(self, nodes, categoryWeightsIndex, stateFrequenciesIndex, seed, map=False):
        """One draw of every listed node's state per pattern on the device (include/beagle_mi355.h beagleMi355SampleAncestralStates).
        ``nodes``: [nodeCount][3] rows {bufferIndex, matrixIndex, parentRow}, the root first.  -> (states uint8 [nodeCount, P],
        categories int32 [P]).  A draw whose total weight was not finite and > 0 raises BeagleException with code -8
        (FLOATING_POINT_ERROR)."""
        rows = _i(nodes).reshape(-1, 3)
        states = np.empty((rows.shape[0], self.patternCount), dtype=np.uint8)
        cats = np.zeros(self.patternCount, dtype=np.int32)
        f = self._ext("beagleMi355SampleAncestralStates", [C.c_int, _IP, C.c_int, C.c_int, C.c_int, C.c_ulonglong, C.c_int,
                                                           C.c_void_p, _IP])
        self._check("sampleAncestralStates", f(self.instance, _ip(rows), rows.shape[0], categoryWeightsIndex, stateFrequenciesIndex,
                                               int(seed) & 0xFFFFFFFFFFFFFFFF, 1 if map else 0, states.ctypes.data, _ip(cats)))
        return states, cats

    def simulateSequences(self, rows, site_count, weights_index, freqs_index, seed, root_states=None, rate_categories=None):
        """An alignment drawn from the model down the tree on the device (include/beagle_mi355.h beagleMi355SimulateSequences).
        ``rows``: [nodeCount][3] rows {outRow, matrixIndex, parentRow}, the root first; outRow -1: the node's states are not
        returned.  ``root_states`` ([site_count], each < stateCount) and ``rate_categories`` ([site_count], each < categoryCount)
        replace the root's draw and the category draw.  -> (states uint8 [1 + max outRow, site_count], categories int32
        [site_count]).  A draw from a vector whose total was not finite and > 0 raises BeagleException with code -8."""
        rows = _i(rows).reshape(-1, 3)
        site_count = int(site_count)
        n_out = int(rows[:, 0].max()) + 1 if rows.shape[0] else 0
        if n_out < 1 or site_count < 1:
            raise BeagleException("simulateSequences", -5)
        states = np.zeros((n_out, site_count), dtype=np.uint8)
        cats = np.zeros(site_count, dtype=np.int32)
        root = None if root_states is None else np.ascontiguousarray(root_states, dtype=np.uint8)
        given = None if rate_categories is None else _i(rate_categories)
        if (root is not None and root.size != site_count) or (given is not None and given.size != site_count):
            raise ValueError("root_states and rate_categories must have one entry per site")
        f = self._ext("beagleMi355SimulateSequences", [C.c_int, _IP, C.c_int, C.c_int, C.c_int, C.c_int, C.c_ulonglong, C.c_int,
                                                       C.c_void_p, _IP, C.c_void_p, _IP])
        self._check("simulateSequences", f(self.instance, _ip(rows), rows.shape[0], site_count, weights_index, freqs_index,
                                           int(seed) & 0xFFFFFFFFFFFFFFFF, 0, None if root is None else root.ctypes.data, _ip(given),
                                           states.ctypes.data, _ip(cats)))
        return states, cats

    def simulateCompleteHistories(self, rows, site_count, branchLengths, infinitesimalMatrices, registers, registerFlags, seed,
                                  nodeHeights=None, categoryRatesIndex=0, categoryWeightsIndex=0, stateFrequenciesIndex=0,
                                  root_states=None, rate_categories=None, states=True, values=True, row_totals=True, site_totals=True,
                                  history=False, event_capacity=None, retry=True):
        """One substitution history per (branch, site), simulated down the tree on the device (include/beagle_mi355.h
        beagleMi355SimulateCompleteHistories).  ``rows``: [nodeCount][3] rows {outRow, qIndex, parentRow}, the root first;
        ``branchLengths`` [nodeCount] (branch rate x time); ``infinitesimalMatrices`` [qCount][S][S]; ``registers`` [K][S][S];
        ``registerFlags`` [K] (JUMPS_REWARDS) or None; ``nodeHeights`` [nodeCount] (needed with ``history``).  -> dict of what was
        asked for: "states" uint8 [1 + max outRow, site_count] and "categories" int32 [site_count], "values" [K, nodeCount,
        site_count], "row_totals" [K, nodeCount], "site_totals" [K, site_count]; with ``history``: "event_counts" int32 [nodeCount,
        site_count], "event_heights" [E], "event_states" uint8 [E, 2], "event_total".  The event buffer starts at ``event_capacity``
        (default: a guess) and the call is made once more with the exact size when it was too small (``retry``; without it a full
        buffer returns the other outputs and "rc" = -5 instead of raising).  A history cut at 100 000 jumps or a failed draw raises
        BeagleException with code -8."""
        rows = _i(rows).reshape(-1, 3)
        n, S, site_count = rows.shape[0], self.stateCount, int(site_count)
        Q = _d(infinitesimalMatrices).reshape(-1, S, S)
        regs = _d(registers).reshape(-1, S, S)
        K = regs.shape[0]
        flags = None if registerFlags is None else _i(registerFlags).reshape(-1)
        lengths = _d(branchLengths).reshape(-1)
        heights = None if nodeHeights is None else _d(nodeHeights).reshape(-1)
        root = None if root_states is None else np.ascontiguousarray(root_states, dtype=np.uint8)
        given = None if rate_categories is None else _i(rate_categories)
        if lengths.shape[0] != n or (heights is not None and heights.shape[0] != n) or (flags is not None and flags.shape[0] != K):
            raise ValueError("branchLengths, nodeHeights and registerFlags must have one entry per row / register")
        if (root is not None and root.size != site_count) or (given is not None and given.size != site_count):
            raise ValueError("root_states and rate_categories must have one entry per site")
        n_out = int(rows[:, 0].max()) + 1 if n else 0
        if site_count < 1 or n < 1 or (states and n_out < 1):
            raise BeagleException("simulateCompleteHistories", -5)
        capacity = int(event_capacity) if event_capacity is not None else n * site_count // 4 + 1024
        f = self._ext("beagleMi355SimulateCompleteHistories",
                      [C.c_int, _IP, C.c_int, C.c_int, _DP, C.c_void_p, _DP, C.c_int, C.c_int, C.c_int, C.c_int, _DP, C.c_void_p,
                       C.c_int, C.c_ulonglong, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                       C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p, C.c_void_p])
        for attempt in range(2):
            out = {}
            if states:
                out["states"] = np.zeros((n_out, site_count), dtype=np.uint8)
                out["categories"] = np.zeros(site_count, dtype=np.int32)
            if values:
                out["values"] = np.empty((K, n, site_count))
            if row_totals:
                out["row_totals"] = np.empty((K, n))
            if site_totals:
                out["site_totals"] = np.empty((K, site_count))
            if history:
                out["event_counts"] = np.empty((n, site_count), dtype=np.int32)
                out["event_heights"] = np.empty(capacity)
                out["event_states"] = np.empty((capacity, 2), dtype=np.uint8)
            total = C.c_longlong(0)

            def ptr(key):
                return out[key].ctypes.data if key in out else None

            rc = f(self.instance, _ip(rows), n, site_count, _dp(lengths), None if heights is None else heights.ctypes.data, _dp(Q),
                   Q.shape[0], categoryRatesIndex, categoryWeightsIndex, stateFrequenciesIndex, _dp(regs),
                   None if flags is None else flags.ctypes.data, K, int(seed) & 0xFFFFFFFFFFFFFFFF, 0,
                   None if root is None else root.ctypes.data, None if given is None else given.ctypes.data, ptr("states"),
                   ptr("categories"), ptr("values"), ptr("row_totals"), ptr("site_totals"), ptr("event_counts"),
                   capacity if history else 0, ptr("event_heights"), ptr("event_states"), C.byref(total) if history else None)
            if rc == -5 and history and total.value > capacity:
                if retry and attempt == 0:
                    capacity = int(total.value)
                    continue
                if not retry:
                    out["rc"] = rc
                    rc = 0
            break
        self._check("simulateCompleteHistories", rc)
        if history:
            out["event_total"] = int(total.value)
            out["event_heights"] = out["event_heights"][:total.value]
            out["event_states"] = out["event_states"][:total.value]
        return out

    def setTipEmission(self, tipIndex, codes, emission):
        """A tip whose partials are the lookup ``emission[codes[p]]`` (include/beagle_mi355.h beagleMi355SetTipEmission): ``emission``
        [K][S], ``codes`` [P] ints (one outside 0..K-1: missing) or None to keep the codes of the previous call and replace the table."""
        e = _d(emission).reshape(-1, self.stateCount)
        c = None if codes is None else _i(codes)
        if c is not None and c.size < self.patternCount:
            raise ValueError("codes must have one entry per pattern")
        f = self._ext("beagleMi355SetTipEmission", [C.c_int, C.c_int, _IP, C.c_int, _DP])
        self._check("setTipEmission", f(self.instance, tipIndex, _ip(c), e.shape[0], _dp(e)))

    def tipEmissionStats(self):
        """Tips with an emission table (include/beagle_mi355.h beagleMi355TipEmissionStats)."""
        out = (C.c_long * 4)()
        self._check("tipEmissionStats", self._ext("beagleMi355TipEmissionStats", [C.c_int, C.POINTER(C.c_long)])(self.instance, out))
        return {"folded": int(out[0]), "expanded": int(out[1]), "fold_launches": int(out[2]), "demotions": int(out[3])}

    def nodeHeightDerivatives(self, nodes, rates, categoryWeightsIndex=0, first=True, second=True):
        """d lnL / d h and d^2 lnL / d h^2 of the listed internal nodes in one call, from the partials on the device
        (include/beagle_mi355.h beagleMi355NodeHeightDerivatives).  ``nodes``: [nodeCount][8] rows {pre(i), post(j), matrix(j),
        dmatrix(j), post(k), matrix(k), dmatrix(k), dmatrix(i)} (dmatrix(i) = -1 at the root); ``rates``: [nodeCount][3] rows
        {r_j, r_k, r_i}.  -> (first, second), each [nodeCount] or None when not asked for.  A result that is not finite raises
        BeagleException with code -8."""
        rows = _i(nodes).reshape(-1, 8)
        r = _d(rates).reshape(-1, 3)
        if r.shape[0] != rows.shape[0]:
            raise ValueError("rates must have one row {r_j, r_k, r_i} per node")
        n = rows.shape[0]
        o1 = np.zeros(n) if first else None
        o2 = np.zeros(n) if second else None
        f = self._ext("beagleMi355NodeHeightDerivatives", [C.c_int, _IP, _DP, C.c_int, C.c_int, _DP, _DP])
        self._check("nodeHeightDerivatives", f(self.instance, _ip(rows), _dp(r), n, categoryWeightsIndex, _dp(o1), _dp(o2)))
        return o1, o2

    DIFFERENTIAL_EXACT, DIFFERENTIAL_FIRST_ORDER = 0, 1

    def updateDifferentialMatrices(self, eigenIndices, categoryRatesIndices, differentials, differentialIndices, matrixIndices,
                                   edgeLengths, count=None, mode=0):
        """The differential matrix of every listed branch and category, formed on the device in one call (include/beagle_mi355.h
        beagleMi355UpdateDifferentialMatrices).  ``differentials`` [D][S][S]: dQ / d theta; per branch its eigen system, rate set
        and differential (each None: 0 for all), the matrix slot it writes and length x clock rate; ``mode``: DIFFERENTIAL_EXACT
        (D = U (V o Phi) U^-1, so that dP / d theta = P D) or DIFFERENTIAL_FIRST_ORDER (D = dist x dQ)."""
        S = self.stateCount
        q = _d(differentials).reshape(-1, S, S)
        e, r, d, m, t = _i(eigenIndices), _i(categoryRatesIndices), _i(differentialIndices), _i(matrixIndices), _d(edgeLengths)
        n = m.size if count is None else int(count)
        for a in (e, r, d, m, t):
            if a is not None and a.size < n:
                raise ValueError("every per-branch list must have one entry per branch")
        f = self._ext("beagleMi355UpdateDifferentialMatrices", [C.c_int, _IP, _IP, _DP, C.c_int, _IP, _IP, _DP, C.c_int, C.c_int])
        self._check("updateDifferentialMatrices", f(self.instance, _ip(e), _ip(r), _dp(q), q.shape[0], _ip(d), _ip(m), _dp(t), n, int(mode)))

    def setReversibleModels(self, eigenIndices, relativeRates, frequencies):
        """The eigen systems of time-reversible models, decomposed on the device in one call (include/beagle_mi355.h
        beagleMi355SetReversibleModels): model k — ``relativeRates[k]`` [S (S - 1) / 2], the upper triangle in row order, and
        ``frequencies[k]`` [S] — into eigen slot ``eigenIndices[k]``, which then holds what setEigenDecomposition would have been
        handed.  Nothing comes back and the host does not wait."""
        S = self.stateCount
        e = _i(eigenIndices).reshape(-1)
        r = _d(relativeRates).reshape(-1, S * (S - 1) // 2) if S > 1 else _d(np.zeros((e.size, 0)))
        f = _d(frequencies).reshape(-1, S)
        if r.shape[0] != e.size or f.shape[0] != e.size:
            raise ValueError("one row of rates and one of frequencies per eigen index")
        fn = self._ext("beagleMi355SetReversibleModels", [C.c_int, _IP, C.c_int, _DP, _DP, C.c_int])
        self._check("setReversibleModels", fn(self.instance, _ip(e), e.size, _dp(r), _dp(f), 0))

    def getEigenDecomposition(self, eigenIndex, complex_eigen=None):
        """-> (U [S][S], U^-1 [S][S], eigenvalues [S], or [2 S] on an EIGEN_COMPLEX instance) of an eigen slot, however it was filled
        (include/beagle_mi355.h beagleMi355GetEigenDecomposition).  Drains the instance's stream.  ``complex_eigen``: for a binding
        attached to an instance it did not create (default: as this binding created it)."""
        S = self.stateCount
        if complex_eigen is None:
            complex_eigen = getattr(self, "eigenComplex", False)
        u, ui, lam = np.empty((S, S)), np.empty((S, S)), np.empty(2 * S if complex_eigen else S)
        fn = self._ext("beagleMi355GetEigenDecomposition", [C.c_int, C.c_int, _DP, _DP, _DP])
        self._check("getEigenDecomposition", fn(self.instance, eigenIndex, _dp(u), _dp(ui), _dp(lam)))
        return u, ui, lam

    def eigenStats(self):
        """What setReversibleModels has done (include/beagle_mi355.h beagleMi355EigenStats)."""
        out = (C.c_longlong * 4)()
        self._check("eigenStats", self._ext("beagleMi355EigenStats", [C.c_int, C.POINTER(C.c_longlong)])(self.instance, out))
        return {"calls": int(out[0]), "models": int(out[1]), "max_sweeps": int(out[2]), "capped": int(out[3])}

    def updateTransitionMatricesFromGenerators(self, generators, generatorIndices, categoryRateIndices, probabilityIndices,
                                               edgeLengths, count=None):
        """exp(Q d) for every listed branch and category straight from the generators, no eigen system (include/beagle_mi355.h
        beagleMi355UpdateTransitionMatricesFromGenerators).  ``generators`` [G][S][S]: what getInfinitesimalMatrix returns; per
        entry its generator and rate set (each None: 0 for all), the matrix slot it writes and its edge length.  Nothing comes
        back and the host does not wait."""
        S = self.stateCount
        q = _d(generators).reshape(-1, S, S)
        g, r, m, t = _i(generatorIndices), _i(categoryRateIndices), _i(probabilityIndices), _d(edgeLengths)
        n = m.size if count is None else int(count)
        for a in (g, r, m, t):
            if a is not None and a.size < n:
                raise ValueError("every per-entry list must have one entry per matrix")
        f = self._ext("beagleMi355UpdateTransitionMatricesFromGenerators", [C.c_int, _DP, C.c_int, _IP, _IP, _IP, _DP, C.c_int])
        self._check("updateTransitionMatricesFromGenerators", f(self.instance, _dp(q), q.shape[0], _ip(g), _ip(r), _ip(m), _dp(t), n))

    def generatorStats(self):
        """What updateTransitionMatricesFromGenerators has done (include/beagle_mi355.h beagleMi355GeneratorStats)."""
        out = (C.c_long * 4)()
        self._check("generatorStats", self._ext("beagleMi355GeneratorStats", [C.c_int, C.POINTER(C.c_long)])(self.instance, out))
        return {"calls": int(out[0]), "matrices": int(out[1]), "max_squarings": int(out[2]), "refused": int(out[3])}

    def updateTransitionMatricesWithEpochs(self, segmentOffsets, segmentEigenIndices, segmentLengths, categoryRateIndices,
                                           probabilityIndices, count=None, flags=0):
        """The branch matrices of an epoch model in one call: slot probabilityIndices[e] receives the product of the transition
        matrices of segments segmentOffsets[e] .. segmentOffsets[e + 1] - 1, root end first (include/beagle_mi355.h
        beagleMi355UpdateTransitionMatricesWithEpochs).  Per segment its eigen slot and length, per entry its rate set (None: 0
        for all) and slot.  Nothing comes back and the host does not wait."""
        o, e, t = _i(segmentOffsets), _i(segmentEigenIndices), _d(segmentLengths)
        r, m = _i(categoryRateIndices), _i(probabilityIndices)
        n = m.size if count is None else int(count)
        if o.size < n + 1 or m.size < n or (r is not None and r.size < n):
            raise ValueError("count + 1 offsets, one slot (and one rate set) per entry")
        if n > 0 and (e.size < o[n] or t.size < o[n]):
            raise ValueError("one eigen index and one length per segment")
        f = self._ext("beagleMi355UpdateTransitionMatricesWithEpochs", [C.c_int, _IP, _IP, _DP, _IP, _IP, C.c_int, C.c_int])
        self._check("updateTransitionMatricesWithEpochs", f(self.instance, _ip(o), _ip(e), _dp(t), _ip(r), _ip(m), n, int(flags)))

    def epochStats(self):
        """What updateTransitionMatricesWithEpochs has done (include/beagle_mi355.h beagleMi355EpochStats)."""
        out = (C.c_long * 4)()
        self._check("epochStats", self._ext("beagleMi355EpochStats", [C.c_int, C.POINTER(C.c_long)])(self.instance, out))
        return {"calls": int(out[0]), "matrices": int(out[1]), "segments": int(out[2]), "longest": int(out[3])}

    def nodePatternLikelihoods(self, nodes, nodeLogWeights, deathState, categoryWeightsIndex=0, stateFrequenciesIndex=0,
                               node_terms=False, flags=0):
        """The stochastic Dollo node-pattern likelihood of every pattern in one call (include/beagle_mi355.h
        beagleMi355NodePatternLikelihoods).  ``nodes``: [nodeCount][4] rows {bufferIndex, scaleBufferIndex, child1Row, child2Row}
        in post-order (a tip: both child rows -1); ``nodeLogWeights`` [nodeCount].  -> (log pattern values [P], node terms
        [nodeCount, P] or None, the pattern-weighted sum, return code): the code is 0, or -8 (FLOATING_POINT) when the sum is not
        finite — the arrays are written either way; every other code raises BeagleException."""
        rows = _i(nodes).reshape(-1, 4)
        w = _d(nodeLogWeights)
        if w.size < rows.shape[0]:
            raise ValueError("one log weight per row")
        log_pattern = np.empty(self.patternCount)
        terms = np.empty((rows.shape[0], self.patternCount)) if node_terms else None
        total = C.c_double(0.0)
        f = self._ext("beagleMi355NodePatternLikelihoods", [C.c_int, _IP, _DP, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _DP, _DP,
                                                            C.POINTER(C.c_double)])
        rc = f(self.instance, _ip(rows), _dp(w), rows.shape[0], deathState, categoryWeightsIndex, stateFrequenciesIndex, flags,
               _dp(log_pattern), _dp(terms), C.byref(total))
        if rc != 0 and rc != -8:
            raise BeagleException("nodePatternLikelihoods", rc)
        return log_pattern, terms, total.value, rc

    def nodePatternStats(self):
        """What nodePatternLikelihoods has done (include/beagle_mi355.h beagleMi355NodePatternStats)."""
        out = (C.c_long * 4)()
        self._check("nodePatternStats", self._ext("beagleMi355NodePatternStats", [C.c_int, C.POINTER(C.c_long)])(self.instance, out))
        return {"calls": int(out[0]), "rows": int(out[1]), "empty_patterns": int(out[2]), "materialised": int(out[3])}

    def nodePosteriors(self, nodes, categoryWeightsIndex=0, full=True, map=False, totals=False, categories=False, flags=0, out=None):
        """Marginal state posteriors of every listed node and pattern in one call (include/beagle_mi355.h
        beagleMi355NodePosteriors).  ``nodes``: [nodeCount][2] rows {post-order buffer, pre-order buffer}.  -> (dict of what was
        asked for, return code): "posteriors" [nodeCount, P, S] (full), "map_states" uint8 [nodeCount, P] and "map_probabilities"
        [nodeCount, P] (map), "totals" [nodeCount, S] (totals), "categories" [P, C] of the first row (categories).  The code is 0,
        or -8 (FLOATING_POINT) when some pattern's likelihood was 0 or not finite — the arrays are written either way, NaN there;
        every other code raises BeagleException.  ``out``: a dict this method returned for the same shape — its arrays are
        written again instead of new ones (a caller that asks every step)."""
        rows = _i(nodes).reshape(-1, 2)
        n, P, S = rows.shape[0], self.patternCount, self.stateCount
        shapes = {}
        if full:
            shapes["posteriors"] = ((n, P, S), np.float64)
        if map:
            shapes["map_states"] = ((n, P), np.uint8)
            shapes["map_probabilities"] = ((n, P), np.float64)
        if totals:
            shapes["totals"] = ((n, S), np.float64)
        if categories:
            shapes["categories"] = ((P, self.categoryCount), np.float64)
        old, out = out or {}, {}
        for key, (shape, dtype) in shapes.items():
            a = old.get(key)
            reuse = a is not None and a.shape == shape and a.dtype == dtype and a.flags.c_contiguous and a.flags.writeable
            out[key] = a if reuse else np.empty(shape, dtype=dtype)
        ms = out.get("map_states")
        f = self._ext("beagleMi355NodePosteriors", [C.c_int, _IP, C.c_int, C.c_int, C.c_int, _DP, C.POINTER(C.c_ubyte), _DP, _DP, _DP])
        rc = f(self.instance, _ip(rows), n, categoryWeightsIndex, int(flags), _dp(out.get("posteriors")),
               ms.ctypes.data_as(C.POINTER(C.c_ubyte)) if ms is not None else None, _dp(out.get("map_probabilities")),
               _dp(out.get("totals")), _dp(out.get("categories")))
        if rc != 0 and rc != -8:
            raise BeagleException("nodePosteriors", rc)
        return out, rc

    def nodePosteriorStats(self):
        """What nodePosteriors has done (include/beagle_mi355.h beagleMi355NodePosteriorStats)."""
        out = (C.c_long * 4)()
        self._check("nodePosteriorStats", self._ext("beagleMi355NodePosteriorStats", [C.c_int, C.POINTER(C.c_long)])(self.instance, out))
        return {"calls": int(out[0]), "rows": int(out[1]), "materialised": int(out[2]), "launches": int(out[3])}

    def placementScores(self, candidates, sitePatterns, queryCodes, codeTable, categoryWeightsIndex=0, flags=0, log_table=False):
        """Scores of attaching every query at every candidate in one call (include/beagle_mi355.h beagleMi355PlacementScores).
        ``candidates``: [candidateCount][7] rows {parentPre, siblingPost, siblingMatrix, childPost, upperMatrix, lowerMatrix,
        pendantMatrix}; ``sitePatterns`` [siteCount] (-1 skips a site); ``queryCodes`` uint8 [queryCount][siteCount] (255 = missing);
        ``codeTable`` [codeCount][S].  -> (scores [queryCount, candidateCount], log table [candidateCount, P, codeCount] or None,
        return code): the code is 0, or -8 (FLOATING_POINT) when some pattern's likelihood was 0 or not finite — the arrays are
        written either way, NaN there; every other code raises BeagleException."""
        rows = _i(candidates).reshape(-1, 7)
        sites = _i(sitePatterns).reshape(-1)
        codes = np.ascontiguousarray(queryCodes, dtype=np.uint8).reshape(-1, max(1, sites.shape[0]))
        table = np.ascontiguousarray(codeTable, dtype=np.float64).reshape(-1, self.stateCount)
        K, Q, X = rows.shape[0], codes.shape[0], table.shape[0]
        scores = np.empty((Q, K), dtype=np.float64)
        logs = np.empty((K, self.patternCount, X), dtype=np.float64) if log_table else None
        f = self._ext("beagleMi355PlacementScores", [C.c_int, _IP, C.c_int, C.c_int, _IP, C.c_int, C.POINTER(C.c_ubyte), C.c_int, _DP, C.c_int,
                                                     C.c_int, _DP, _DP])
        rc = f(self.instance, _ip(rows), K, categoryWeightsIndex, _ip(sites), sites.shape[0], codes.ctypes.data_as(C.POINTER(C.c_ubyte)), Q,
               _dp(table), X, int(flags), _dp(scores), _dp(logs))
        if rc != 0 and rc != -8:
            raise BeagleException("placementScores", rc)
        return scores, logs, rc

    def placementStats(self):
        """What placementScores has done (include/beagle_mi355.h beagleMi355PlacementStats)."""
        out = (C.c_long * 4)()
        self._check("placementStats", self._ext("beagleMi355PlacementStats", [C.c_int, C.POINTER(C.c_long)])(self.instance, out))
        return {"calls": int(out[0]), "candidates": int(out[1]), "materialised": int(out[2]), "launches": int(out[3])}

    def regraftScores(self, candidates, subtree, subtree_scale=NONE, categoryWeightsIndex=0, flags=0, pattern_log_ratios=False):
        """Scores of hanging a pruned subtree at every candidate in one call (include/beagle_mi355.h beagleMi355RegraftScores).
        ``candidates``: [candidateCount][7] rows as for placementScores; ``subtree``: the post-order buffer of the subtree's root;
        ``subtree_scale``: the scale buffer with its accumulated factors, or NONE.  -> (scores [candidateCount], R [candidateCount, P]
        or None, return code): the code is 0, or -8 (FLOATING_POINT) when some pattern's likelihood was 0 or not finite — the arrays
        are written either way, NaN there; every other code raises BeagleException."""
        rows = _i(candidates).reshape(-1, 7)
        K = rows.shape[0]
        scores = np.empty(K, dtype=np.float64)
        ratios = np.empty((K, self.patternCount), dtype=np.float64) if pattern_log_ratios else None
        f = self._ext("beagleMi355RegraftScores", [C.c_int, _IP, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _DP, _DP])
        rc = f(self.instance, _ip(rows), K, int(subtree), int(subtree_scale), int(categoryWeightsIndex), int(flags), _dp(scores), _dp(ratios))
        if rc != 0 and rc != -8:
            raise BeagleException("regraftScores", rc)
        return scores, ratios, rc

    def regraftStats(self):
        """What regraftScores has done (include/beagle_mi355.h beagleMi355RegraftStats)."""
        out = (C.c_long * 4)()
        self._check("regraftStats", self._ext("beagleMi355RegraftStats", [C.c_int, C.POINTER(C.c_long)])(self.instance, out))
        return {"calls": int(out[0]), "candidates": int(out[1]), "materialised": int(out[2]), "launches": int(out[3])}

    def sampleMarkovJumps(self, nodes, branchTimes, branchRates, eigenIndex, categoryRatesIndex, categoryWeightsIndex,
                          stateFrequenciesIndex, registers, registerFlags, seed, map=False, states=False, jumps=False,
                          pattern_totals=True, row_totals=True):
        """One ancestral draw plus the expected Markov-jump counts / rewards of every register on every row and pattern
        (include/beagle_mi355.h beagleMi355SampleMarkovJumps).  ``nodes``: as for sampleAncestralStates; ``branchTimes`` [nodeCount]
        (parent height - child height), ``branchRates`` [nodeCount] or None (all 1); ``registers`` [K][S][S]; ``registerFlags`` [K]
        (JUMPS_REWARDS | JUMPS_SCALE_BY_TIME).  -> dict of what was asked for: "states" uint8 [nodeCount, P] and "categories"
        int32 [P] (states=True), "jumps" [K, nodeCount, P], "pattern_totals" [K, P], "row_totals" [K, nodeCount].  A failed draw
        or a value that is not finite raises BeagleException with code -8."""
        rows = _i(nodes).reshape(-1, 3)
        n, P = rows.shape[0], self.patternCount
        regs = _d(registers).reshape(-1, self.stateCount, self.stateCount)
        K = regs.shape[0]
        flags = _i(registerFlags).reshape(-1)
        times = _d(branchTimes).reshape(-1)
        rates = None if branchRates is None else _d(branchRates).reshape(-1)
        if times.shape[0] != n or (rates is not None and rates.shape[0] != n) or flags.shape[0] != K:
            raise ValueError("branchTimes, branchRates and registerFlags must have one entry per row / register")
        out = {}
        if states:
            out["states"] = np.empty((n, P), dtype=np.uint8)
            out["categories"] = np.zeros(P, dtype=np.int32)
        if jumps:
            out["jumps"] = np.empty((K, n, P))
        if pattern_totals:
            out["pattern_totals"] = np.empty((K, P))
        if row_totals:
            out["row_totals"] = np.empty((K, n))

        def ptr(key):
            return out[key].ctypes.data if key in out else None

        f = self._ext("beagleMi355SampleMarkovJumps", [C.c_int, _IP, C.c_int, _DP, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                                       _DP, _IP, C.c_int, C.c_ulonglong, C.c_int, C.c_void_p, C.c_void_p,
                                                       C.c_void_p, C.c_void_p, C.c_void_p])
        self._check("sampleMarkovJumps", f(self.instance, _ip(rows), n, _dp(times), None if rates is None else rates.ctypes.data,
                                           eigenIndex, categoryRatesIndex, categoryWeightsIndex, stateFrequenciesIndex, _dp(regs),
                                           _ip(flags), K, int(seed) & 0xFFFFFFFFFFFFFFFF, 1 if map else 0, ptr("states"),
                                           ptr("categories"), ptr("jumps"), ptr("pattern_totals"), ptr("row_totals")))
        return out

    def robustCounts(self, others, nodes, branchLengths, eigenVectors, inverseEigenVectors, eigenValues, infinitesimalMatrix, registers,
                     seeds, categoryWeightsIndices=(0, 0, 0), stateFrequenciesIndices=(0, 0, 0), map=False, include_rows=None,
                     states=False, counts=False, site_totals=True, branch_totals=True, tables=False):
        """Codon robust counts over three 4-state instances in one call (include/beagle_mi355.h beagleMi355RobustCounts): this
        instance is codon position 1, ``others`` the two Beagle objects of positions 2 and 3.  ``nodes`` [3][nodeCount][3]: a node
        list per position as for sampleAncestralStates; ``branchLengths`` [nodeCount] (branch rate x time); the 64-state product
        chain's eigen system and Q; ``registers`` [K][64][64]; ``seeds`` [3]; ``include_rows`` [nodeCount] or None (all).  -> dict of
        what was asked for: "states" uint8 [3, nodeCount, P], "counts" [K, nodeCount, P], "site_totals" [K, P], "branch_totals"
        [K, nodeCount], "tables" [K, nodeCount, 64, 64].  A failed draw or a gathered value that is not finite raises
        BeagleException with code -8."""
        rows = _i(nodes).reshape(3, -1, 3)
        n, P = rows.shape[1], self.patternCount
        regs = _d(registers).reshape(-1, 64, 64)
        K = regs.shape[0]
        tau = _d(branchLengths).reshape(-1)
        if tau.shape[0] != n:
            raise ValueError("branchLengths must have one entry per row")
        U, Ui, lam, Q = _d(eigenVectors).reshape(64, 64), _d(inverseEigenVectors).reshape(64, 64), _d(eigenValues).reshape(64), \
            _d(infinitesimalMatrix).reshape(64, 64)
        handles = _i([self.instance] + [o.instance for o in others])
        w, fr = _i(list(categoryWeightsIndices)), _i(list(stateFrequenciesIndices))
        sd = np.array([int(x) & 0xFFFFFFFFFFFFFFFF for x in seeds], dtype=np.uint64)
        if handles.size != 3 or w.size != 3 or fr.size != 3 or sd.size != 3:
            raise ValueError("three instances, weight indices, frequency indices and seeds")
        inc = None if include_rows is None else np.ascontiguousarray(include_rows, dtype=np.uint8)
        if inc is not None and inc.size != n:
            raise ValueError("include_rows must have one entry per row")
        out = {}
        if states:
            out["states"] = np.empty((3, n, P), dtype=np.uint8)
        if counts:
            out["counts"] = np.empty((K, n, P))
        if site_totals:
            out["site_totals"] = np.empty((K, P))
        if branch_totals:
            out["branch_totals"] = np.empty((K, n))
        if tables:
            out["tables"] = np.empty((K, n, 64, 64))

        def ptr(key):
            return out[key].ctypes.data if key in out else None

        f = self._ext("beagleMi355RobustCounts", [_IP, _IP, C.c_int, _IP, _IP, C.c_void_p, C.c_int, _DP, _DP, _DP, _DP, _DP, _DP, C.c_int,
                                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p])
        self._check("robustCounts", f(_ip(handles), _ip(rows), n, _ip(w), _ip(fr), sd.ctypes.data, 1 if map else 0, _dp(tau), _dp(U),
                                      _dp(Ui), _dp(lam), _dp(Q), _dp(regs), K, None if inc is None else inc.ctypes.data, ptr("states"),
                                      ptr("counts"), ptr("site_totals"), ptr("branch_totals"), ptr("tables")))
        return out

    def simulateUnconditionedCounts(self, infinitesimalMatrix, startFrequencies, lengths, site_count, registers, seed, counts=True,
                                    totals=True):
        """One unconditional Gillespie history per (length, site) on the device (include/beagle_mi355.h
        beagleMi355SimulateUnconditionedCounts); the instance only names the device.  ``infinitesimalMatrix`` [S][S], S = 2..64;
        ``startFrequencies`` [S]; ``lengths`` [L]; ``registers`` [K][S][S].  -> dict: "counts" [K, L, site_count], "totals" [K, L].
        A history cut at 100 000 jumps or a failed draw raises BeagleException with code -8."""
        Q = _d(infinitesimalMatrix)
        S = int(round(np.sqrt(Q.size)))
        Q = Q.reshape(S, S)
        pi = _d(startFrequencies).reshape(-1)
        regs = _d(registers).reshape(-1, S, S)
        ln = _d(lengths).reshape(-1)
        if pi.shape[0] != S:
            raise ValueError("startFrequencies must have one entry per state")
        K, L, site_count = regs.shape[0], ln.shape[0], int(site_count)
        out = {}
        if counts:
            out["counts"] = np.empty((K, L, max(site_count, 0)))
        if totals:
            out["totals"] = np.empty((K, L))
        f = self._ext("beagleMi355SimulateUnconditionedCounts", [C.c_int, C.c_int, _DP, _DP, _DP, C.c_int, C.c_int, _DP, C.c_int,
                                                                 C.c_ulonglong, C.c_void_p, C.c_void_p])
        self._check("simulateUnconditionedCounts", f(self.instance, S, _dp(Q), _dp(pi), _dp(ln), L, site_count, _dp(regs), K,
                                                     int(seed) & 0xFFFFFFFFFFFFFFFF,
                                                     out["counts"].ctypes.data if counts else None,
                                                     out["totals"].ctypes.data if totals else None))
        return out

    def sampleMarkovJumpsUniformized(self, nodes, branchTimes, branchRates, nodeHeights, infinitesimalMatrix, categoryRatesIndex,
                                     categoryWeightsIndex, stateFrequenciesIndex, registers, registerFlags, seed, simulants=1,
                                     map=False, states=False, jumps=False, pattern_totals=True, row_totals=True, history=False,
                                     event_capacity=None, retry=True):
        """One ancestral draw plus SAMPLED Markov-jump counts / rewards by uniformization (include/beagle_mi355.h
        beagleMi355SampleMarkovJumpsUniformized).  Arguments as for sampleMarkovJumps, and ``nodeHeights`` [nodeCount] (row order;
        needed with ``history``), ``infinitesimalMatrix`` Q [S][S], ``simulants`` (1..1024).  -> dict as sampleMarkovJumps returns,
        and "fallbacks" (histories that took the reference's uniform-event fallback); with ``history``: "event_counts" int32
        [nodeCount, P], "event_heights" [E], "event_states" uint8 [E, 2], "event_total".  The event buffer starts at
        ``event_capacity`` (default: a guess) and the call is made once more with the exact size when it was too small (``retry``;
        without it a full buffer returns the other outputs and "rc" = -5 instead of raising)."""
        rows = _i(nodes).reshape(-1, 3)
        n, P, S = rows.shape[0], self.patternCount, self.stateCount
        regs = _d(registers).reshape(-1, S, S)
        K = regs.shape[0]
        flags = _i(registerFlags).reshape(-1)
        times = _d(branchTimes).reshape(-1)
        rates = None if branchRates is None else _d(branchRates).reshape(-1)
        heights = None if nodeHeights is None else _d(nodeHeights).reshape(-1)
        Q = _d(infinitesimalMatrix).reshape(S, S)
        if times.shape[0] != n or (rates is not None and rates.shape[0] != n) or flags.shape[0] != K or \
                (heights is not None and heights.shape[0] != n):
            raise ValueError("branchTimes, branchRates, nodeHeights and registerFlags must have one entry per row / register")
        capacity = int(event_capacity) if event_capacity is not None else n * P // 4 + 1024
        f = self._ext("beagleMi355SampleMarkovJumpsUniformized",
                      [C.c_int, _IP, C.c_int, _DP, C.c_void_p, C.c_void_p, _DP, C.c_int, C.c_int, C.c_int, _DP, _IP, C.c_int,
                       C.c_int, C.c_ulonglong, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                       C.c_longlong, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p])
        for attempt in range(2):
            out = {}
            if states:
                out["states"] = np.empty((n, P), dtype=np.uint8)
                out["categories"] = np.zeros(P, dtype=np.int32)
            if jumps:
                out["jumps"] = np.empty((K, n, P))
            if pattern_totals:
                out["pattern_totals"] = np.empty((K, P))
            if row_totals:
                out["row_totals"] = np.empty((K, n))
            if history:
                out["event_counts"] = np.empty((n, P), dtype=np.int32)
                out["event_heights"] = np.empty(capacity)
                out["event_states"] = np.empty((capacity, 2), dtype=np.uint8)
            total, fallbacks = C.c_longlong(0), C.c_longlong(0)

            def ptr(key):
                return out[key].ctypes.data if key in out else None

            rc = f(self.instance, _ip(rows), n, _dp(times), None if rates is None else rates.ctypes.data,
                   None if heights is None else heights.ctypes.data, _dp(Q), categoryRatesIndex, categoryWeightsIndex,
                   stateFrequenciesIndex, _dp(regs), _ip(flags), K, int(simulants), int(seed) & 0xFFFFFFFFFFFFFFFF, 1 if map else 0,
                   ptr("states"), ptr("categories"), ptr("jumps"), ptr("pattern_totals"), ptr("row_totals"), ptr("event_counts"),
                   capacity if history else 0, ptr("event_heights"), ptr("event_states"), C.byref(total) if history else None,
                   C.byref(fallbacks))
            if rc == -5 and history and total.value > capacity:
                if retry and attempt == 0:
                    capacity = int(total.value)
                    continue
                if not retry:
                    out["rc"] = rc
                    rc = 0
            break
        self._check("sampleMarkovJumpsUniformized", rc)
        out["fallbacks"] = int(fallbacks.value)
        if history:
            out["event_total"] = int(total.value)
            out["event_heights"] = out["event_heights"][:total.value]
            out["event_states"] = out["event_states"][:total.value]
        return out

    # BASTA structured coalescent (beagle.basta.BeagleBasta; include/beagle_mi355.h beagleBasta*)
    def allocateCoalescentBuffers(self, bufferCount, maxCoalescentIntervalCount, partialsBufferCount, initial, threadCount=-1):
        f = self._ext("beagleBastaAllocateCoalescentBuffers", [C.c_int] * 6)
        self._check("allocateCoalescentBuffers",
                    f(self.instance, bufferCount, maxCoalescentIntervalCount, partialsBufferCount, initial, threadCount))

    def updateBastaPartials(self, operations, operationCount, intervals, intervalCount, populationSizesIndex,
                            coalescentProbabilityIndex):
        ops, iv = _i(operations), _i(intervals)
        f = self._ext("beagleBastaUpdatePartials", [C.c_int, _IP, C.c_int, _IP, C.c_int, C.c_int, C.c_int])
        self._check("updateBastaPartials", f(self.instance, _ip(ops), operationCount, _ip(iv), intervalCount,
                                             populationSizesIndex, coalescentProbabilityIndex))

    def accumulateBastaPartials(self, operations, operationCount, intervals, intervalCount, intervalLengths,
                                populationSizesIndex, coalescentProbabilityIndex, result):
        """``result`` (a float64 array) is in/out: the log-density is ADDED to result[0]."""
        ops, iv, ln = _i(operations), _i(intervals), _d(intervalLengths)
        assert isinstance(result, np.ndarray) and result.dtype == np.float64 and result.flags.c_contiguous
        f = self._ext("beagleBastaAccumulatePartials", [C.c_int, _IP, C.c_int, _IP, C.c_int, _DP, C.c_int, C.c_int, _DP])
        self._check("accumulateBastaPartials", f(self.instance, _ip(ops), operationCount, _ip(iv), intervalCount, _dp(ln),
                                                 populationSizesIndex, coalescentProbabilityIndex, _dp(result)))

    def getBastaBuffer(self, index):
        n = self._ext("beagleBastaGetBufferLength", [C.c_int, C.c_int])(self.instance, index)
        if n < 0:
            raise BeagleException("getBastaBuffer", n)
        out = np.empty(n)
        self._check("getBastaBuffer", self._ext("beagleBastaGetBuffer", [C.c_int, C.c_int, _DP])(self.instance, index, _dp(out)))
        return out

    def bastaStats(self):
        """(uploads of an operation list, updates run as one launch, updates run interval by interval, partialsBufferCount)"""
        out = (C.c_long * 4)()
        self._check("bastaStats", self._ext("beagleBastaStats", [C.c_int, C.POINTER(C.c_long)])(self.instance, out))
        return tuple(out)

    BASTA_STATES_AS_WRITTEN = 2

    def sampleBastaStates(self, operations, operationCount, intervals, intervalCount, stateFrequenciesIndex, replicateCount, seed,
                          flags=0, partialsBufferCount=None, states=True, occupancy=False, changes=False):
        """beagleBastaSampleStates -> {"states": uint8 [replicateCount][partialsBufferCount], "occupancy": [intervalCount - 1][S],
        "changes": [S][S], "bad": a draw met a total that is not finite and positive} (the arrays that were asked for)."""
        ops, iv = _i(operations), _i(intervals)
        if partialsBufferCount is None:
            partialsBufferCount = self.bastaStats()[3]
        s = self.stateCount
        out = {}
        if states:
            out["states"] = np.empty((max(replicateCount, 0), partialsBufferCount), dtype=np.uint8)
        if occupancy:
            out["occupancy"] = np.zeros((max(intervalCount - 1, 0), s))
        if changes:
            out["changes"] = np.zeros((s, s))
        f = self._ext("beagleBastaSampleStates", [C.c_int, _IP, C.c_int, _IP, C.c_int, C.c_int, C.c_int, C.c_ulonglong, C.c_int,
                                                  C.c_void_p, _DP, _DP])
        rc = f(self.instance, _ip(ops), operationCount, _ip(iv), intervalCount, stateFrequenciesIndex, replicateCount,
               seed & 0xFFFFFFFFFFFFFFFF, flags, out["states"].ctypes.data if states else None,
               _dp(out["occupancy"]) if occupancy else None, _dp(out["changes"]) if changes else None)
        out["bad"] = rc == -8
        if not out["bad"]:
            self._check("sampleBastaStates", rc)
        return out

    def bastaStatesStats(self):
        """(sampleBastaStates calls, launches of the last one per chunk of replicates, its chunks, its chains)"""
        out = (C.c_long * 4)()
        self._check("bastaStatesStats", self._ext("beagleBastaStatesStats", [C.c_int, C.POINTER(C.c_long)])(self.instance, out))
        return tuple(out)

    def bastaGradient(self, operations, operationCount, intervals, intervalCount, intervalLengths, intervalDistances,
                      populationSizesIndex, coalescentProbabilityIndex, flags=0, partialsBufferCount=None, population_sizes=True,
                      migration=True, adjoints=False):
        """beagleBastaGradient -> {"theta": [S] (with respect to 1 / size), "migration": [S][S], "adjoints": [partialsBufferCount][S],
        "bad": a returned value is not finite} (the arrays that were asked for)."""
        ops, iv, ln = _i(operations), _i(intervals), _d(intervalLengths)
        dist = None if intervalDistances is None else _d(intervalDistances)
        if partialsBufferCount is None:
            partialsBufferCount = self.bastaStats()[3]
        s = self.stateCount
        out = {}
        if population_sizes:
            out["theta"] = np.zeros(s)
        if migration:
            out["migration"] = np.zeros((s, s))
        if adjoints:
            out["adjoints"] = np.zeros((partialsBufferCount, s))
        f = self._ext("beagleBastaGradient", [C.c_int, _IP, C.c_int, _IP, C.c_int, _DP, _DP, C.c_int, C.c_int, C.c_int, _DP, _DP, _DP])
        rc = f(self.instance, _ip(ops), operationCount, _ip(iv), intervalCount, _dp(ln), None if dist is None else _dp(dist),
               populationSizesIndex, coalescentProbabilityIndex, flags, _dp(out["theta"]) if population_sizes else None,
               _dp(out["migration"]) if migration else None, _dp(out["adjoints"]) if adjoints else None)
        out["bad"] = rc == -8
        if not out["bad"]:
            self._check("bastaGradient", rc)
        return out

    def bastaGradientStats(self):
        """(bastaGradient calls, kernel launches of the last one, its levels of coalescences, its chains)"""
        out = (C.c_long * 4)()
        self._check("bastaGradientStats", self._ext("beagleBastaGradientStats", [C.c_int, C.POINTER(C.c_long)])(self.instance, out))
        return tuple(out)

    def walkStats(self):
        """Counters of the 4-state pattern walk since the last kernelTimer call (include/beagle_mi355.h)."""
        out = (C.c_long * 8)()
        self._check("walkStats", self._ext("beagleMi355WalkStats", [C.c_int, C.POINTER(C.c_long)])(self.instance, out))
        keys = ("micro_ops", "stored", "mem_reads", "tip_reads", "scale_reads", "walks", "scale_writes", "fast_walks")
        stats = {k: int(out[i]) for i, k in enumerate(keys)}
        rep = self.repeatStats()      # clades evaluated once per distinct sub-pattern: the counters above stay those of full-width vectors
        stats.update({k: rep[k] for k in ("table_rows", "table_reads", "repeat_clades")})
        return stats

    def repeatStats(self):
        """Repeated sub-patterns (include/beagle_mi355.h beagleMi355RepeatStats): the first three since the last kernelTimer call."""
        out = (C.c_long * 10)()
        self._check("repeatStats", self._ext("beagleMi355RepeatStats", [C.c_int, C.POINTER(C.c_long)])(self.instance, out))
        keys = ("table_rows", "table_reads", "repeat_clades", "table_bytes", "clades_indexed", "index_host_us", "two_table_nodes",
                "tables_under_definitions", "index_host_bytes", "index_resets")
        return {k: int(out[i]) for i, k in enumerate(keys)}

    def repeatSubRunStats(self):
        """Plain clades taken from class tables inside definitions that are not taken whole, since the last kernelTimer call
        (include/beagle_mi355.h beagleMi355RepeatSubRunStats)."""
        out = (C.c_long * 2)()
        self._check("repeatSubRunStats", self._ext("beagleMi355RepeatSubRunStats", [C.c_int, C.POINTER(C.c_long)])(self.instance, out))
        return {"sub_runs": int(out[0]), "sub_run_micro_ops": int(out[1])}

    def tableOperandStats(self):
        """Class-table operands in the assembly loop's programs since the last kernelTimer call (include/beagle_mi355.h beagleMi355TableOperandStats)."""
        out = (C.c_long * 4)()
        self._check("tableOperandStats", self._ext("beagleMi355TableOperandStats", [C.c_int, C.POINTER(C.c_long)])(self.instance, out))
        return {"table_first_children": int(out[0]), "behind_memory_first_child": int(out[1]), "behind_fused_cherry": int(out[2]),
                "max_classes": int(out[3])}

    def walkHealth(self):
        """The one-launch walk since instance creation (include/beagle_mi355.h beagleMi355WalkHealth)."""
        out = (C.c_long * 4)()
        self._check("walkHealth", self._ext("beagleMi355WalkHealth", [C.c_int, C.POINTER(C.c_long)])(self.instance, out))
        return {"self_served": int(out[0]), "spin_limit_us": int(out[1]), "folded_vectors": int(out[2]), "fold_builds": int(out[3])}

    def walkLaunchInfo(self):
        """How the one-launch walks were run (include/beagle_mi355.h beagleMi355WalkLaunchInfo)."""
        out = (C.c_long * 8)()
        self._check("walkLaunchInfo", self._ext("beagleMi355WalkLaunchInfo", [C.c_int, C.POINTER(C.c_long)])(self.instance, out))
        return {"ticket_walks": int(out[0]), "flag_walks": int(out[1]), "rows": int(out[2]), "slices": int(out[3]),
                "fused_cherries": int(out[4]), "micro_ops": int(out[5]), "slice_accumulations": int(out[6]), "partition_roots_in_walk": int(out[7])}

    def gradientStats(self):
        """How the pre-order lists of this instance were run (include/beagle_mi355.h beagleMi355GradientStats)."""
        out = (C.c_long * 4)()
        self._check("gradientStats", self._ext("beagleMi355GradientStats", [C.c_int, C.POINTER(C.c_long)])(self.instance, out))
        return {"fused": int(out[0]), "by_operation": int(out[1]), "walked": int(out[2]), "late": int(out[3])}

    def deviceBytes(self):
        return self._ext("beagleMi355DeviceBytes", [C.c_int], C.c_long)(self.instance)
