"""What each JNI native of beast-mcmc_amd/csrc/jni_shim.cpp hands the C ABI, and what it hands back — on the CPU, no engine.

BEAST calls the 47 Java_beagle_BeagleJNIWrapper_* natives, never the C ABI, and the shim is not a pass-through: per native it
decides how many entries of each Java array to copy, which arrays may be null, which are outputs, when an output is written
back.  Here jni_shim.cpp is compiled with tests/native/abi_recorder.cpp (every beagle* function as a recorder) into a temporary
shared object and each native is called through tests/jni_env.py — argument types from the class file's descriptors
(tests/golden/jni_natives.json), Java arrays LONGER than the call needs with sentinel tails, as BEAST's are
(BeagleDataLikelihoodDelegate.java:179-183: operations[] sized internalNodeCount * 7 whatever the count, the whole
branchLengths[nodeCount]).

CONTRACT below is the table of what each call may touch.  It is written from the BEAGLE API as include/beagle_mi355.h documents
it and from what the reference's Java callers pass, not read off the shim:
  * 7 ints per operation, 9 per partitioned operation (beagle.Beagle.OPERATION_TUPLE_SIZE; MultiPartitionDataLikelihoodDelegate
    .java:972-997), `count` entries of every index / edge-length array of a call that takes a count;
  * partials double[C][P][S], matrices double[C][S][S], eigen S*S, S*S, S, frequencies S, category rates / weights C, tip
    states and pattern weights and partitions P (header "Layouts at the boundary");
  * calculateRootLogLikelihoodsByPartition: partitionCount * count buffer / weights / frequencies / scale indices and results
    per partition, partitionCount partition indices, count sums (MultiPartitionDataLikelihoodDelegate.java:1074-1083 passes
    arrays of partitionCount with count = 1);
  * calculateEdgeDifferentials: count * P per-pattern derivatives, count sums, ONE category-weights index
    (AbstractBeagleBranchGradientDelegate.java:83-90 passes new int[]{0}); calculateCrossProductDifferentials: one rates and one
    weights index, S*S sums that the call ADDS to (SubstitutionModelCrossProductDelegate.java:155-162 zero-fills `first`).
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import jni_env

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.path.join(ROOT, "beast-mcmc_amd", "csrc", "jni_shim.cpp")
SHIM_UNDER_TEST = os.environ.get("BEAGLE_MI355_JNI_SHIM_SOURCE", SHIM)      # development: a deliberately broken copy of the shim

# the instance the recorder's beagleMi355GetDimensions describes:
# {tipCount, partialsBufferCount, stateCount, patternCount, categoryCount, matrixBufferCount, scaleBufferCount, partitionCount}
S, P, C_ = 5, 11, 3
DIMS = [6, 20, S, P, C_, 30, 9, 4]
COUNT, PARTITIONS = 2, 3
TAIL = 3                                 # entries every Java array is longer than the call needs
IN_SENTINEL, OUT_SENTINEL = -9999, -4242


def IN(n): return ("in", n, False)           # noqa: E704  count-derived input: exactly n entries are read
def IN0(n): return ("in", n, True)           # noqa: E704  ... that may be null
def ALL(n): return ("all", n, False)         # noqa: E704  input whose length the instance defines: read from 0, at least n
def OUT(n): return ("out", n, False)         # noqa: E704  output: nothing read, exactly n entries written on success / -8
def OUT0(n): return ("out", n, True)         # noqa: E704
def ADD0(n): return ("add", n, True)         # noqa: E704  in/out: n entries reach the ABI, n come back


OBJECT = ("object", "0", True)
# native -> (C function, parameters in the order of the descriptor: a scalar's name, or an array's role and contract length)
CONTRACT = {
    "createInstance": ("beagleCreateInstance", ["tipCount", "partialsBufferCount", "compactBufferCount", "stateCount", "patternCount",
                                                "eigenBufferCount", "matrixBufferCount", "categoryCount", "scaleBufferCount",
                                                IN0("resourceCount"), "resourceCount", "preferenceFlags", "requirementFlags", OBJECT]),
    "finalize": ("beagleFinalizeInstance", ["instance"]),
    "setCPUThreadCount": ("beagleSetCPUThreadCount", ["instance", "threadCount"]),
    "setPatternWeights": ("beagleSetPatternWeights", ["instance", ALL("P")]),
    "setPatternPartitions": ("beagleSetPatternPartitions", ["instance", "partitionCount", ALL("P")]),
    "setTipStates": ("beagleSetTipStates", ["instance", "tipIndex", ALL("P")]),
    "getTipStates": ("beagleGetTipStates", ["instance", "tipIndex", OUT("P")]),
    "setTipPartials": ("beagleSetTipPartials", ["instance", "tipIndex", ALL("P*S")]),
    "setRootPrePartials": ("beagleSetRootPrePartials", ["instance", IN("count"), IN("count"), "count"]),
    "setPartials": ("beagleSetPartials", ["instance", "bufferIndex", ALL("C*P*S")]),
    "getPartials": ("beagleGetPartials", ["instance", "bufferIndex", "scaleIndex", OUT("C*P*S")]),
    "getLogScaleFactors": ("beagleGetLogScaleFactors", ["instance", "scaleIndex", OUT("P")]),
    "setEigenDecomposition": ("beagleSetEigenDecomposition", ["instance", "eigenIndex", ALL("S*S"), ALL("S*S"), ALL("S")]),
    "setStateFrequencies": ("beagleSetStateFrequencies", ["instance", "stateFrequenciesIndex", ALL("S")]),
    "setCategoryWeights": ("beagleSetCategoryWeights", ["instance", "categoryWeightsIndex", ALL("C")]),
    "setCategoryRates": ("beagleSetCategoryRates", ["instance", ALL("C")]),
    "setCategoryRatesWithIndex": ("beagleSetCategoryRatesWithIndex", ["instance", "categoryRatesIndex", ALL("C")]),
    "setTransitionMatrix": ("beagleSetTransitionMatrix", ["instance", "matrixIndex", ALL("C*S*S"), "paddedValue"]),
    "setDifferentialMatrix": ("beagleSetDifferentialMatrix", ["instance", "matrixIndex", ALL("C*S*S")]),
    "getTransitionMatrix": ("beagleGetTransitionMatrix", ["instance", "matrixIndex", OUT("C*S*S")]),
    "convolveTransitionMatrices": ("beagleConvolveTransitionMatrices", ["instance", IN("count"), IN("count"), IN("count"), "count"]),
    "addTransitionMatrices": ("beagleAddTransitionMatrices", ["instance", IN("count"), IN("count"), IN("count"), "count"]),
    "transposeTransitionMatrices": ("beagleTransposeTransitionMatrices", ["instance", IN("count"), IN("count"), "count"]),
    "updateTransitionMatrices": ("beagleUpdateTransitionMatrices", ["instance", "eigenIndex", IN("count"), IN0("count"), IN0("count"),
                                                                    IN("count"), "count"]),
    "updateTransitionMatricesWithMultipleModels": ("beagleUpdateTransitionMatricesWithMultipleModels",
                                                   ["instance", IN("count"), IN("count"), IN("count"), IN0("count"), IN0("count"),
                                                    IN("count"), "count"]),
    "updatePrePartials": ("beagleUpdatePrePartials", ["instance", IN("7*count"), "count", "cumulativeScaleIndex"]),
    "updatePrePartialsByPartition": ("beagleUpdatePrePartialsByPartition", ["instance", IN("9*count"), "count"]),
    "updatePartials": ("beagleUpdatePartials", ["instance", IN("7*count"), "count", "cumulativeScaleIndex"]),
    "updatePartialsByPartition": ("beagleUpdatePartialsByPartition", ["instance", IN("9*count"), "count"]),
    "waitForPartials": ("beagleWaitForPartials", ["instance", IN("count"), "count"]),
    "accumulateScaleFactors": ("beagleAccumulateScaleFactors", ["instance", IN("count"), "count", "cumulativeScaleIndex"]),
    "accumulateScaleFactorsByPartition": ("beagleAccumulateScaleFactorsByPartition",
                                          ["instance", IN("count"), "count", "cumulativeScaleIndex", "partitionIndex"]),
    "removeScaleFactors": ("beagleRemoveScaleFactors", ["instance", IN("count"), "count", "cumulativeScaleIndex"]),
    "removeScaleFactorsByPartition": ("beagleRemoveScaleFactorsByPartition",
                                      ["instance", IN("count"), "count", "cumulativeScaleIndex", "partitionIndex"]),
    "resetScaleFactors": ("beagleResetScaleFactors", ["instance", "cumulativeScaleIndex"]),
    "resetScaleFactorsByPartition": ("beagleResetScaleFactorsByPartition", ["instance", "cumulativeScaleIndex", "partitionIndex"]),
    "copyScaleFactors": ("beagleCopyScaleFactors", ["instance", "destScalingIndex", "srcScalingIndex"]),
    "calculateRootLogLikelihoods": ("beagleCalculateRootLogLikelihoods", ["instance", IN("count"), IN("count"), IN("count"), IN("count"),
                                                                          "count", OUT("count")]),
    "calculateRootLogLikelihoodsByPartition": ("beagleCalculateRootLogLikelihoodsByPartition",
                                               ["instance", IN("partitionCount*count"), IN("partitionCount*count"),
                                                IN("partitionCount*count"), IN("partitionCount*count"), IN("partitionCount"),
                                                "partitionCount", "count", OUT("partitionCount*count"), OUT("count")]),
    "getSiteLogLikelihoods": ("beagleGetSiteLogLikelihoods", ["instance", OUT("P")]),
    "calculateEdgeDifferentials": ("beagleCalculateEdgeDifferentials", ["instance", IN("count"), IN("count"), IN("count"), ALL("1"),
                                                                        "count", OUT0("count*P"), OUT0("count"), OUT0("count")]),
    "calculateCrossProductDifferentials": ("beagleCalculateCrossProductDifferentials",
                                           ["instance", IN("count"), IN("count"), ALL("1"), ALL("1"), IN("count"), "count",
                                            ADD0("S*S"), ADD0("S*S")]),
}
PINNED = {"getPartials": "beagleMi355GetPartialsPinned", "getSiteLogLikelihoods": "beagleMi355GetSiteLogLikelihoodsPinned"}
# natives that take this tier's route without a table row: two strings, the refusal
OTHERS = ["getVersion", "getCitation", "calculateEdgeDerivative"]
MARSHALLED = sorted(CONTRACT)


@pytest.fixture(scope="module")
def recorder(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("jni_recorder") / "libshim_recorder.so")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-fPIC", "-shared", "-Wall", "-I", os.path.dirname(SHIM), SHIM_UNDER_TEST,
                           os.path.join(ROOT, "tests", "native", "abi_recorder.cpp"), "-o", so])
    lib = C.CDLL(so, mode=C.RTLD_LOCAL)
    lib.rec_name.restype = C.c_char_p
    lib.rec_scalar.restype = lib.rec_pointer_value.restype = lib.rec_fill.restype = C.c_double
    lib.rec_fill.argtypes = [C.c_int, C.c_long]
    lib.rec_pointer_overrun.restype = C.c_long
    lib.rec_set_dims((C.c_int * 8)(*DIMS))
    return lib


def records(lib):
    out = []
    for i in range(lib.rec_count()):
        ptrs = [(bool(lib.rec_pointer_null(i, k)), [lib.rec_pointer_value(i, k, j) for j in range(lib.rec_pointer_seen(i, k))])
                for k in range(lib.rec_pointer_count(i))]
        for k in range(lib.rec_pointer_count(i)):              # (the recorder stops at the end of the wrapper's buffer and says so)
            assert lib.rec_pointer_overrun(i, k) == 0, "%s: pointer %d is %d entries shorter than what the library touches" % (
                lib.rec_name(i).decode(), k, lib.rec_pointer_overrun(i, k))
        out.append((lib.rec_name(i).decode(), [lib.rec_scalar(i, k) for k in range(lib.rec_scalar_count(i))], ptrs))
    return out


class Case:
    """One call of one native: distinct scalars, arrays with sentinel tails, the recorder told what the contract lets it touch."""

    def __init__(self, name, count=COUNT, nulls=(), shorten=None, pad=TAIL):
        self.name = name
        self.abi, spec = CONTRACT[name]
        kinds, _ = jni_env.parse_descriptor(jni_env.natives()[name])
        assert len(kinds) == len(spec), name
        self.scalars, self.arrays, self.args = [], [], []          # arrays: (role, n, array or None, what it held before the call)
        names = {"S": S, "P": P, "C": C_, "count": count, "partitionCount": PARTITIONS, "resourceCount": count}
        for pos, (kind, what) in enumerate(zip(kinds, spec)):
            if isinstance(what, str):
                assert kind in "IJD", (name, pos)
                v = names.get(what)
                if v is None:
                    v = {"I": 101 + 7 * pos, "J": (1 << 40) + 13 * pos, "D": 0.625 + pos}[kind]      # a long that an int cannot hold
                self.scalars.append(float(v))
                self.args.append(v)
                continue
            role, n, nullable = what
            if role == "object":
                self.args.append(None)
                continue
            n = int(eval(n, {}, names))
            index = len(self.arrays)
            if index in nulls:
                assert nullable, (name, pos)
                self.arrays.append((role, 0, None, None))
                self.args.append(None)
                continue
            size = max(0, n + pad - (pad + 1 if shorten == index else 0))
            dtype = np.int32 if kind == "[I" else np.float64
            if role == "out":
                a = np.full(size, OUT_SENTINEL, dtype=dtype)
            else:
                a = np.full(size, IN_SENTINEL, dtype=dtype)
                a[:n] = (1000 * (pos + 1) + np.arange(n) + (0.25 if kind == "[D" else 0))[:size]
            self.arrays.append((role, n, a, a.copy()))
            self.args.append(a)

    def run(self, lib, env, rc=0):
        lib.rec_reset()
        lib.rec_set_rc(rc)
        lens = [n for _, n, _, _ in self.arrays]
        lib.rec_expect((C.c_long * max(1, len(lens)))(*lens), len(lens))
        got = env.call(lib, self.name, *self.args)
        self.log = list(env.log)
        return got

    def moved(self, env, index):
        env.log = self.log
        return [m for m in env.moved(self.arrays[index][2]) if m[2] > 0]


def check_inputs(case, env, rec):
    """The one record: the C function, the scalars in ABI order, every pointer null or holding the first n entries — and the region
    log: exactly n read of a count-derived input, one read from 0 of an instance-sized one, nothing read of an output."""
    name, scalars, ptrs = rec
    assert name == case.abi
    assert scalars == case.scalars, (case.name, scalars, case.scalars)
    assert len(ptrs) == len(case.arrays), case.name
    for k, ((role, n, a, before), (is_null, seen)) in enumerate(zip(case.arrays, ptrs)):
        assert is_null == (a is None), (case.name, k)
        if a is None:
            assert seen == []
            continue
        gets = [m for m in case.moved(env, k) if m[0] == "get"]
        if role == "out":
            assert gets == [], (case.name, k, gets)
            continue
        assert seen == [float(x) for x in before[:n]], (case.name, k)
        if role == "in":
            assert gets == ([("get", 0, n)] if n else []), (case.name, k, gets)
        else:
            assert len(gets) == 1 and gets[0][1] == 0 and n <= gets[0][2] <= a.size, (case.name, k, gets)


def check_outputs(case, env, lib, committed):
    for k, (role, n, a, before) in enumerate(case.arrays):
        if a is None:
            continue
        sets = [m for m in case.moved(env, k) if m[0] == "set"]
        if role in ("in", "all") or not committed:
            assert sets == [], (case.name, k, sets)
            assert np.array_equal(a, before), (case.name, k)
            continue
        fill = np.array([lib.rec_fill(k, j) for j in range(n)]) + (0.5 if a.dtype == np.float64 else 0)
        if role == "out":
            assert sets == ([("set", 0, n)] if n else []), (case.name, k, sets)
            assert np.array_equal(a[:n], fill.astype(a.dtype)), (case.name, k)
        else:                                                        # in/out: what the array held, plus what the call added
            assert len(sets) == 1 and sets[0][1] == 0 and n <= sets[0][2] <= a.size, (case.name, k, sets)
            assert np.array_equal(a[:n], before[:n] + fill), (case.name, k)
        assert np.array_equal(a[n:], before[n:]), (case.name, k, "the tail")


def nullable_sets(name):
    """() and, for a native with nullable arrays, each of them null alone and all of them null."""
    idx, k = [], 0
    for what in CONTRACT[name][1]:
        if isinstance(what, tuple) and what[0] != "object":
            if what[2]:
                idx.append(k)
            k += 1
    return [()] + [(i,) for i in idx] + ([tuple(idx)] if len(idx) > 1 else [])


# ---- signatures --------------------------------------------------------------------------------------------------------------
def shim_descriptors(path):
    """The JNI_FN(ret, name)(JNIEnv*, jobject, ...) definitions of the shim as method descriptors; object types (which C cannot
    tell apart) take the class the fixture names at that position."""
    text = re.sub(r"//[^\n]*", "", open(path).read())
    fixture = jni_env.natives()
    code = {"jint": "I", "jlong": "J", "jdouble": "D", "jintArray": "[I", "jdoubleArray": "[D"}
    out = {}
    for ret, name, params in re.findall(r"JNI_FN\((\w+),\s*(\w+)\)\s*\(([^)]*)\)", text):
        types = [re.match(r"\s*([\w*]+)", p).group(1) for p in params.split(",")]
        assert types[:2] == ["JNIEnv*", "jobject"], name
        want_params, want_ret = jni_env.parse_descriptor(fixture[name]) if name in fixture else ([], "")
        desc = ""
        for k, t in enumerate(types[2:]):
            if t in code:
                desc += code[t]
            else:
                assert t in ("jobject", "jstring", "jobjectArray"), (name, t)
                w = want_params[k] if k < len(want_params) else "?"
                desc += w if (w.startswith("[L") if t == "jobjectArray" else w.startswith("L")) else "<%s>" % t
        if ret in code:
            r = code[ret]
        else:
            r = want_ret if (want_ret.startswith("[L") if ret == "jobjectArray" else want_ret.startswith("L")) else "<%s>" % ret
        assert name not in out, name
        out[name] = "(%s)%s" % (desc, r)
    return out


def test_shim_signatures_are_the_class_files_descriptors():
    fixture = jni_env.natives()
    assert len(fixture) == 47
    got = shim_descriptors(SHIM_UNDER_TEST)
    assert sorted(got) == sorted(fixture)
    wrong = {n: (got[n], fixture[n]) for n in fixture if got[n] != fixture[n]}
    assert not wrong, wrong


def test_the_table_covers_every_native_callable_without_java_objects():
    assert sorted(MARSHALLED + OTHERS + ["getResourceList", "getBenchmarkedResourceList"]) == sorted(jni_env.natives())
    assert len(MARSHALLED) + len(OTHERS) == 45


# ---- cases -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MARSHALLED)
def test_arguments_reach_the_abi_and_results_return(recorder, name):
    """rc 0: scalars in ABI order, inputs intact and exactly as long as the contract says, null arrays as NULL, outputs back with
    exactly the defined entries and the tail kept."""
    for pinned in ((1, 0) if name in PINNED else (1,)):
        recorder.rec_set_pinned(pinned)
        for nulls in nullable_sets(name):
            env = jni_env.JniEnv()
            case = Case(name, nulls=nulls)
            assert case.run(recorder, env) == 0
            recs = records(recorder)
            assert len(recs) == 1, [r[0] for r in recs]
            if name in PINNED and pinned:                          # the pinned route: no output pointer, the same entries come back
                assert recs[0][0] == PINNED[name] and recs[0][1] == case.scalars
            else:
                check_inputs(case, env, recs[0])
            check_outputs(case, env, recorder, committed=True)
            env.assert_clean()
    recorder.rec_set_pinned(1)


@pytest.mark.parametrize("name", [n for n in MARSHALLED if any(isinstance(w, tuple) and w[0] in ("out", "add") for w in CONTRACT[n][1])])
def test_outputs_are_written_on_success_and_floating_point_error_only(recorder, name):
    """-8 (FLOATING_POINT: the value IS the result, BeagleJNIImpl tolerates it) writes the outputs as success does; any other
    code leaves every Java array as it was.  The code itself always comes back."""
    for pinned in ((1, 0) if name in PINNED else (1,)):
        recorder.rec_set_pinned(pinned)
        for rc in (-8, -1, -5, -7):
            if rc == -7 and name in PINNED and pinned:           # (from a ...Pinned call -7 means "take the other route")
                continue
            env = jni_env.JniEnv()
            case = Case(name)
            assert case.run(recorder, env, rc=rc) == rc
            assert len(records(recorder)) == 1
            check_outputs(case, env, recorder, committed=(rc == -8))
            env.assert_clean()
    recorder.rec_set_pinned(1)


def _arrays_with_a_length(name):
    return [k for k, (role, n, a, _) in enumerate(Case(name).arrays) if n > 0]


@pytest.mark.parametrize("name,index", [(n, k) for n in MARSHALLED for k in _arrays_with_a_length(n)])
def test_an_array_one_entry_short_is_refused(recorder, name, index):
    """-5 (OUT_OF_RANGE) from the wrapper itself: the library is not called (it would run past the copy), no array changes."""
    for pinned in ((1, 0) if name in PINNED else (1,)):
        recorder.rec_set_pinned(pinned)
        env = jni_env.JniEnv()
        case = Case(name, shorten=index)
        assert case.arrays[index][2].size == case.arrays[index][1] - 1
        assert case.run(recorder, env) == -5, name
        assert [r[0] for r in records(recorder) if r[0] not in PINNED.values()] == [], name
        for k, (role, n, a, before) in enumerate(case.arrays):
            assert np.array_equal(a, before), (name, k)
            assert [m for m in case.moved(env, k) if m[0] == "set"] == []
        env.assert_clean()
    recorder.rec_set_pinned(1)


@pytest.mark.parametrize("name", [n for n in MARSHALLED if "count" in CONTRACT[n][1]])
def test_count_zero_reaches_the_abi_and_moves_nothing(recorder, name):
    env = jni_env.JniEnv()
    case = Case(name, count=0)
    assert case.run(recorder, env) == 0
    recs = records(recorder)
    assert len(recs) == 1
    check_inputs(case, env, recs[0])
    check_outputs(case, env, recorder, committed=True)
    for k, (role, n, a, before) in enumerate(case.arrays):
        if n == 0:
            assert case.moved(env, k) == [] and np.array_equal(a, before), (name, k)
    env.assert_clean()


def test_cross_product_sums_go_in_and_come_back(recorder):
    """The sums are ADDED to (SubstitutionModelCrossProductDelegate zero-fills them; a caller that pre-fills them gets its values
    plus the call's): what the arrays held reaches the ABI, the sum returns."""
    env = jni_env.JniEnv()
    case = Case("calculateCrossProductDifferentials")
    assert case.run(recorder, env) == 0
    (_, _, ptrs), = records(recorder)
    for k in (5, 6):
        role, n, a, before = case.arrays[k]
        assert role == "add" and n == S * S
        assert ptrs[k][1] == [float(x) for x in before[:n]] and before[0] != 0
        assert np.array_equal(a[:n], before[:n] + np.array([recorder.rec_fill(k, j) + 0.5 for j in range(n)]))
    env.assert_clean()


def test_strings_and_the_refusal(recorder):
    env = jni_env.JniEnv()
    recorder.rec_reset()
    assert env.call(recorder, "getVersion") == "9.8.7-recorder"
    assert env.call(recorder, "getCitation") == "recorder citation\nsecond line"
    assert [r[0] for r in records(recorder)] == ["beagleGetVersion", "beagleGetCitation"]
    # calculateEdgeDerivative (I[I[II[I[IIII[II[D[D)I: no caller in the reference; refused, no array looked at
    recorder.rec_reset()
    ints = [np.full(4, 7, dtype=np.int32) for _ in range(5)]
    dbls = [np.full(4, 7.5) for _ in range(2)]
    rc = env.call(recorder, "calculateEdgeDerivative", 1, ints[0], ints[1], 2, ints[2], ints[3], 3, 4, 5, ints[4], 6, dbls[0], dbls[1])
    assert rc == -7
    assert records(recorder) == [] and env.log == []
    assert all(np.all(a == 7) for a in ints) and all(np.all(a == 7.5) for a in dbls)
    env.assert_clean()


def test_a_call_outside_the_environment_is_recorded_not_fatal():
    """The trap record the other tests assert to be empty does fill: slot 6 (FindClass) called by hand."""
    env = jni_env.JniEnv()
    table = C.cast(C.cast(env.env, C.POINTER(C.c_void_p))[0], C.POINTER(C.c_void_p))
    assert C.CFUNCTYPE(C.c_void_p, C.c_void_p, C.c_char_p)(table[6])(env.env, b"beagle/ResourceDetails") is None
    assert env.traps == [6]
    with pytest.raises(AssertionError):
        env.assert_clean()
