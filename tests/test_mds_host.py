"""CPU tier of multidimensional scaling: the symbols of libmds2_jni.so against its header and the fixture of native names, the
refusal without a GPU, the host restatement (tests/mds_reference.py) against itself — incremental path against full evaluation,
gradient against central differences, restore, long double — and the marshalling of the 14 natives through a Python JNIEnv
(tests/jni_env_mds.py) against a recording stand-in for the C ABI (tests/native/mds_abi_recorder.cpp)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import jni_env_mds
import mds_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_DIR = os.path.join(ROOT, "beast-mcmc_amd", "lib")
MDS_LIB = os.path.join(LIB_DIR, "libmds2_jni.so")
HEADER = os.path.join(ROOT, "include", "mds_mi355.h")


@pytest.fixture(scope="module")
def mds_library():
    if not os.path.exists(MDS_LIB):
        __import__("importlib").import_module("beast-mcmc_amd.build").build_mds()
    return MDS_LIB


def exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
    return sorted(line.split()[-1] for line in out.splitlines() if line.strip())


def header_functions():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\bint\s+(mds[A-Za-z0-9]+)\s*\(", text)))


# -- the library's surface -------------------------------------------------------------------------------------------------------

def test_the_library_exports_the_header_and_the_fourteen_natives_and_nothing_else(mds_library):
    natives = jni_env_mds.natives()
    assert len(natives) == 14
    declared = header_functions()
    for name in ("Initialize", "UpdateLocations", "GetSumOfIncrements", "StoreState", "RestoreState", "AcceptState", "MakeDirty",
                 "SetPairwiseData", "GetPairwiseData", "SetParameters", "GetLocationGradient", "GetInternalDimension", "Finalize",
                 "Stats"):
        assert "mds" + name in declared
    assert exported(mds_library) == sorted(declared + [jni_env_mds.prefix() + n for n in natives])


def test_the_python_binding_types_every_function_of_the_header():
    from beast_mcmc_amd import mds
    assert sorted(mds.ABI) == header_functions()


def test_the_library_does_not_need_the_engine_library(mds_library):
    dyn = subprocess.run(["readelf", "-d", mds_library], check=True, capture_output=True, text=True).stdout
    assert "hmsbeagle" not in dyn and "libamdhip64" in dyn


def test_the_engine_library_exports_what_it_did(mds_library):
    """Nothing of MDS went into libhmsbeagle-jni.so: its exports are still the beagle* functions of its header and its natives."""
    names = exported(os.path.join(LIB_DIR, "libhmsbeagle-jni.so"))
    assert names and not [n for n in names if "mds" in n.lower()]
    assert all(n.startswith(("beagle", "Java_beagle_BeagleJNIWrapper_", "JNI_On")) for n in names), names


def test_without_a_gpu_initialize_answers_no_resource(mds_library):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from beast_mcmc_amd import mds
    native = mds.NativeMDS()
    assert native.raw.mdsInitialize(2, 10, 0, -1, 0) == -6
    assert native.raw.mdsInitialize(2, 10, mds.LEFT_TRUNCATION, 0, 4) == -6
    with pytest.raises(mds.MDSError) as e:
        mds.MultiDimensionalScalingLikelihood(2, np.zeros((3, 3)), np.zeros((3, 2)), 1.0)
    assert e.value.code == -6
    assert native.raw.mdsStoreState(0) == -4 and native.raw.mdsInitializeLayout(2, 3, 4, 0, -1, 0) == -7


# -- the restatement against itself ----------------------------------------------------------------------------------------------

def core(n, d, truncated, seed, missing=0.05, dtype=np.float64):
    x, y = ref.synthetic(n, d, seed, missing=missing)
    c = ref.Core(d, n, ref.LEFT_TRUNCATION if truncated else 0, dtype=dtype)
    c.set_parameters([1.7])
    c.set_pairwise_data(y)
    c.update_location(-1, x)
    c.make_dirty()
    return c, x, y


@pytest.mark.parametrize("truncated", [False, True])
def test_by_hand_three_locations(truncated):
    """(0,0), (3,4), (0,1): distances 5, 1, sqrt(18); one pair missing."""
    from scipy.special import log_ndtr
    x = np.array([[0.0, 0.0], [3.0, 4.0], [0.0, 1.0]])
    y = np.array([[0.0, 4.5, np.nan], [4.5, 0.0, 4.0], [np.nan, 4.0, 0.0]])
    tau = 0.8
    c = ref.Core(2, 3, ref.LEFT_TRUNCATION if truncated else 0)
    c.set_parameters([tau])
    c.set_pairwise_data(y)
    c.update_location(-1, x)
    want = 0.5 * tau * ((5 - 4.5) ** 2 + (np.sqrt(18.0) - 4.0) ** 2)
    if truncated:
        want += log_ndtr(5 * np.sqrt(tau)) + log_ndtr(np.sqrt(18.0 * tau))
    assert abs(c.sum_of_increments() - want) <= 4e-16 * abs(want) and c.observation_count() == 2
    assert abs(c.log_likelihood() - (0.5 * (np.log(tau) - np.log(2 * np.pi)) * 2 - want)) <= 1e-15 * abs(want)


@pytest.mark.parametrize("truncated", [False, True])
@pytest.mark.parametrize("d", [1, 2, 3, 6])
def test_incremental_path_is_the_full_evaluation(d, truncated):
    n = 40
    c, x, y = core(n, d, truncated, seed=d)
    rng = np.random.default_rng(100 + d)
    c.sum_of_increments()
    for step in range(60):
        c.store_state()
        before = c.sum_of_increments()
        k = int(rng.integers(n))
        x_new = x.copy()
        x_new[k] += rng.normal(0.0, 0.5, size=d)
        c.update_location(k, x_new[k])
        got = c.sum_of_increments()
        assert c.paths[-1] == "row"
        fresh = ref.Core(d, n, ref.LEFT_TRUNCATION if truncated else 0)
        fresh.set_parameters([1.7])
        fresh.set_pairwise_data(y)
        fresh.update_location(-1, x_new)
        assert abs(got - fresh.sum_of_increments()) <= 1e-12 * fresh.absolute_sum()
        if rng.random() < 0.5:
            c.restore_state()
            after = c.sum_of_increments()
            assert after.tobytes() == before.tobytes()                     # restore: the stored value's bits
        else:
            c.accept_state()
            x = x_new
    # a second single update before the next store, an all-location update, makeDirty: full evaluations
    c.store_state()
    c.update_location(1, x[1] + 0.1)
    c.update_location(2, x[2] - 0.1)
    c.sum_of_increments()
    assert c.paths[-1] == "all"
    c.update_location(-1, x)
    c.sum_of_increments()
    assert c.paths[-1] == "all"
    count = len(c.paths)
    c.set_parameters([2.0])
    c.sum_of_increments()
    assert (len(c.paths) == count + 1 and c.paths[-1] == "all") if truncated else len(c.paths) == count
    c.make_dirty()
    c.sum_of_increments()
    assert c.paths[-1] == "all"


@pytest.mark.parametrize("truncated", [False, True])
@pytest.mark.parametrize("d", [1, 2, 3, 6])
def test_gradient_is_the_derivative_of_the_log_likelihood(d, truncated):
    """Central differences with step 1e-5: truncation error O(h^2 f''') ~ 1e-10 and rounding ~ eps |log L| / h ~ 1e-8 of the
    largest entry, both far below the bound of 1e-6 of the largest entry."""
    n, h = 40, 1e-5
    c, x, y = core(n, d, truncated, seed=10 + d)
    g, _ = c.gradient()
    numeric = np.zeros_like(g)
    for i in range(n):
        for k in range(d):
            value = []
            for sign in (1.0, -1.0):
                moved = x.copy()
                moved[i, k] += sign * h
                c.update_location(-1, moved)
                value.append(c.log_likelihood())
            numeric[i, k] = (value[0] - value[1]) / (2.0 * h)
    worst = np.abs(g - numeric).max() / np.abs(g).max()
    print("D = %d truncated = %s: worst difference %.2e of the largest entry" % (d, truncated, worst))
    assert worst <= 1e-6


@pytest.mark.parametrize("truncated", [False, True])
@pytest.mark.parametrize("n,d", [(64, 2), (257, 3), (400, 6)])
def test_fp64_restatement_against_long_double(n, d, truncated):
    """Both runs from the same fp64 inputs; S within 1e-10 of sum |increment| and every gradient entry within 1e-10 of its row's
    sum of absolute terms: the bounds the device is held to, which the restatement itself must meet with room to spare."""
    if np.finfo(np.longdouble).eps >= np.finfo(np.float64).eps:
        pytest.skip("numpy.longdouble is no wider than float64 on this platform")
    c64, _, _ = core(n, d, truncated, seed=n)
    cld, _, _ = core(n, d, truncated, seed=n, dtype=np.longdouble)
    s64, sld, scale = c64.sum_of_increments(), cld.sum_of_increments(), cld.absolute_sum()
    print("N = %d: |S - S_ld| = %.2e of sum |increment|" % (n, abs(s64 - sld) / scale))
    assert abs(s64 - sld) <= 1e-10 * scale
    assert abs(c64.log_likelihood() - cld.log_likelihood()) <= 1e-10 * abs(cld.log_likelihood())
    g64, _ = c64.gradient()
    gld, rows = cld.gradient()
    assert np.all(np.abs(g64 - gld) <= 1e-10 * rows)


def test_missing_pairs_and_coincident_locations():
    c, x, y = core(30, 2, True, seed=5, missing=1.0)
    assert c.observation_count() == 0 and c.sum_of_increments() == 0.0
    g, _ = c.gradient()
    assert not g.any()
    c, x, y = core(30, 2, True, seed=6, missing=0.0)
    x[7] = x[3]
    c.update_location(-1, x)
    g, _ = c.gradient()
    assert np.all(np.isfinite(g)) and np.isfinite(c.sum_of_increments())


# -- the natives' marshalling ----------------------------------------------------------------------------------------------------

N, D = 5, 3                                      # the recorder's instance
TAIL, SENTINEL = 4, -4242.0


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("mds_jni") / "libmds_jni_recorded.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-Wall",
                           os.path.join(ROOT, "beast-mcmc_amd", "jni_mds", "jni_mds.cpp"),
                           os.path.join(ROOT, "tests", "native", "mds_abi_recorder.cpp"), "-o", out])
    lib = C.CDLL(out)
    lib.mdsRecorderName.restype = C.c_char_p
    lib.mdsRecorderScalar.restype = C.c_longlong
    lib.mdsRecorderLength.restype = C.c_longlong
    return lib


def recorded(lib, only=None):
    """[(name, scalars, length, data)] of the calls that reached the C ABI, the size queries left out unless asked for."""
    calls = []
    for i in range(lib.mdsRecorderCalls()):
        name = lib.mdsRecorderName(i).decode()
        scalars = [lib.mdsRecorderScalar(i, k) for k in range(lib.mdsRecorderScalarCount(i))]
        length = lib.mdsRecorderLength(i)
        data = np.zeros(max(length, 0))
        if length > 0 and name.startswith(("mdsUpdate", "mdsSet")):
            lib.mdsRecorderData(i, data.ctypes.data_as(C.POINTER(C.c_double)))
        calls.append((name, scalars, length, data))
    if only is None:
        calls = [c for c in calls if c[0] not in ("mdsGetLocationCount", "mdsGetInternalDimension")]
    return calls


def java_array(n, rng):
    a = rng.normal(size=n + TAIL)
    a[n:] = SENTINEL
    return a


@pytest.fixture
def env(shim):
    shim.mdsRecorderReset()
    return jni_env_mds.MdsJniEnv()


def test_scalar_natives_pass_their_arguments(shim, env):
    assert env.call(shim, "initialize__IIJII", 3, 50, (1 << 40) + 33, 2, 8) == 7
    assert [c[:2] for c in recorded(shim)] == [("mdsInitialize", [3, 50, (1 << 40) + 33, 2, 8])]
    for name, function in (("storeState", "mdsStoreState"), ("restoreState", "mdsRestoreState"), ("acceptState", "mdsAcceptState"),
                           ("makeDirty", "mdsMakeDirty")):
        shim.mdsRecorderReset()
        assert env.call(shim, name, 4) is None
        assert [c[:2] for c in recorded(shim)] == [(function, [4])] and env.thrown == []
    shim.mdsRecorderReset()
    assert env.call(shim, "getSumOfIncrements", 4) == 42.5
    assert env.call(shim, "getInternalDimension", 4) == D
    env.assert_clean()


def test_the_layout_initialize_and_the_observation_gradient_are_refused(shim, env):
    assert env.call(shim, "initialize__IIIJII", 2, 10, 20, 1, -1, 0) == -7
    assert env.thrown == [("java/lang/RuntimeException", "mdsInitializeLayout: -7")]
    assert recorded(shim)[0][:2] == ("mdsInitializeLayout", [2, 10, 20, 1, -1, 0])
    out = np.full(8, SENTINEL)
    env.call(shim, "getObservationGradient", 0, out)
    assert env.thrown == [("java/lang/RuntimeException", "mdsGetObservationGradient: -7")]
    assert np.all(out == SENTINEL) and env.moved(out) == []
    env.assert_clean()


@pytest.mark.parametrize("index,need", [(-1, N * D), (0, D), (4, D)])
def test_update_locations_copies_what_the_call_uses(shim, env, index, need):
    a = java_array(need, np.random.default_rng(need))
    env.call(shim, "updateLocations", 9, index, a)
    (name, scalars, length, data), = recorded(shim)
    assert (name, scalars, length) == ("mdsUpdateLocations", [9, index], need)
    assert np.array_equal(data, a[:need]) and env.moved(a) == [("get", 0, need)] and env.thrown == []
    env.assert_clean()


def test_set_pairwise_data_and_parameters(shim, env):
    y = java_array(N * N, np.random.default_rng(1))
    env.call(shim, "setPairwiseData", 2, y)
    (name, scalars, length, data), = recorded(shim)
    assert (name, scalars, length) == ("mdsSetPairwiseData", [2], N * N) and np.array_equal(data, y[:N * N])
    assert env.moved(y) == [("get", 0, N * N)]
    shim.mdsRecorderReset()
    p = java_array(1, np.random.default_rng(2))
    env.call(shim, "setParameters", 2, p)
    (name, scalars, length, data), = recorded(shim)
    assert (name, scalars, length) == ("mdsSetParameters", [2], 1) and data[0] == p[0] and env.moved(p) == [("get", 0, 1)]
    env.assert_clean()


def test_get_pairwise_data_allocates_n_squared(shim, env):
    out = env.call(shim, "getPairwiseData", 3)
    assert out is not None and out.size == N * N and len(env.created) == 1
    assert np.array_equal(out, 1000.0 + np.arange(N * N)) and env.moved(out) == [("set", 0, N * N)]
    assert [c[:3] for c in recorded(shim)] == [("mdsGetPairwiseData", [3], N * N)]
    env.assert_clean()


def test_get_location_gradient_fills_n_times_d(shim, env):
    g = np.full(N * D + TAIL, SENTINEL)
    env.call(shim, "getLocationGradient", 3, g)
    assert np.array_equal(g[:N * D], -(np.arange(N * D) + 1.0)) and np.all(g[N * D:] == SENTINEL)
    assert env.moved(g) == [("set", 0, N * D)] and env.thrown == []
    env.assert_clean()


@pytest.mark.parametrize("name,function,args,short", [
    ("updateLocations", "mdsUpdateLocations", (1, -1), N * D - 1),
    ("updateLocations", "mdsUpdateLocations", (1, 2), D - 1),
    ("setPairwiseData", "mdsSetPairwiseData", (1,), N * N - 1),
    ("setParameters", "mdsSetParameters", (1,), 0),
    ("getLocationGradient", "mdsGetLocationGradient", (1,), N * D - 1),
])
def test_short_and_null_arrays_raise_and_leave_everything_untouched(shim, env, name, function, args, short):
    for array in (np.full(short, SENTINEL), None):
        shim.mdsRecorderReset()
        env.call(shim, name, *(args + (array,)))
        assert env.thrown == [("java/lang/RuntimeException", "%s: -5" % function)]
        assert recorded(shim) == []                                       # the C ABI was not called
        if array is not None:
            assert np.all(array == SENTINEL) and env.moved(array) == []
    env.assert_clean()


@pytest.mark.parametrize("name,function,args,failed_result", [
    ("initialize__IIJII", "mdsInitialize", (2, 10, 1, -1, 0), -6),
    ("updateLocations", "mdsUpdateLocations", (1, 0, np.zeros(D)), None),
    ("getSumOfIncrements", "mdsGetSumOfIncrements", (1,), "nan"),
    ("storeState", "mdsStoreState", (1,), None),
    ("restoreState", "mdsRestoreState", (1,), None),
    ("acceptState", "mdsAcceptState", (1,), None),
    ("makeDirty", "mdsMakeDirty", (1,), None),
    ("setPairwiseData", "mdsSetPairwiseData", (1, np.zeros(N * N)), None),
    ("setParameters", "mdsSetParameters", (1, np.ones(1)), None),
    ("getPairwiseData", "mdsGetPairwiseData", (1,), None),
    ("getLocationGradient", "mdsGetLocationGradient", (1, np.full(N * D, SENTINEL)), None),
    ("getInternalDimension", "mdsGetInternalDimension", (1,), -6),
])
def test_a_negative_code_becomes_one_exception(shim, env, name, function, args, failed_result):
    shim.mdsRecorderFail(function.encode(), -6)
    out = env.call(shim, name, *args)
    assert env.thrown == [("java/lang/RuntimeException", "%s: -6" % function)]
    if failed_result == "nan":
        assert np.isnan(out)
    else:
        assert out == failed_result
    assert env.created == []                                              # no array is made for a failed getPairwiseData
    for a in args:
        if isinstance(a, np.ndarray) and a.size == N * D and a[0] == SENTINEL:
            assert np.all(a == SENTINEL)
    env.assert_clean()


def test_an_unknown_instance_raises_before_any_array_is_read(shim, env):
    shim.mdsRecorderFail(b"mdsGetLocationCount", -4)
    a = np.zeros(N * D)
    env.call(shim, "updateLocations", 77, -1, a)
    assert env.thrown == [("java/lang/RuntimeException", "mdsUpdateLocations: -4")] and env.moved(a) == []
    assert env.call(shim, "getPairwiseData", 77) is None
    assert env.thrown == [("java/lang/RuntimeException", "mdsGetPairwiseData: -4")]
    env.assert_clean()
