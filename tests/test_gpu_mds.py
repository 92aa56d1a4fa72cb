"""GPU tier of multidimensional scaling: libmds2_jni.so on the device against the host restatement (tests/mds_reference.py).

Inputs (mds_reference.synthetic, seeded): locations N(0, 2^2), observations |true distance + N(0, 0.3^2)| symmetrised, 5 % of the
pairs NaN, tau = 1.7.  Bounds, derived and not tuned:
  * |S - S_ref| <= 1e-10 sum |increment| — the restatement's own absolute sum; with truncation the terms have both signs, so a
    bound relative to S could be empty;
  * log L to the project's parity bound, 1e-10 relative;
  * every gradient entry within 1e-10 of its row's sum of absolute terms (a row's terms cancel).
"""
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import jni_env_mds
import mds_reference as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAU = 1.7


@pytest.fixture(scope="module")
def mds():
    from beast_mcmc_amd import mds as module
    if not os.path.exists(module.MDS_LIB):
        __import__("importlib").import_module("beast-mcmc_amd.build").build_mds()
    return module


class Restated:
    """MultiDimensionalScalingLikelihood's call order (beast_mcmc_amd.mds has the same) over the restated core."""

    def __init__(self, dimension, observations, locations, precision, left_truncated=False):
        n = observations.shape[0]
        self.core = ref.Core(dimension, n, ref.LEFT_TRUNCATION if left_truncated else 0)
        self.core.set_parameters([precision])
        self.core.set_pairwise_data(observations)
        self.core.update_location(-1, locations)
        self.count = self.core.observation_count()
        self.log_likelihood = self.stored_log_likelihood = 0.0
        self.makeDirty()

    def setLocation(self, k, x):
        self.core.update_location(k, x)
        self.known = False

    def setLocations(self, x):
        self.core.update_location(-1, x)
        self.known = False

    def setPrecision(self, tau):
        self.core.set_parameters([tau])
        self.known = False

    def storeState(self):
        self.stored_log_likelihood = self.log_likelihood
        self.core.store_state()

    def restoreState(self):
        self.log_likelihood, self.known = self.stored_log_likelihood, True
        self.core.restore_state()

    def acceptState(self):
        self.core.accept_state()

    def makeDirty(self):
        self.known = False
        self.core.make_dirty()

    def getLogLikelihood(self):
        if not self.known:
            self.log_likelihood, self.known = float(self.core.log_likelihood(self.count)), True
        return self.log_likelihood


def both(mds, n, d, truncated, seed, missing=0.05):
    x, y = ref.synthetic(n, d, seed, missing=missing)
    return (mds.MultiDimensionalScalingLikelihood(d, y, x, TAU, left_truncated=truncated), Restated(d, y, x, TAU, truncated), x, y)


def check_sum_and_gradient(device, restated, label):
    s = device.native.getSumOfIncrements(device.instance)
    s_ref, scale = float(restated.core.sum_of_increments()), float(restated.core.absolute_sum())
    print("%s: S = %.12g, |S - S_ref| = %.3e, 1e-10 sum|increment| = %.3e" % (label, s, abs(s - s_ref), 1e-10 * scale))
    assert abs(s - s_ref) <= 1e-10 * scale
    logl, logl_ref = device.getLogLikelihood(), restated.getLogLikelihood()
    assert device.observation_count == restated.count
    print("%s: log L = %.12g, relative difference %.3e" % (label, logl, abs(logl - logl_ref) / max(abs(logl_ref), 1e-300)))
    assert abs(logl - logl_ref) <= 1e-10 * abs(logl_ref)
    g = device.getGradientLogDensity().reshape(device.location_count, device.dimension)
    g_ref, rows = restated.core.gradient()
    worst = float(np.max(np.abs(g - g_ref) / np.maximum(rows, 1e-300))) if rows.any() else 0.0
    print("%s: gradient, worst |g - g_ref| / row's absolute sum = %.3e" % (label, worst))
    assert np.all(np.abs(g - g_ref) <= 1e-10 * rows)


@pytest.mark.parametrize("truncated", [False, True])
@pytest.mark.parametrize("d", [1, 2, 3, 6])
@pytest.mark.parametrize("n", [1, 2, 3, 64, 65, 257, 1000, 4097])
def test_sum_log_likelihood_and_gradient_against_the_restatement(mds, n, d, truncated):
    for missing in (0.05, 0.0):
        device, restated, x, y = both(mds, n, d, truncated, seed=1000 * d + n, missing=missing)
        try:
            check_sum_and_gradient(device, restated, "N = %d D = %d truncated = %s missing = %s" % (n, d, truncated, missing))
            assert np.array_equal(device.native.getPairwiseData(device.instance), y.reshape(-1), equal_nan=True)
            assert device.internal_dimension == d
        finally:
            device.close()


@pytest.mark.parametrize("truncated", [False, True])
def test_all_missing_table_and_coincident_locations(mds, truncated):
    device, restated, x, y = both(mds, 65, 2, truncated, seed=3, missing=1.0)
    try:
        assert device.observation_count == 0 and device.native.getSumOfIncrements(device.instance) == 0.0
        assert device.getLogLikelihood() == 0.0 and not device.getGradientLogDensity().any()
    finally:
        device.close()
    device, restated, x, y = both(mds, 65, 3, truncated, seed=4, missing=0.0)
    try:
        x[7] = x[3]
        x[64] = x[0]
        device.setLocations(x)
        restated.setLocations(x)
        check_sum_and_gradient(device, restated, "coincident, truncated = %s" % truncated)
        assert np.all(np.isfinite(device.getGradientLogDensity()))
    finally:
        device.close()


def run_chain(mds, likelihoods, x, tau, steps, seed, each_step=None):
    """One chain of proposals applied in lockstep to every likelihood of the list (the first is the device's through the C ABI).
    Returns per step the list's log likelihoods after the proposal."""
    rng = np.random.default_rng(seed)
    n, d = x.shape
    x, values = x.copy(), []
    for like in likelihoods:
        like.getLogLikelihood()
    for step in range(1, steps + 1):
        if step % 50 == 10:
            # makeDirty BETWEEN proposals: inside one, after the row update, the Java core's full evaluation would fill the other
            # rows' column k from the proposed location, and a restore brings back row k only (MultiDimensionalScalingCoreImpl.java:
            # 198-199) — its table, and with it the restatement's, is stale from then on.  The library has no table to go stale.
            for like in likelihoods:
                like.makeDirty()
        before = [like.getLogLikelihood() for like in likelihoods]
        if step % 50 == 10 and each_step:
            each_step(step, "dirty", x, tau, before)
        for like in likelihoods:
            like.storeState()
        x_new, tau_new, kind = x.copy(), tau, "one"
        if step % 50 == 0:
            kind = "two"
            for k in rng.choice(n, size=2, replace=False):
                x_new[k] += rng.normal(0.0, 0.3, size=d)
                for like in likelihoods:
                    like.setLocation(int(k), x_new[k])
        elif step % 25 == 0:
            kind, tau_new = "tau", tau * float(np.exp(rng.normal(0.0, 0.1)))
            for like in likelihoods:
                like.setPrecision(tau_new)
        elif step % 20 == 0:
            kind = "all"
            x_new += rng.normal(0.0, 0.05, size=x.shape)
            for like in likelihoods:
                like.setLocations(x_new)
        else:
            k = int(rng.integers(n))
            x_new[k] += rng.normal(0.0, 0.3, size=d)
            for like in likelihoods:
                like.setLocation(k, x_new[k])
        values.append([like.getLogLikelihood() for like in likelihoods])
        if each_step:
            each_step(step, kind, x_new, tau_new, values[-1])
        if rng.random() < 0.5:
            for like in likelihoods:
                like.acceptState()
            x, tau = x_new, tau_new
        else:
            for like in likelihoods:
                like.restoreState()
            after = [like.getLogLikelihood() for like in likelihoods]
            assert [np.float64(v).tobytes() for v in after] == [np.float64(v).tobytes() for v in before]
            if each_step:
                each_step(step, "restored", x, tau, after)
    return values


@pytest.mark.parametrize("truncated", [False, True])
def test_a_chain_in_lockstep_with_the_restatement(mds, truncated):
    n, d = 300, 3
    device, restated, x, y = both(mds, n, d, truncated, seed=77)
    scratch = mds.MultiDimensionalScalingLikelihood(d, y, x, TAU, left_truncated=truncated)
    seen = {"row": 0, "all": 0, "known": 0, "worst": 0.0}
    sums = {}

    def each_step(step, kind, x_now, tau_now, logl):
        got, want = logl
        stats = device.stats()
        if kind == "restored":
            # the sum itself comes back with the stored bits, and costs nothing
            assert np.float64(device.native.getSumOfIncrements(device.instance)).tobytes() == sums["before"]
            assert device.stats()["last_path"] == mds.PATH_KNOWN
            return
        if kind == "dirty":
            assert abs(got - want) <= 1e-10 * abs(want) and stats["last_path"] == mds.PATH_ALL and stats["last_launches"] == 2, step
            return
        sums["before"] = sums.get("now", None)
        seen["worst"] = max(seen["worst"], abs(got - want) / abs(want))
        assert abs(got - want) <= 1e-10 * abs(want), (step, kind)
        path = {mds.PATH_ROW: "row", mds.PATH_ALL: "all", mds.PATH_KNOWN: "known"}[stats["last_path"]]
        seen[path] += 1
        if kind == "one" and restated.core.paths[-1] == "row":
            assert path == "row" and stats["last_launches"] == 1, (step, stats)
        if kind in ("two", "all"):
            assert path == "all" and stats["last_launches"] == 2
        if kind == "tau":
            assert path == ("all" if truncated else "known")
        scratch.setLocations(x_now)
        scratch.setPrecision(tau_now)
        scratch.makeDirty()
        fresh = scratch.getLogLikelihood()
        assert abs(got - fresh) <= 1e-10 * abs(fresh), (step, kind)
        if step % 50 == 30:
            g = device.getGradientLogDensity().reshape(n, d)
            g_ref, rows = restated.core.gradient()
            assert np.all(np.abs(g - g_ref) <= 1e-10 * rows), step

    def remember(step, kind, x_now, tau_now, logl):
        if kind != "restored":
            each_step(step, kind, x_now, tau_now, logl)
            sums["now"] = np.float64(device.native.getSumOfIncrements(device.instance)).tobytes()
        else:
            each_step(step, kind, x_now, tau_now, logl)
            sums["now"] = sums["before"]

    try:
        sums["now"] = np.float64(device.native.getSumOfIncrements(device.instance)).tobytes()
        run_chain(mds, [device, restated], x, TAU, 400, seed=5, each_step=remember)
        print("truncated = %s: %d row updates, %d full evaluations, %d known; worst relative difference of log L %.3e"
              % (truncated, seen["row"], seen["all"], seen["known"], seen["worst"]))
        assert seen["row"] >= 300
    finally:
        device.close()
        scratch.close()


@pytest.mark.parametrize("truncated", [False, True])
def test_the_same_inputs_give_the_same_bits(mds, truncated):
    n, d = 1000, 3
    x, y = ref.synthetic(n, d, seed=9)
    a = mds.MultiDimensionalScalingLikelihood(d, y, x, TAU, left_truncated=truncated)
    b = mds.MultiDimensionalScalingLikelihood(d, y, x, TAU, left_truncated=truncated)
    try:
        s_a, s_b = a.native.getSumOfIncrements(a.instance), b.native.getSumOfIncrements(b.instance)
        g_a, g_b = a.getGradientLogDensity(), b.getGradientLogDensity()
        assert np.float64(s_a).tobytes() == np.float64(s_b).tobytes() and g_a.tobytes() == g_b.tobytes()
        a.makeDirty()
        assert np.float64(a.native.getSumOfIncrements(a.instance)).tobytes() == np.float64(s_a).tobytes()
        assert a.stats()["last_path"] == mds.PATH_ALL and a.getGradientLogDensity().tobytes() == g_a.tobytes()
        # a single-location step takes the row path in one launch, on both instances with the same bits
        moved = x[17] + 0.25
        for like in (a, b):
            like.storeState()
            like.setLocation(17, moved)
        before = a.stats()
        s_a, s_b = a.native.getSumOfIncrements(a.instance), b.native.getSumOfIncrements(b.instance)
        after = a.stats()
        assert np.float64(s_a).tobytes() == np.float64(s_b).tobytes()
        assert after["last_path"] == mds.PATH_ROW and after["last_launches"] == 1
        assert after["row_updates"] == before["row_updates"] + 1 and after["launches"] == before["launches"] + 1
        assert after["full_evaluations"] == before["full_evaluations"]
        assert a.getGradientLogDensity().tobytes() == b.getGradientLogDensity().tobytes()
    finally:
        a.close()
        b.close()


def test_instance_numbers_count_from_zero_in_a_new_process(mds):
    script = ("import sys; sys.path.insert(0, %r); from beast_mcmc_amd import mds; m = mds.NativeMDS(); "
              "print([m.initialize(2, 10, 1), m.initialize(3, 5, 33), m.initialize(1, 7, 0)])" % ROOT)
    out = subprocess.run([sys.executable, "-c", script], check=True, capture_output=True, text=True, timeout=300).stdout
    assert out.strip().splitlines()[-1] == "[0, 1, 2]"


def test_two_instances_from_two_threads(mds):
    results, errors = {}, []

    def work(tag, truncated):
        try:
            device, restated, x, y = both(mds, 257, 2, truncated, seed=50 + tag)
            values = run_chain(mds, [device, restated], x, TAU, 60, seed=tag)
            results[tag] = max(abs(a - b) / abs(b) for a, b in values)
            device.close()
        except Exception as exc:                                        # noqa: BLE001 — reported below, in the main thread
            errors.append((tag, repr(exc)))

    threads = [threading.Thread(target=work, args=(t, bool(t))) for t in (0, 1)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    assert results[0] <= 1e-10 and results[1] <= 1e-10


def test_errors(mds):
    native = mds.NativeMDS()
    raw = native.raw
    assert raw.mdsStoreState(10 ** 6) == -4 and raw.mdsStoreState(-1) == -4
    assert raw.mdsInitialize(0, 10, 0, -1, 0) == -5 and raw.mdsInitialize(2, 0, 0, -1, 0) == -5
    assert raw.mdsInitialize(9, 10, 0, -1, 0) == -7
    assert raw.mdsInitializeLayout(2, 10, 12, 0, -1, 0) == -7
    i = native.initialize(2, 10, mds.USE_NATIVE_MDS | mds.SINGLE_PRECISION | mds.MULTI_CORE | mds.OPENCL_VECTORIZATION)
    short = np.zeros(200)
    p = short.ctypes.data_as(mds._D)
    assert raw.mdsUpdateLocations(i, -1, p, 19) == -5 and raw.mdsUpdateLocations(i, 3, p, 1) == -5
    assert raw.mdsUpdateLocations(i, 10, p, 2) == -5 and raw.mdsUpdateLocations(i, -2, p, 20) == -5
    assert raw.mdsUpdateLocations(i, -1, None, 20) == -5
    assert raw.mdsSetPairwiseData(i, p, 99) == -5 and raw.mdsGetPairwiseData(i, p, 99) == -5
    assert raw.mdsSetParameters(i, p, 0) == -5 and raw.mdsGetLocationGradient(i, p, 19) == -5
    assert raw.mdsGetSumOfIncrements(i, None) == -5
    assert raw.mdsGetObservationGradient(i, p, 100) == -7
    assert raw.mdsUpdateLocations(i, -1, p, 200) == 0 and raw.mdsGetInternalDimension(i) == 2 and raw.mdsGetLocationCount(i) == 10
    with pytest.raises(mds.MDSError) as e:
        native.getObservationGradient(i, short)
    assert e.value.code == -7
    native.finalize(i)
    assert raw.mdsFinalize(i) == -4 and raw.mdsStoreState(i) == -4 and raw.mdsGetInternalDimension(i) == -4
    out = mds.C.c_double(0.0)
    assert raw.mdsGetSumOfIncrements(i, mds.C.byref(out)) == -4
    j = native.initialize(2, 10, 0)
    assert j == i + 1                                                    # numbers are not reused
    native.finalize(j)


class ThroughTheNatives:
    """beast_mcmc_amd.mds.NativeMDS's method set, every call made through the Java_..._NativeMDSSingleton_* natives of the library
    the way a JVM makes it."""

    def __init__(self, mds):
        self.env, self.lib, self.mds = jni_env_mds.MdsJniEnv(), mds.library(), mds

    def _call(self, name, *args):
        out = self.env.call(self.lib, name, *args)
        if self.env.thrown:
            function, code = self.env.thrown[0][1].split(": ")
            raise self.mds.MDSError(function, int(code))
        self.env.assert_clean()
        return out

    def initialize(self, dimension, count, flags, device=-1, threads=0):
        return self._call("initialize__IIJII", dimension, count, flags, device, threads)

    def updateLocations(self, instance, index, values):
        self._call("updateLocations", instance, index, np.ascontiguousarray(values, dtype=np.float64).reshape(-1))

    def setPairwiseData(self, instance, y):
        self._call("setPairwiseData", instance, np.ascontiguousarray(y, dtype=np.float64).reshape(-1))

    def setParameters(self, instance, p):
        self._call("setParameters", instance, np.asarray(p, dtype=np.float64))

    def getLocationGradient(self, instance, out):
        self._call("getLocationGradient", instance, out)

    def finalize(self, instance):
        assert self.lib.mdsFinalize(instance) == 0                        # (the Java side never frees)

    def stats(self, instance):
        return self.mds.NativeMDS.stats(self.mds.NativeMDS(), instance)

    def __getattr__(self, name):
        if name in ("getSumOfIncrements", "storeState", "restoreState", "acceptState", "makeDirty", "getPairwiseData", "getInternalDimension"):
            return lambda instance: self._call(name, instance)
        raise AttributeError(name)


@pytest.mark.parametrize("truncated", [False, True])
def test_the_natives_end_to_end(mds, truncated):
    n, d = 120, 2
    x, y = ref.synthetic(n, d, seed=21)
    direct = mds.MultiDimensionalScalingLikelihood(d, y, x, TAU, left_truncated=truncated)
    jvm = mds.MultiDimensionalScalingLikelihood(d, y, x, TAU, left_truncated=truncated, native=ThroughTheNatives(mds))
    try:
        values = run_chain(mds, [direct, jvm], x, TAU, 20, seed=8)
        assert all(np.float64(a).tobytes() == np.float64(b).tobytes() for a, b in values)
        assert direct.getGradientLogDensity().tobytes() == jvm.getGradientLogDensity().tobytes()
        assert np.array_equal(jvm.native.getPairwiseData(jvm.instance), y.reshape(-1), equal_nan=True)
        with pytest.raises(mds.MDSError) as e:
            jvm.native._call("getObservationGradient", jvm.instance, np.zeros(4))
        assert e.value.code == -7
        with pytest.raises(mds.MDSError) as e:
            jvm.native._call("initialize__IIIJII", 2, 5, 6, 1, -1, 0)
        assert e.value.code == -7
    finally:
        direct.close()
        jvm.close()
