"""Reversible models decomposed on the device in one call (include/beagle_mi355.h beagleMi355SetReversibleModels; csrc/kernels_eigen.hip)
against the numpy restatement of the kernel's iteration and the longdouble yardstick (tests/eigen_reference.py, pinned on the CPU
tier), the call's protocol, and branch-specific evaluations through eigensystems.SubstitutionModelSet against the CPU oracle."""
import ctypes as C
import os

import numpy as np
import pytest

import beast_mcmc_amd as bm
import eigen_reference as er
import helpers
from beast_mcmc_amd.inputs import substmodel

pytestmark = pytest.mark.gpu

EPS = np.finfo(float).eps
NONE = bm.beagle.NONE


def instance(S, eigens, complex_eigen=False, resource_list=(1,), slots=8):
    """2 tips x 16 patterns, 4 categories: enough to turn an eigen slot into transition matrices and site likelihoods."""
    b = bm.beagle.Beagle(2, 3, 2, S, 16, eigens, slots, 4, 0, resourceList=resource_list,
                         requirementFlags=bm.beagle.FLAG_EIGEN_COMPLEX if complex_eigen else 0)
    b.setCategoryRates(er.CATEGORY_RATES)
    return b


def sharded_instance(S, eigens, shards=3):
    """(as tests/test_gpu_sharded_instance.py builds it: three shards on the one device)"""
    old = os.environ.get("BEAGLE_MI355_SHARDS")
    os.environ["BEAGLE_MI355_SHARDS"] = str(shards)
    try:
        g = len(bm.beagle.engine().resource_list()) - 2
        return instance(S, eigens, resource_list=(g + 1,))
    finally:
        if old is None:
            os.environ.pop("BEAGLE_MI355_SHARDS", None)
        else:
            os.environ["BEAGLE_MI355_SHARDS"] = old


def device_p(b, eigen_index):
    """-> [len(LENGTHS)][C][S][S]: P(t rate_c) from the slot, as every evaluation forms it."""
    n = len(er.LENGTHS)
    b.updateTransitionMatrices(eigen_index, np.arange(n), None, None, er.LENGTHS, n)
    return np.stack([b.getTransitionMatrix(k) for k in range(n)])


@pytest.mark.parametrize("S", er.STATES + [6] + er.BOUNDARY_STATES)
def test_accuracy_against_the_longdouble_yardstick(S):
    """One call over the models of this state count, then per model: |U U^-1 - I|, |U L U^-1 - Q/n| / |Q/n| and max |P_dev - P_ld| over
    t in {0, 1e-3, 0.11, 0.9, 25} x four category rates, each at most 8 max(e_ref, S eps) with e_ref what the float64 restatement
    loses against longdouble on the same input (check_case's rule and factor).  Beside the shape table's state counts: the reducible
    6-state model, and the state counts on either side of the workgroup kernel's register sizes."""
    models = [m for m in er.accuracy_models() if m[0] == S]
    b = instance(S, len(models))
    b.setReversibleModels(np.arange(len(models)), np.stack([m[2] for m in models]), np.stack([m[3] for m in models]))
    stats = b.eigenStats()
    assert stats["calls"] == 1 and stats["models"] == len(models) and stats["capped"] == 0 and 1 <= stats["max_sweeps"] <= 15
    failures = []
    for k, (_, name, r, pi) in enumerate(models):
        u, ui, lam = b.getEigenDecomposition(k)
        assert np.all(np.isfinite(lam)) and np.all(np.diff(lam) >= 0)
        ref = er.decompose(r, pi)
        dev = er.Decomposition(u, ui, lam, 0, False)
        ident, recon = er.residuals(dev, r, pi)
        ident_ref, recon_ref = er.residuals(ref, r, pi)
        got = device_p(b, k)
        p_err = p_ref = 0.0
        for a, t in enumerate(er.LENGTHS):
            for c, rate in enumerate(er.CATEGORY_RATES):
                yard = er.yardstick_p(r, pi, t * rate)
                p_err = max(p_err, float(np.max(np.abs(got[a, c] - yard))))
                p_ref = max(p_ref, float(np.max(np.abs(er.transition_probabilities(ref, t * rate) - yard))))
        rows = (("identity", ident, ident_ref), ("reconstruction", recon, recon_ref), ("P(t)", p_err, p_ref))
        for what, err, e_ref in rows:
            bound = 8 * max(e_ref, S * EPS)
            print("S = %d %s %s: device %.3e  e_ref %.3e  bound %.3e  ratio %.3f  (%d sweeps in the restatement)"
                  % (S, name, what, err, e_ref, bound, err / bound, ref.sweeps))
            if not err <= bound:
                failures.append((name, what, err, bound))
    b.finalize()
    assert not failures, failures


def evaluation_setup(b, S):
    rng = np.random.default_rng(S)
    for t in range(2):
        b.setTipStates(t, rng.integers(0, S, size=16))
    b.setPatternWeights(np.ones(16))
    b.setStateFrequencies(0, np.full(S, 1.0 / S))
    b.setCategoryWeights(0, np.full(4, 0.25))


def site_values(b, eigen_index):
    """The 16 site log-likelihoods of the two-tip tree under the slot's model: every shard of a sharded handle answers for its patterns."""
    b.updateTransitionMatrices(eigen_index, [0, 1], None, None, [0.11, 0.9], 2)
    b.updatePartials([2, NONE, NONE, 0, 0, 1, 1], 1, NONE)
    out = [0.0]
    b.calculateRootLogLikelihoods([2], [0], [0], [NONE], 1, out)
    return b.getSiteLogLikelihoods().copy()


def read_slots(b, slots):
    return [np.concatenate([x.ravel() for x in b.getEigenDecomposition(int(s))]) for s in slots]


@pytest.mark.parametrize("S,count", [(4, 257), (20, 33)])
def test_same_bits_whatever_the_list_the_split_and_the_shard(S, count, monkeypatch):
    rng = np.random.default_rng(7 * S)
    rates = np.stack([er.random_model(S, rng)[0] for _ in range(count)])
    freqs = np.stack([er.random_model(S, rng)[1] for _ in range(count)])
    b = instance(S, 2 * count)
    every = np.arange(count)
    b.setReversibleModels(every, rates, freqs)
    first = read_slots(b, every)
    assert b.eigenStats()["models"] == count
    for k in every:                                            # one by one, into other slots
        b.setReversibleModels([count + k], rates[k:k + 1], freqs[k:k + 1])
    for k, got in enumerate(read_slots(b, count + every)):
        assert np.array_equal(got, first[k]), k
    b.setReversibleModels(count + every[::-1], rates[::-1], freqs[::-1])                     # the list reversed: model k is entry count - 1 - k
    for k, got in enumerate(read_slots(b, count + every)):
        assert np.array_equal(got, first[k]), k
    monkeypatch.setenv("BEAGLE_MI355_EIGEN_CHUNK", "7")        # several launches of one call
    b.setReversibleModels(count + every, rates, freqs)
    monkeypatch.delenv("BEAGLE_MI355_EIGEN_CHUNK")
    for k, got in enumerate(read_slots(b, count + every)):
        assert np.array_equal(got, first[k]), k
    stats = b.eigenStats()
    assert stats["calls"] == 3 + count and stats["models"] == 4 * count and stats["capped"] == 0 and stats["max_sweeps"] <= 15
    # the sharded handle: the slot one shard answers with, and — through the site values, which every shard forms for its own
    # patterns from its own copy of the slot — every shard's
    many = sharded_instance(S, count)
    many.setReversibleModels(every, rates, freqs)
    for k, got in enumerate(read_slots(many, every)):
        assert np.array_equal(got, first[k]), k
    evaluation_setup(b, S); evaluation_setup(many, S)
    for k in every[::16]:
        assert np.array_equal(site_values(many, int(k)), site_values(b, int(k))), k
    many.finalize(); b.finalize()


def test_a_later_set_eigen_decomposition_is_not_skipped():
    """setEigenDecomposition(X), the device call into the same slot, setEigenDecomposition(X) again: the slot holds X (the host's
    record of what the slot holds is dropped by the call)."""
    rng = np.random.default_rng(3)
    x, _ = substmodel.random_reversible(5, rng)
    r, pi = er.random_model(5, rng)
    b = instance(5, 2)
    as_set = np.concatenate([x.evec.ravel(), x.ievc.ravel(), x.evals])
    b.setEigenDecomposition(1, x.evec, x.ievc, x.evals)
    assert np.array_equal(read_slots(b, [1])[0], as_set)       # (the getter serves slots filled either way)
    b.setReversibleModels([1], [r], [pi])
    assert not np.array_equal(read_slots(b, [1])[0], as_set)
    b.setEigenDecomposition(1, x.evec, x.ievc, x.evals)
    assert np.array_equal(read_slots(b, [1])[0], as_set)
    b.finalize()


@pytest.mark.parametrize("S", [4, 20])
def test_complex_instance_gets_zero_imaginary_parts(S):
    rng = np.random.default_rng(S)
    r, pi = er.random_model(S, rng)
    real, cplx = instance(S, 2), instance(S, 2, complex_eigen=True)
    real.setReversibleModels([1], [r], [pi]); cplx.setReversibleModels([1], [r], [pi])
    u, ui, lam = real.getEigenDecomposition(1)
    cu, cui, clam = cplx.getEigenDecomposition(1)
    assert clam.shape == (2 * S,) and not np.any(clam[S:]) and not np.any(np.signbit(clam[S:]))
    assert np.array_equal(cu, u) and np.array_equal(cui, ui) and np.array_equal(clam[:S], lam)
    p_real, p_cplx = device_p(real, 1), device_p(cplx, 1)
    # the complex kernel multiplies by cos(0 t) = 1 and adds sin(0 t) = 0 terms: the same values to rounding
    assert np.max(np.abs(p_real - p_cplx)) <= 8 * S * EPS
    real.finalize(); cplx.finalize()


def test_refusals_leave_the_slots_as_they_were():
    S = 4
    rng = np.random.default_rng(1)
    b = instance(S, 3)
    held = [substmodel.random_reversible(S, rng)[0] for _ in range(3)]
    for k, e in enumerate(held):
        b.setEigenDecomposition(k, e.evec, e.ievc, e.evals)
    before = read_slots(b, range(3))
    rates = np.stack([er.random_model(S, rng)[0] for _ in range(2)])
    freqs = np.stack([er.random_model(S, rng)[1] for _ in range(2)])
    f = b._ext("beagleMi355SetReversibleModels", [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int])
    ptr = lambda a: None if a is None else a.ctypes.data

    def call(idx=(0, 2), count=2, r=rates, pi=freqs, flags=0):
        idx = None if idx is None else np.ascontiguousarray(idx, dtype=np.int32)
        r = None if r is None else np.ascontiguousarray(r, dtype=np.float64)
        pi = None if pi is None else np.ascontiguousarray(pi, dtype=np.float64)
        return f(b.instance, ptr(idx), count, ptr(r), ptr(pi), flags)

    def refused(code, **change):
        assert call(**change) == code, change
        for got, want in zip(read_slots(b, range(3)), before):
            assert np.array_equal(got, want)

    def with_entry(a, where, value):
        a = a.copy()
        a[where] = value
        return a

    refused(-5, idx=None)
    refused(-5, r=None)
    refused(-5, pi=None)
    refused(-5, count=-1)
    refused(-5, idx=(0, 3))
    refused(-5, idx=(-1, 2))
    refused(-5, idx=(2, 2))                                    # a slot named twice
    refused(-5, flags=1)
    for bad in (0.0, -0.1, np.nan, np.inf):
        refused(-5, pi=with_entry(freqs, (1, 2), bad))
    for bad in (-1e-300, np.nan, np.inf):
        refused(-5, r=with_entry(rates, (1, 5), bad))
    refused(-5, r=with_entry(rates, 1, 0.0))                   # all rates zero: n is not > 0
    assert call(count=0) == 0 and call(idx=None, r=None, pi=None, count=0) == 0
    for got, want in zip(read_slots(b, range(3)), before):
        assert np.array_equal(got, want)
    assert b.eigenStats() == {"calls": 0, "models": 0, "max_sweeps": 0, "capped": 0}
    g = b._ext("beagleMi355GetEigenDecomposition", [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p])
    out = np.zeros(16)
    assert g(b.instance, 3, ptr(out), ptr(out), ptr(out)) == -5 and g(b.instance, 0, None, ptr(out), ptr(out)) == -5
    assert call() == 0                                         # ... and the call as it stands is accepted
    after = read_slots(b, range(3))
    assert not np.array_equal(after[0], before[0]) and np.array_equal(after[1], before[1]) and not np.array_equal(after[2], before[2])
    b.finalize()
    big = bm.beagle.Beagle(2, 3, 2, 65, 4, 1, 4, 1, 0)
    with pytest.raises(bm.beagle.BeagleException) as e:
        big.setReversibleModels([0], [np.ones(65 * 32)], [np.full(65, 1 / 65)])
    assert e.value.code == -7
    big.finalize()


@pytest.mark.parametrize("kind", ["hky", "gy94"])
def test_branch_specific_likelihood_matches_the_oracle_and_the_host_route(kind, oracle_lib):
    """8 taxa x 64 patterns x 4 categories, a model per branch (HKY kappa at 4 states, GY94 omega at 61) through
    updateTransitionMatricesWithMultipleModels: lnL with the device route against the CPU oracle fed the host route's eigen systems,
    and against the host route on the engine itself, to the project's 1e-10 relative; twice, so that both sets of eigen buffers serve."""
    _, dev_models, dev = er.branch_model_plan(kind, None, "device")
    _, host_models, host = er.branch_model_plan(kind, None, "host")
    _, oracle_models, oracle = er.branch_model_plan(kind, oracle_lib, "host")
    for attempt in range(2):
        got, same_engine, want = dev.log_likelihood(), host.log_likelihood(), oracle.log_likelihood()
        print("%s: lnL device route %.12f  host route %.12f  oracle %.12f" % (kind, got, same_engine, want))
        assert helpers.rel_err(got, want) <= 1e-10
        assert helpers.rel_err(got, same_engine) <= 1e-10
        for m in (dev_models, host_models, oracle_models):
            m.dirty[:] = True
    stats = dev.b.eigenStats()
    edges = dev.tree.node_count - 1
    assert stats == {"calls": 2, "models": 2 * edges, "max_sweeps": stats["max_sweeps"], "capped": 0} and 1 <= stats["max_sweeps"] <= 15
    dev.close(); host.close(); oracle.close()
