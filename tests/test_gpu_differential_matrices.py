"""Substitution-parameter differential matrices formed on the device in one call (include/beagle_mi355.h
beagleMi355UpdateDifferentialMatrices; csrc/kernels_differential.hip) against the numpy restatement of the reference's
getExactDifferentialMassMatrix (tests/differential_matrices_reference.py, pinned on the CPU tier against finite differences of P), and
the gradients built on them (beast_mcmc_amd.substgradient) against the host route on the CPU oracle."""
import os

import numpy as np
import pytest

import beast_mcmc_amd as bm
import differential_matrices_reference as dr
import helpers
from beast_mcmc_amd import substgradient as sg
from beast_mcmc_amd.inputs import substmodel
from differential_matrices_reference import CODON_PI, complex_case, three_class_plan

pytestmark = pytest.mark.gpu

EPS = np.finfo(float).eps
EXACT, FIRST_ORDER = dr.EXACT, dr.FIRST_ORDER
LENGTHS = np.array([0.0, 1e-3, 0.11, 0.9, 25.0])         # one branch of length 0 (D is all zeros), one long
RATE_SETS = 3


class Case:
    """An instance of S states and C categories with `eigens` eigen systems (and as many rate sets) and the differentials `dq`, plus
    the restatement of any slot, cached by what it depends on."""

    def __init__(self, S, C, eigens, dq, complex_eigen=False, slots=300, resource_list=(1,)):
        self.S, self.C, self.eigens, self.dq = S, C, eigens, np.ascontiguousarray(dq)
        self.b = bm.beagle.Beagle(2, 3, 2, S, 16, max(RATE_SETS, len(eigens)), slots, C, 0, resourceList=resource_list,
                                  requirementFlags=bm.beagle.FLAG_EIGEN_COMPLEX if complex_eigen else 0)
        for k, e in enumerate(eigens):
            self.b.setEigenDecomposition(k, e.evec, e.ievc, e.evals)
        rng = np.random.default_rng(7)
        self.rates = [np.sort(rng.gamma(2.0, 0.5, size=C)) for _ in range(RATE_SETS)]
        for k, r in enumerate(self.rates):
            self.b.setCategoryRatesWithIndex(k, r)
        self._cache = {}
        gap = max(float(np.ptp(e.evals[:S])) for e in eigens)
        assert LENGTHS.max() * max(r.max() for r in self.rates) * gap <= 600.0      # (beyond exp's range the reference's value is not pinned)

    def expect(self, eig, rate_set, diff, length, mode, dtype=np.float64):
        key = (eig, rate_set, diff, float(length), mode, dtype)
        if key not in self._cache:
            e = self.eigens[eig]
            self._cache[key] = dr.slot(e.evec, e.ievc, e.evals, self.dq[diff], length, self.rates[rate_set], mode, dtype)
        return self._cache[key]

    def guard(self):
        for e in self.eigens:
            for q in self.dq:
                dr.assert_guard(dr.rotate(e.evec, e.ievc, q)[1], e.evals, self.S)

    def close(self):
        self.b.finalize()


def branch_lists(count, mixed, n_eig, n_diff, seed=3):
    rng = np.random.default_rng(seed + count)
    slots = rng.permutation(300)[:count].astype(np.int32)
    lengths = LENGTHS[np.arange(count) % len(LENGTHS)]
    if not mixed:
        return None, None, None, slots, lengths
    return (rng.integers(0, n_eig, count).astype(np.int32), rng.integers(0, RATE_SETS, count).astype(np.int32),
            rng.integers(0, n_diff, count).astype(np.int32), slots, lengths)


def check_case(case, count, mixed, mode):
    """max |D_dev - D_64| / max |D_64| <= 8 max(e_ref, S eps) for every matrix of the call, e_ref = the largest max |D_64 - D_ld| /
    max |D_ld| of the case: what float64 itself loses, with a factor 8 for the device's other association (two products where the
    reference has four, blocked sums)."""
    eig, rate, diff, slots, lengths = branch_lists(count, mixed, len(case.eigens), len(case.dq))
    case.b.updateDifferentialMatrices(eig, rate, case.dq, diff, slots, lengths, count, mode)
    e_ref, worst = 0.0, 0.0
    rows = []
    for k in range(count):
        key = (0 if eig is None else int(eig[k]), 0 if rate is None else int(rate[k]), 0 if diff is None else int(diff[k]), lengths[k], mode)
        d64, dld = case.expect(*key), case.expect(*key, dtype=np.longdouble)
        got = case.b.getTransitionMatrix(int(slots[k]))
        if lengths[k] == 0.0:
            assert not np.any(got) and not np.any(d64)
            continue
        for c in range(case.C):
            scale = float(np.max(np.abs(d64[c])))
            e_ref = max(e_ref, float(np.max(np.abs(d64[c] - dld[c])) / np.max(np.abs(dld[c]))))
            rows.append(float(np.max(np.abs(got[c] - d64[c]))) / scale)
    worst = max(rows) if rows else 0.0
    bound = 8 * max(e_ref, case.S * EPS)
    print("S = %d C = %d count = %d %s mode %d: device error %.3e  e_ref %.3e  bound %.3e"
          % (case.S, case.C, count, "mixed" if mixed else "one pair", mode, worst, e_ref, bound))
    assert worst <= bound
    return worst, e_ref


def reversible_case(S, C, seed=11):
    rng = np.random.default_rng(seed + S)
    eigens, dq = [], []
    for _ in range(3):
        e, pi = substmodel.random_reversible(S, rng)
        eigens.append(e)
    for _ in range(2):
        dq.append(substmodel.reversible_q(rng.gamma(1.0, 1.0, size=S * (S - 1) // 2), rng.dirichlet(np.full(S, 5.0))))
    return Case(S, C, eigens, np.stack(dq))


STATES = [2, 3, 4, 5, 7, 8, 9, 16, 20, 61, 64]
SHAPES = ((1, ((1, False), (257, True))), (4, ((3, True), (257, False))))      # (categories, ((branches, mixed), ...))


def shape_table_errors(S):
    """-> (largest device error, largest e_ref) over the shape table at S states (tools/differential_matrices_bench.py records them)."""
    worst = [0.0, 0.0]
    for C, shapes in SHAPES:
        case = reversible_case(S, C)
        case.guard()
        for count, mixed in shapes:
            worst = [max(a, b) for a, b in zip(worst, check_case(case, count, mixed, EXACT))]
        check_case(case, 3, True, FIRST_ORDER)
        case.close()
    return tuple(worst)


@pytest.mark.parametrize("S", STATES)
def test_matrices_match_the_restatement(S):
    """Both dispatch paths and their boundary (one thread per matrix up to 8 states, one workgroup from 9), state counts that are no
    multiple of 4, 257 matrices past one 256-thread block, one (eigen, differential) pair and 3 x 2 of them mixed per branch, both modes."""
    shape_table_errors(S)


def complex_model(S, pairs):
    """The first seeded ComplexSubstitutionModel of S states with exactly `pairs` conjugate pairs."""
    for seed in range(400):
        make, theta = complex_case(S, seed)
        m = make(theta)
        if len(dr.split_eigenvalues(m.eig.evals, S)[3]) == pairs:
            return m
    raise AssertionError("no such model")


@pytest.mark.parametrize("S,pairs", [(5, 1), (6, 2), (10, 2)])
def test_complex_eigen_systems_match_the_restatement(S, pairs):
    """Conjugate pairs next to real eigenvalues: one pair at 5 states, two at 6 (one thread per matrix) and at 10 (one workgroup)."""
    m = complex_model(S, pairs)
    _, _, real, firsts = dr.split_eigenvalues(m.eig.evals, S)
    assert len(firsts) == pairs and len(real) == S - 2 * pairs and len(real) >= 1
    other = complex_model(S, pairs + 1 if S == 5 else pairs - 1)            # a second eigen system with another pair structure
    rng = np.random.default_rng(S)
    dq = np.stack([m.dq[0], substmodel.complex_q(rng.gamma(1.0, 1.0, size=S * (S - 1)), S)])
    for C in (1, 4):
        case = Case(S, C, [m.eig, other.eig, m.eig], dq, complex_eigen=True)
        case.guard()
        check_case(case, 1, False, EXACT)
        check_case(case, 257, True, EXACT)
        check_case(case, 3, True, FIRST_ORDER)
        case.close()


def read_slots(b, slots):
    return np.stack([b.getTransitionMatrix(int(s)) for s in slots])


@pytest.mark.parametrize("S", [4, 20])
def test_same_bits_repeated_permuted_split_and_sharded(S):
    case = reversible_case(S, 4)
    eig, rate, diff, slots, lengths = branch_lists(40, True, 3, 2)
    call = lambda b, sel: b.updateDifferentialMatrices(eig[sel], rate[sel], case.dq, diff[sel], slots[sel], lengths[sel], len(sel), EXACT)
    every = np.arange(40)
    call(case.b, every)
    first = read_slots(case.b, slots)
    call(case.b, every)
    assert np.array_equal(read_slots(case.b, slots), first)
    case.b.updateDifferentialMatrices(eig, rate, case.dq, diff, slots, np.zeros(40), 40, FIRST_ORDER)       # (the slots forget)
    call(case.b, np.random.default_rng(1).permutation(40))
    assert np.array_equal(read_slots(case.b, slots), first)
    case.b.updateDifferentialMatrices(eig, rate, case.dq, diff, slots, np.zeros(40), 40, FIRST_ORDER)
    call(case.b, every[:13]); call(case.b, every[13:])
    assert np.array_equal(read_slots(case.b, slots), first)
    # the sharded handle (as tests/test_gpu_sharded_instance.py builds it: three shards on the one device)
    old = os.environ.get("BEAGLE_MI355_SHARDS")
    os.environ["BEAGLE_MI355_SHARDS"] = "3"
    try:
        g = len(bm.beagle.engine().resource_list()) - 2
        many = Case(S, 4, case.eigens, case.dq, resource_list=(g + 1,))
    finally:
        if old is None:
            os.environ.pop("BEAGLE_MI355_SHARDS", None)
        else:
            os.environ["BEAGLE_MI355_SHARDS"] = old
    call(many.b, every)
    assert np.array_equal(read_slots(many.b, slots), first)
    many.close(); case.close()


@pytest.mark.parametrize("S", [4, 9])
def test_neighbouring_slots_are_untouched(S):
    case = reversible_case(S, 4)
    sentinel = np.random.default_rng(5).normal(size=(300, 4, S, S))
    for s in range(300):
        case.b.setTransitionMatrix(s, sentinel[s])
    slots = np.array([1, 2, 5, 17, 298], dtype=np.int32)
    for mode in (EXACT, FIRST_ORDER):
        case.b.updateDifferentialMatrices(None, None, case.dq, None, slots, LENGTHS, 5, mode)
        for s in range(300):
            assert np.array_equal(case.b.getTransitionMatrix(s), sentinel[s]) == (s not in slots), s
        for s in slots:
            case.b.setTransitionMatrix(int(s), sentinel[s])
    case.close()


def model_plan(kind, library, route):
    if kind == "hky":
        wl = helpers.random_workload(9, 300, 4, 4, seed=41)
        models = [sg.hky_kappa(k, wl.freqs) for k in (1.7, 3.2, 0.8)]
        classes = np.arange(wl.tree.node_count) % 3
    elif kind == "reversible20":
        wl = helpers.random_workload(8, 100, 20, 2, seed=42)
        rng = np.random.default_rng(42)
        models = [sg.reversible_rate(rng.gamma(1.0, 1.0, size=190) + 0.05, wl.freqs, [10, 120]) for _ in range(2)]      # (two exchangeabilities as parameters)
        classes = np.arange(wl.tree.node_count) % 2
    elif kind == "gy94":
        wl = helpers.random_workload(6, 70, 61, 1, seed=43)
        models, classes = [sg.gy94_omega(2.0, 0.4, CODON_PI)], None
    else:
        wl = helpers.random_workload(7, 120, 5, 3, seed=44)
        make, theta = complex_case(5, 0)
        models, classes = [make(theta), make(1.5 * theta)], np.arange(wl.tree.node_count) % 2
    return wl, sg.SubstitutionParameterGradient(wl, models, classes, route=route, library=library)


@pytest.mark.parametrize("kind", ["hky", "reversible20", "gy94", "complex5"])
def test_gradient_device_route_matches_host_route_on_the_oracle(kind, oracle_lib):
    """(S, C, T, P) = (4, 4, 9, 300), (20, 2, 8, 100), (61, 1, 6, 70) and a complex 5-state model, to the path's 1e-10 relative."""
    wl, dev = model_plan(kind, None, "device")
    _, host = model_plan(kind, oracle_lib, "host")
    for m in dev.models:
        for q in m.dq:
            dr.assert_guard(dr.rotate(m.eig.evec, m.eig.ievc, q)[1], m.eig.evals, dev.S)
    for _ in range(2):                       # (4 states: the second evaluation answers from the held pre-order list)
        ld, gd = dev.gradient()
        lh, gh = host.gradient()
        assert helpers.rel_err(ld, lh) <= 1e-10
        assert np.max(np.abs(gd - gh)) <= 1e-10 * max(1.0, float(np.max(np.abs(gh)))), (gd, gh)
    dev.close(); host.close()


def test_gradient_matches_finite_differences_on_the_engine():
    wl, kappas, g = three_class_plan(None, route="device", T=9, P=300, seed=41)
    lnl, grad = g.gradient()
    for k, kappa in enumerate(kappas):
        h = 1e-4 * kappa
        g.set_model(k, sg.hky_kappa(kappa + h, wl.freqs)); up = g.log_likelihood()
        g.set_model(k, sg.hky_kappa(kappa - h, wl.freqs)); dn = g.log_likelihood()
        g.set_model(k, sg.hky_kappa(kappa, wl.freqs))
        noise = 50 * EPS * abs(lnl) / h
        assert abs((up - dn) / (2 * h) - grad[k, 0]) <= 1e-5 * max(1.0, abs(grad[k, 0])) + noise
    g.close()


def test_held_pre_order_list_stays_held_unless_its_slots_are_written():
    """4 states: from an instance's second evaluation on, updatePrePartials is held back and calculateEdgeDifferentials answers from the
    held list.  The device call leaves it held, as setDifferentialMatrix does (the list reads no differential slot); written into a
    slot the list READS, a branch matrix, it makes the list run first, with the matrix it was issued with."""
    wl, kappas, g = three_class_plan(None, route="device", T=9, P=300, seed=41)
    _, _, h = three_class_plan(None, route="host", T=9, P=300, seed=41)
    g.gradient(); h.gradient()               # (the first evaluation of an instance runs its list together with the derivatives)
    _, gd = g.gradient()
    _, gh = h.gradient()
    assert np.max(np.abs(gd - gh)) <= 1e-10 * np.max(np.abs(gh))
    for x in (g, h):
        assert x.b.gradientStats() == {"fused": 1, "by_operation": 0, "walked": 1, "late": 0}
    dq = np.stack([m.dq[0] for m in g.models])
    g.b.updateDifferentialMatrices(None, None, dq, None, [g.matrix_index(int(g._nodes[0]))], [0.3], 1, EXACT)
    assert g.b.gradientStats()["late"] == 1
    g.set_differential_matrices(0)           # ... and the pre-order partials it wrote give the same derivatives
    s1, _, _ = g.b.calculateEdgeDifferentials(g._edge_post[g._set], g._pre_idx, g._d_idx, g._w0, len(g._nodes), want_squared=False)
    grad = np.zeros((3, 1))
    np.add.at(grad[:, 0], g._edge_model, s1)
    assert np.max(np.abs(grad - gh)) <= 1e-10 * np.max(np.abs(gh))
    assert g.b.gradientStats()["late"] == 1
    g.close(); h.close()


def test_return_codes():
    case = reversible_case(4, 2)
    b = case.b
    sentinel = np.random.default_rng(9).normal(size=(300, 2, 4, 4))
    for s in range(300):
        b.setTransitionMatrix(s, sentinel[s])
    ok = dict(eigenIndices=[0, 1], categoryRatesIndices=[0, 2], differentials=case.dq, differentialIndices=[1, 0], matrixIndices=[3, 4],
              edgeLengths=[0.1, 0.2], count=2, mode=EXACT)

    def refused(code, **change):
        with pytest.raises(bm.beagle.BeagleException) as e:
            b.updateDifferentialMatrices(**dict(ok, **change))
        assert e.value.code == code
        for s in (2, 3, 4, 5):
            assert np.array_equal(b.getTransitionMatrix(s), sentinel[s])

    refused(-5, eigenIndices=[0, 3])
    refused(-5, eigenIndices=[-1, 0])
    refused(-5, categoryRatesIndices=[0, 3])
    refused(-5, differentialIndices=[2, 0])
    refused(-5, matrixIndices=[3, 300])
    refused(-5, matrixIndices=[-1, 4])
    refused(-5, matrixIndices=[3, 3])                      # a slot named twice
    refused(-5, mode=2)
    refused(-5, mode=-1)
    import ctypes as C
    f = b._ext("beagleMi355UpdateDifferentialMatrices", [C.c_int] + [C.c_void_p] * 3 + [C.c_int] + [C.c_void_p] * 3 + [C.c_int, C.c_int])
    dq, slots, lens = np.ascontiguousarray(case.dq), np.array([3, 4], dtype=np.int32), np.array([0.1, 0.2])
    ptr = lambda a: a.ctypes.data
    assert f(b.instance, None, None, None, 2, None, ptr(slots), ptr(lens), 2, EXACT) == -5
    assert f(b.instance, None, None, ptr(dq), 2, None, None, ptr(lens), 2, EXACT) == -5
    assert f(b.instance, None, None, ptr(dq), 2, None, ptr(slots), None, 2, EXACT) == -5
    assert f(b.instance, None, None, ptr(dq), 0, None, ptr(slots), ptr(lens), 2, EXACT) == -5
    assert f(b.instance, None, None, None, 2, None, None, None, 0, EXACT) == 0          # count 0: success, nothing launched
    assert f(b.instance, None, None, ptr(dq), 2, None, ptr(slots), ptr(lens), -3, EXACT) == 0
    for s in (2, 3, 4, 5):
        assert np.array_equal(b.getTransitionMatrix(s), sentinel[s])
    assert f(b.instance, None, None, ptr(dq), 2, None, ptr(slots), ptr(lens), 2, EXACT) == 0     # ... and NULL index lists name 0
    assert not np.array_equal(b.getTransitionMatrix(3), sentinel[3])
    case.close()
    big = bm.beagle.Beagle(2, 3, 2, 65, 4, 1, 4, 1, 0)
    with pytest.raises(bm.beagle.BeagleException) as e:
        big.updateDifferentialMatrices(None, None, np.zeros((1, 65, 65)), None, [0], [0.1], 1, EXACT)
    assert e.value.code == -7
    big.finalize()
    basta = bm.beagle.Beagle(0, 6, 0, 4, 1, 2, 8, 1, 1, requirementFlags=bm.beagle.FLAG_EIGEN_COMPLEX)      # (as basta.py creates it)
    basta.setCategoryRates([1.0])
    basta.allocateCoalescentBuffers(5, 8, 6, 1)
    with pytest.raises(bm.beagle.BeagleException) as e:
        basta.updateDifferentialMatrices(None, None, np.zeros((1, 4, 4)), None, [0], [0.1], 1, EXACT)
    assert e.value.code == -7
    basta.finalize()
