"""Tip error models as emission tables (beast_mcmc_amd.tipmodels, include/beagle_mi355.h beagleMi355SetTipEmission), the tier that
needs no GPU: the tables state exactly what the reference's two models write, and a tip with a table is a compact tip whose branch matrix
is M E^T — the identity the device's fold rests on, checked between the CPU oracle (given the expanded partials) and a numpy pruning over
compact codes with host-folded matrices."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import beast_mcmc_amd as bm
import helpers
import tip_emission_cases as cases
import tip_models_reference as ref
from beast_mcmc_amd import tipmodels
from beast_mcmc_amd.treelikelihood import BeagleTreeLikelihood, RESCALE_NONE

_DP = C.POINTER(C.c_double)
ALIGNMENT_STATES = np.array([0, 1, 2, 3, 5, 4, 6, 15, 16, 17, -1] * 3, dtype=np.int32)     # every nucleotide, the context A, ambiguities, gaps


def test_library_exports_and_header_declares_the_calls(engine_lib):
    hdr = open(os.path.join(helpers.ROOT, "include", "beagle_mi355.h")).read()
    for name in ("beagleMi355SetTipEmission", "beagleMi355TipEmissionStats"):
        assert hasattr(engine_lib.lib, name)
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr)
        assert name in bm.beagle.ABI_SYMBOLS
    assert hasattr(bm.beagle.Beagle, "setTipEmission") and hasattr(bm.beagle.Beagle, "tipEmissionStats")


@pytest.mark.parametrize("error_type", ["all", "transitions"])
@pytest.mark.parametrize("base_rate,age_rate", [(0.013, None), (None, 0.4), (0.02, 0.25), (None, None)])
@pytest.mark.parametrize("has_indicator,indicator,excluded", [(False, 1.0, False), (True, 1.0, False), (True, 0.0, False), (False, 1.0, True),
                                                             (True, 0.0, True)])
def test_sequence_error_tables_expand_to_the_reference_partials(error_type, base_rate, age_rate, has_indicator, indicator, excluded):
    states = ALIGNMENT_STATES
    expect = ref.sequence_error_partials(states, error_type, base_rate, age_rate, 1.7, has_indicator, indicator, excluded)
    e = tipmodels.sequence_error_emission(error_type, base_rate, age_rate, 1.7, indicator_on=(not has_indicator) or indicator > 0.0,
                                          excluded=excluded)
    assert e.shape == (4, 4)
    codes = np.where((states >= 0) & (states < 4), states, -1)
    assert np.array_equal(tipmodels.expand(codes, e), expect)
    if (has_indicator and indicator <= 0.0) or excluded:
        assert np.array_equal(e, np.eye(4))


@pytest.mark.parametrize("rate,hyper", [(0.0, True), (0.31, True), (0.31, False), (1.0, True)])
def test_hypermutant_table_expands_to_the_reference_partials(rate, hyper):
    expect = ref.hypermutant_partials(ALIGNMENT_STATES, rate, hyper)
    e = tipmodels.hypermutant_emission(rate, hyper)
    assert e.shape == (5, 4)
    assert np.array_equal(tipmodels.expand(tipmodels.hypermutant_codes(ALIGNMENT_STATES), e), expect)


def test_ambiguity_table():
    e = tipmodels.ambiguity_emission([(0,), (1,), (2,), (3,), (0, 2), (1, 3), (0, 1, 2, 3)], 4)
    assert np.array_equal(tipmodels.expand([4, 6, 0, 9], e), [[1, 0, 1, 0], [1, 1, 1, 1], [1, 0, 0, 0], [1, 1, 1, 1]])


def test_fold_adds_the_products_in_ascending_order_without_fusing():
    rng = np.random.default_rng(2)
    m, e = rng.uniform(size=(2, 5, 5)), rng.uniform(size=(3, 5))
    f = tipmodels.fold(m, e)
    for c in range(2):
        for i in range(5):
            for k in range(5):
                acc = 0.0
                for j in range(5):
                    acc = acc + (m[c, i, j] * e[k, j] if k < 3 else 0.0)      # columns behind the table's are zero
                assert f[c, i, k] == acc


@pytest.mark.parametrize("shape", cases.SHAPES)
def test_oracle_on_expanded_partials_equals_pruning_over_codes_with_folded_matrices(shape, oracle_lib):
    """lnL(oracle; setTipPartials(expand(codes, E_t))) = lnL(numpy pruning; compact codes, tip matrices M_t E_t^T) to 1e-12 relative."""
    wl, codes, _ = cases.workload(shape)
    S, T = shape[0], shape[1]
    tabs = cases.tables(shape, 0.02)
    o = BeagleTreeLikelihood(wl, library=oracle_lib, rescaling=RESCALE_NONE)
    for t in range(T):
        p = np.ascontiguousarray(tipmodels.expand(codes[t], tabs[t]))
        assert o.h.btlSetTipPartials(o.ptr, t, p.ctypes.data_as(_DP)) == 0
    o.makeDirty()
    lnl = o.getLogLikelihood()
    sites = o.getSiteLogLikelihoods()
    o.close()
    mats = cases.transition_matrices(wl)
    for t in range(T):
        mats[t] = tipmodels.fold(mats[t], tabs[t])
    got, got_sites = ref.prune(wl.tree, codes, mats, wl.freqs, wl.cat_weights, wl.weights)
    assert helpers.rel_err(got, lnl) <= 1e-12, (got, lnl)
    assert np.max(np.abs(got_sites - sites) / np.abs(sites)) <= 1e-12
