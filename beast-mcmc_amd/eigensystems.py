"""The eigen systems of a set of substitution models: the caller's side of the reference's
SubstitutionModelDelegate.updateSubstitutionModels (treedatalikelihood/SubstitutionModelDelegate.java:272-288; one model:
HomogenousSubstitutionModelDelegate.java:228-240) over the ``beagle.Beagle`` method set.

The reference decomposes every changed model on the host (BaseSubstitutionModel.java:256-289) and hands ``(U, U^-1, lambda)`` to
``setEigenDecomposition``, one call per model, into an eigen buffer that is flipped first (BufferIndexHelper).  With branch-specific
models — a kappa or an omega per branch, epochs, a model per partition — that loop is the largest cost in front of an evaluation.
``route="host"`` is that sequence, with ``inputs.substmodel.decompose_reversible`` as the decomposition: the only route a library
without the extension offers (the CPU oracle).  ``route="device"`` hands the models' relative rates and frequencies over in one call
(``Beagle.setReversibleModels``, include/beagle_mi355.h beagleMi355SetReversibleModels) and the device decomposes them where the
eigen slots are.  A single model is one workgroup's work there; the host's LAPACK call wins that case (README), which is what the
host route stays for.
"""
import numpy as np

from . import beagle as _b
from .inputs import substmodel

SYMBOL = "beagleMi355SetReversibleModels"


class SubstitutionModelSet:
    """``count`` reversible models of ``state_count`` states as (relative rates [S (S - 1) / 2], upper triangle in row order;
    frequencies [S]) and a double-buffered eigen index per model: model k lives in eigen buffer k or count + k, flipped when it is
    updated, as BufferIndexHelper flips (BufferIndexHelper.java:65-85) — so an instance for it needs ``eigen_buffer_count`` buffers.
    ``library``: the EngineLibrary the instances will come from (default: the HIP engine); route "device" needs its extension."""

    def __init__(self, state_count, count, route="device", library=None):
        if route not in ("device", "host"):
            raise ValueError("route is 'device' or 'host'")
        self.lib = library or _b.engine()
        self._require(route, self.lib)
        self.S, self.count, self.route = int(state_count), int(count), route
        self.rates = np.zeros((self.count, self.S * (self.S - 1) // 2))
        self.freqs = np.full((self.count, self.S), 1.0 / self.S)
        self.offset = np.zeros(self.count, dtype=np.int32)
        self._stored_offset = self.offset.copy()
        self.dirty = np.ones(self.count, dtype=bool)

    @staticmethod
    def _require(route, lib):
        if route == "device" and not hasattr(lib.lib, SYMBOL):
            raise ValueError("this library decomposes no models: route='host'")

    @property
    def eigen_buffer_count(self):
        return 2 * self.count

    def eigen_indices(self):
        """The eigen buffer every model lives in now."""
        return (np.arange(self.count, dtype=np.int32) + self.offset * self.count).astype(np.int32)

    def set_model(self, k, relative_rates, frequencies):
        self.rates[k] = np.asarray(relative_rates, dtype=np.float64)
        self.freqs[k] = np.asarray(frequencies, dtype=np.float64)
        self.dirty[k] = True

    def set_hky(self, kappas, frequencies, which=None):
        """HKY with a kappa per model (HKY.java:157-230: kappa on AG and CT); ``which``: the models they go to (default: all)."""
        which = np.arange(self.count) if which is None else np.asarray(which)
        for k, kappa in zip(which, kappas):
            self.set_model(int(k), [1.0, kappa, 1.0, 1.0, kappa, 1.0], frequencies)

    def set_gy94(self, kappa, omegas, codon_frequencies=None, which=None):
        """GY94 over the 61 sense codons with an omega per model (inputs.substmodel.gy94_rates)."""
        pi = np.full(61, 1.0 / 61) if codon_frequencies is None else np.asarray(codon_frequencies, dtype=np.float64)
        which = np.arange(self.count) if which is None else np.asarray(which)
        synonymous, unit = np.asarray(substmodel.gy94_rates(kappa, 0.0)), np.asarray(substmodel.gy94_rates(kappa, 1.0))
        for k, omega in zip(which, omegas):                   # (the rates are affine in omega)
            self.set_model(int(k), synonymous + omega * (unit - synonymous), pi)

    def host_decomposition(self, k):
        """Model k as the host route decomposes it (Q as inputs.substmodel.reversible_q forms it, entry for entry)."""
        pi = self.freqs[k]
        r = np.zeros((self.S, self.S))
        r[np.triu_indices(self.S, 1)] = self.rates[k]
        q = (r + r.T) * pi[None, :]
        np.fill_diagonal(q, -q.sum(axis=1))
        return substmodel.decompose_reversible(q, pi)

    def store(self):
        self._stored_offset = self.offset.copy()

    def restore(self):
        """Back to the buffers of the last store(): a rejected move costs no decomposition."""
        self.offset = self._stored_offset.copy()

    def update(self, beagle, route=None, flip=True):
        """Every changed model into its (flipped) eigen buffer of ``beagle``, by ``route`` (default: the set's).  -> the models
        that were updated."""
        route = self.route if route is None else route
        if route not in ("device", "host"):
            raise ValueError("route is 'device' or 'host'")
        self._require(route, beagle.lib)
        which = np.flatnonzero(self.dirty)
        if which.size == 0:
            return which
        if flip:
            self.offset[which] ^= 1
        idx = self.eigen_indices()[which]
        if route == "device":
            beagle.setReversibleModels(idx, self.rates[which], self.freqs[which])
        else:
            for k, slot in zip(which, idx):
                e = self.host_decomposition(int(k))
                beagle.setEigenDecomposition(int(slot), e.evec, e.ievc, e.evals)
        self.dirty[:] = False
        return which
