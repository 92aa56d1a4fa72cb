"""Branch matrices of models that have no usable eigen system: the caller's side of the reference's
SubstitutionModelDelegate.updateSubstitutionModels + updateTransitionMatrices (treedatalikelihood/SubstitutionModelDelegate.java
:213-288) for ComplexSubstitutionModel, BSSVS / GLM rate matrices and migration matrices, over the ``beagle.Beagle`` method set.

The reference decomposes every changed generator on the host (ComplexSubstitutionModel.java:121-173), uploads the eigen system with
``setEigenDecomposition`` and asks for U exp(Lambda d) U^-1.  For a sparse or defective generator that product cancels — negative
"probabilities", or nothing usable at all (tests/test_generator_matrices_host.py).  ``route="host"`` is that sequence, with
``inputs.substmodel.decompose_complex`` as the decomposition: the only route a library without the extension offers (the CPU
oracle); it needs an EIGEN_COMPLEX instance with ``eigen_buffer_count`` eigen buffers.  ``route="device"`` hands the generators
over in one call (``Beagle.updateTransitionMatricesFromGenerators``, include/beagle_mi355.h
beagleMi355UpdateTransitionMatricesFromGenerators) and the device forms exp(Q d) by uniformization with scaling and squaring: no
eigen system, no negative entry, the same on a defective generator as anywhere else.
"""
import numpy as np

from . import beagle as _b
from .inputs import substmodel

SYMBOL = "beagleMi355UpdateTransitionMatricesFromGenerators"


def normalised(q):
    """q scaled to one expected substitution per unit time at its stationary distribution — what getInfinitesimalMatrix returns and
    what ``decompose_complex`` decomposes."""
    q = np.asarray(q, dtype=np.float64)
    pi = substmodel.stationary_distribution(q)
    return q / float(-(np.diag(q) * pi).sum())


class GeneratorModelSet:
    """``count`` generators of ``state_count`` states, [count][S][S], as getInfinitesimalMatrix returns them (already normalised).
    ``library``: the EngineLibrary the instances will come from (default: the HIP engine); route "device" needs its extension."""

    def __init__(self, state_count, count=1, route="device", library=None):
        if route not in ("device", "host"):
            raise ValueError("route is 'device' or 'host'")
        self.lib = library or _b.engine()
        self._require(route, self.lib)
        self.S, self.count, self.route = int(state_count), int(count), route
        self.generators = np.zeros((self.count, self.S, self.S))

    @staticmethod
    def _require(route, lib):
        if route == "device" and not hasattr(lib.lib, SYMBOL):
            raise ValueError("this library forms no matrices from generators: route='host'")

    @property
    def eigen_buffer_count(self):
        """Eigen buffers the host route needs (the device route needs none of its own)."""
        return self.count

    def set_generator(self, k, q):
        q = np.asarray(q, dtype=np.float64)
        if q.shape != (self.S, self.S):
            raise ValueError("a generator is [S][S]")
        self.generators[k] = q

    def host_decomposition(self, k):
        """Generator k as the host route decomposes it."""
        return substmodel.decompose_complex(self.generators[k])[1]

    def update_matrices(self, beagle, probability_indices, edge_lengths, generator_indices=None, category_rate_indices=None, route=None):
        """The matrices of the listed branches into their slots of ``beagle``, by ``route`` (default: the set's)."""
        route = self.route if route is None else route
        if route not in ("device", "host"):
            raise ValueError("route is 'device' or 'host'")
        self._require(route, beagle.lib)
        m = np.asarray(probability_indices, dtype=np.int32).reshape(-1)
        t = np.asarray(edge_lengths, dtype=np.float64).reshape(-1)
        g = np.zeros(m.size, dtype=np.int32) if generator_indices is None else np.asarray(generator_indices, dtype=np.int32).reshape(-1)
        r = np.zeros(m.size, dtype=np.int32) if category_rate_indices is None else np.asarray(category_rate_indices, dtype=np.int32).reshape(-1)
        if not (t.size == g.size == r.size == m.size):
            raise ValueError("one length, generator and rate set per matrix")
        if m.size == 0:
            return
        if route == "device":
            beagle.updateTransitionMatricesFromGenerators(self.generators, None if generator_indices is None else g,
                                                          None if category_rate_indices is None else r, m, t)
            return
        for k in np.unique(g):
            e = self.host_decomposition(int(k))
            beagle.setEigenDecomposition(int(k), e.evec, e.ievc, e.evals)
        if self.count == 1 and category_rate_indices is None:
            beagle.updateTransitionMatrices(0, m, None, None, t, m.size)
        else:
            beagle.updateTransitionMatricesWithMultipleModels(g, r, m, None, None, t, m.size)
