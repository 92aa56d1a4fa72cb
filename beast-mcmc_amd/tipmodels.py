"""Tip error models as emission tables: the caller side of ``beagleMi355SetTipEmission`` (include/beagle_mi355.h).

The reference's ``TipStatesModel`` implementations (src/dr/evomodel/tipstatesmodel/SequenceErrorModel.java,
HypermutantErrorModel.java) write a tip's partials pattern by pattern on the host and the tree likelihood re-sends them with
``setTipPartials`` for every tip whose ``updateNode`` is set (BeagleTreeLikelihood.java:917-930).  What they write is a lookup: the
vector of a pattern is one of a handful of columns chosen by the observed code.  This module states those columns as a table
``E[k][i] = P(observed code k | true state i)``; the engine then needs the codes once and K * S doubles per parameter change.
"""
import numpy as np

ALL_SUBSTITUTIONS, TRANSITIONS_ONLY = "all", "transitions"
# the code a hypermutation-context A is observed as (Nucleotides.R_STATE in the reference's alignment coding) and its row of the table
HYPERMUTANT_CONTEXT_STATE, HYPERMUTANT_CONTEXT_CODE = 5, 4
_TRANSITION_OF = (2, 3, 0, 1)        # A <-> G, C <-> T


def sequence_error_emission(error_type, base_rate=None, age_rate=None, tip_age=0.0, indicator_on=True, excluded=False):
    """E [4][4] of SequenceErrorModel.getTipPartials (:126-155): row k is what an observed nucleotide k contributes.  ``base_rate`` /
    ``age_rate`` None: the model has no such parameter.  Indicator off, or an excluded taxon: the identity table."""
    if error_type not in (ALL_SUBSTITUTIONS, TRANSITIONS_ONLY):
        raise ValueError("only TRANSITIONS_ONLY and ALL_SUBSTITUTIONS are supported")
    p_undamaged, p_ts, p_tv = 1.0, 0.0, 0.0
    if indicator_on and not excluded:
        if base_rate is not None:
            p_undamaged = p_undamaged - float(base_rate)
        if age_rate is not None:
            p_undamaged *= np.exp(-float(age_rate) * float(tip_age))
        if error_type == ALL_SUBSTITUTIONS:
            p_ts = (1.0 - p_undamaged) / 3.0
            p_tv = p_ts
        else:
            p_ts = 1.0 - p_undamaged
            p_tv = 0.0
    e = np.full((4, 4), float(p_tv))
    for k in range(4):
        e[k, _TRANSITION_OF[k]] = p_ts
        e[k, k] = p_undamaged
    return e


def hypermutant_emission(rate, is_hypermutated):
    """E [5][4] of HypermutantErrorModel.getTipPartials: the four nucleotides as themselves, and code 4 — an A in a hypermutation
    context — as A or, in a hypermutated sequence, a mutated G with probability ``rate``."""
    e = np.zeros((5, 4))
    e[:4] = np.eye(4)
    e[4] = (1.0 - float(rate), 0.0, float(rate), 0.0) if is_hypermutated else (1.0, 0.0, 0.0, 0.0)
    return e


def hypermutant_codes(states):
    """Alignment states (0..3 nucleotides, 5 the context A, anything else an ambiguity) -> codes of ``hypermutant_emission``."""
    s = np.asarray(states)
    return np.where((s >= 0) & (s < 4), s, np.where(s == HYPERMUTANT_CONTEXT_STATE, HYPERMUTANT_CONTEXT_CODE, -1)).astype(np.int32)


def ambiguity_emission(state_sets, state_count):
    """The 0/1 table of a ``useAmbiguities`` run: row k is one for the states code k may stand for."""
    e = np.zeros((len(state_sets), state_count))
    for k, members in enumerate(state_sets):
        e[k, list(members)] = 1.0
    return e


def expand(codes, emission):
    """The tip's partials [P][S] — what ``setTipPartials`` would be given: ``emission[code]``, all ones for a code outside the table."""
    e = np.asarray(emission, dtype=np.float64)
    c = np.asarray(codes)
    known = (c >= 0) & (c < e.shape[0])
    out = np.ones((c.shape[0], e.shape[1]))
    out[known] = e[c[known]]
    return out


def fold(matrix, emission):
    """[C][S][S] branch matrices of a folded tip, M E^T with zero columns behind the table's — the host statement of the device's
    fold, in its order: the products added with j ascending and never fused."""
    m = np.asarray(matrix, dtype=np.float64)
    e = np.asarray(emission, dtype=np.float64)
    S = m.shape[-1]
    out = np.zeros_like(m)
    for k in range(e.shape[0]):
        acc = np.zeros(m.shape[:-1])
        for j in range(S):
            acc = acc + m[..., j] * e[k, j]
        out[..., k] = acc
    return out


class TipErrorModel:
    """A sequence-error model bound to a BeagleTreeLikelihood: the codes go to the engine once; a parameter change sends the tables of
    the affected tips only and marks those tips for update — the protocol of BeagleTreeLikelihood.java:917-930 with K * S doubles a
    tip instead of P * S."""

    def __init__(self, tl, codes, error_type=ALL_SUBSTITUTIONS, base_rate=None, age_rate=None, tip_ages=None, indicators=None,
                 excluded=None):
        from . import beagle as _b
        self.tl = tl
        self.raw = _b.Beagle.attach(tl)
        self.error_type = error_type
        self.base_rate, self.age_rate = base_rate, age_rate
        n = tl.tip_count
        self.tip_ages = np.zeros(n) if tip_ages is None else np.asarray(tip_ages, dtype=np.float64).copy()
        self.indicators = np.ones(n, dtype=bool) if indicators is None else np.asarray(indicators, dtype=bool).copy()
        self.excluded = np.zeros(n, dtype=bool) if excluded is None else np.asarray(excluded, dtype=bool).copy()
        self.codes = np.asarray(codes)
        for t in range(n):
            self.raw.setTipEmission(t, self.codes[t], self.table(t))
        tl.makeDirty()

    def table(self, tip):
        return sequence_error_emission(self.error_type, self.base_rate, self.age_rate, self.tip_ages[tip], bool(self.indicators[tip]),
                                       bool(self.excluded[tip]))

    def partials(self, tip):
        return expand(self.codes[tip], self.table(tip))

    def _send(self, tips):
        for t in tips:
            self.raw.setTipEmission(int(t), None, self.table(int(t)))
            # updateNode[tip]: its branch and the nodes above it are evaluated again (the height itself does not change)
            self.tl.set_node_height(int(t), self.tl.node_height(int(t)))

    def set_rates(self, base_rate=None, age_rate=None):
        """A move of the base or the age-related error rate: every taxon's table changes."""
        if base_rate is not None:
            self.base_rate = base_rate
        if age_rate is not None:
            self.age_rate = age_rate
        self._send(range(self.tl.tip_count))

    def set_indicator(self, tip, on):
        self.indicators[tip] = bool(on)
        self._send([tip])
