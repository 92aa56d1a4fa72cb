"""Seeded random call sequences over the single-partition ``beagle.Beagle`` method set, to be run on the engine and the CPU oracle in
lockstep (tests/test_gpu_call_sequences.py) or on the oracle alone (tests/test_call_sequences_host.py).

The generator is plain Python and numpy: it loads neither library (the extension profile takes the threshold guard of its differential
matrices from tests/differential_matrices_reference.py).  ``generate(shape, seed, length, profile)`` returns call records

    {"m": method of beagle.Beagle, "a": [arguments as plain lists / numbers], "action": name in ACTIONS (+ ACTIONS_EXT), "motif": letter
     or None, "variant": variant of a motif that has variants, or None}

which survive a JSON round trip unchanged (``dump`` / ``load``; a profile other than "base" travels in the file).  ``execute(b,
record, side)`` makes one call on a binding object and returns (return code, reads), a read being (kind, array); ``deviation(kind,
got, want)`` is the normalised error of a read, so that one bound (1e-10) holds for every kind.

Three profiles ("extensions" and "queries" are described below and behind it).  "base" (the default) is the method set of ACTIONS with motifs (a)-(i); its sequences are pinned record for record by
tests/golden/call_sequence_digests.json.  "extensions" (shapes of at most 64 states) adds ACTIONS_EXT — the one-call entry points
sampleAncestralStates, sampleMarkovJumps, simulateSequences, nodeHeightDerivatives, updateDifferentialMatrices, setReversibleModels
and getEigenDecomposition, each of which decides for itself what happens to the deferred state (whether a held pre-order list runs,
whether unstored nodes are materialised, whether a folded tip is demoted, whether an upload shadow is cleared) — and motifs
  (j) a held whole-tree pre-order list, one of five of those calls, the edge derivatives' sums;
  (k) setReversibleModels(slot), every branch matrix from that slot, partials, a root call, Markov jumps on that slot (variant
      "reupload": the slot's previous values uploaded behind the device's write — an upload that must not be skipped);
  (l) a sampler right behind a whole-tree list with flipped buffers and no root call (variants with setTipEmission on a tip first);
  (m) a differential matrix written by the device over a branch matrix that the held list reads, the matrix put back, the child's
      pre-order partial read.
The oracle has none of these calls: ``execute_extension`` makes them from its own calls and the numpy restatements that the
extensions' own tests use.  New kinds of read: "states" / "cats" (a draw: equal on every decided pattern — ancestral_reference
.near_a_boundary — with at most UNDECIDED_CAP of a sequence's (sampler call, pattern) pairs undecided), "exact" (the device's draw
against the restatement over what the SAME instance reads back after the call: byte for byte), "jumps" (Markov-jump values, restated
for the device's own states), "eigen" (an eigen system through what it reconstructs); node-height derivatives are "deriv".  The
generator also tracks, for these calls, which (eigen slot, rate slot, length) every branch matrix was built from and whether that
slot has changed since (sampleMarkovJumps is emitted over matrices of one unchanged pair only), and what kind of matrix a
differential slot holds (nodeHeightDerivatives wants Q x category rate).

"queries" (shapes of at most 64 states; its sequences leave those of the other two profiles record for record what they were:
tests/golden/call_sequence_digests_extensions.json pins the second profile's) is ACTIONS plus setReversibleModels plus ACTIONS_Q — the
five entry points merged after the second profile was written: updateTransitionMatricesFromGenerators,
updateTransitionMatricesWithEpochs, nodePosteriors, nodePatternLikelihoods, placementScores — with motifs (a)-(i) and
  (n) nodePosteriors over every internal node behind a held whole-tree pre-order list, the edge derivatives' sums (variants: the
      post-order buffers freshly flipped with no root call; setPartials into a listed pre-order buffer between list and call);
  (o) nodePatternLikelihoods over the whole tree behind that list, which does not write its buffers, the edge sums (variants "plain",
      "raw" and "log" scale buffers, "emission": a folded tip demoted under the list);
  (p) a branch matrix that the held list reads rewritten by the generator call or the epoch call (variants "_spare": a spare slot,
      the list stays held), the edge sums, the child's pre-order partial, the matrix put back;
  (q) placementScores right behind a whole-tree list with flipped buffers and no root call (variant with setTipEmission first, the
      tip a candidate's child), then a root call;
  (r) setReversibleModels(slot), every branch matrix by an epoch call over both slots, partials, a root call (variant "reupload").
The oracle's side of the two matrix calls is generator_matrices_reference.yardstick / epoch_matrices_reference.yardstick rounded to
double, then setTransitionMatrix (an epoch entry of ONE segment: the oracle's own updateTransitionMatricesWithMultipleModels; every
sequence has one); of the three that return values, node_posteriors_reference, stochastic_dollo_reference and placement_reference over
the oracle's getPartials, getLogScaleFactors and getTransitionMatrix and the compact states it was sent.  Kinds of read: "posterior"
(posteriors, category posteriors, MAP probabilities, state totals over the sum of the pattern weights: absolute difference), "logval"
(log pattern values, node terms, log tables, scores: against max(1, |value|)), the sum of a node-pattern call as "sum", MAP states as
"states" (undecided where the oracle side's two largest posteriors lie within MAP_MARGIN), node terms' -inf entries as a "states"
mask, and "exact" for the device's posteriors against node_posteriors_reference.posteriors over the same instance's read-back.
nodePatternLikelihoods takes its death state from the compact tip states the generator itself sent, so that every pattern has a tip
outside it (where no state does — a subtree over one compact tip — the whole tree is taken; the action is given up if that fails too).

Instance layout for T tips, N = 2T - 1 nodes (``Layout``): internal node n lives in partials buffer T + j (T - 1) + (n - T) of set j
(j flips per node each time the node is written, as BufferIndexHelper does), its pre-order partials in T + 2 (T - 1) + n; the branch
matrix of node n in slot j N + n, four spare slots behind them (two for products / sums / transposes / detached updates, two for
differential matrices); scale buffer j (T - 1) + (n - T) per internal node and set, two cumulative ones behind them; two eigen /
weight / frequency / category-rate slots; T compact buffers.

The definedness model: the generator tracks which partials buffers, matrices and scale buffers hold a defined value (a scale buffer
also whether it holds the factors of a rescaling operation, "raw", or accumulated logarithms, "log": a read-mode operation divides
by raw factors only, accumulate / remove add into log buffers only), and which scale buffer each partials buffer was last written
with.  Reads and consuming calls are emitted on defined inputs only, and never what the contract leaves open: an operation writing one
of its own children, convolve / transpose onto an input, accumulate of a never-written buffer, a root call with count != 1, derivative
indices to updateTransitionMatrices.  Branch matrices are non-negative whenever something consumes them (differential matrices stay
in their two spare slots, but for motif (m), which puts the branch's matrix back before any consumer).

Replay of a failing sequence:  python tests/call_sequences.py --replay FILE --upto N  runs engine and oracle up to step N and prints
the first diverging read; it stops at the first non-zero return code or exception.
"""
import json
import types

import numpy as np

NONE = -1
BOUND = 1e-10

ACTIONS = (
    "setEigenDecomposition", "setCategoryRates", "setCategoryRatesWithIndex", "setCategoryWeights", "setStateFrequencies",
    "setPatternWeights",
    "setTipStates", "setTipPartials", "setPartials", "compactToPartials", "setTipEmission",
    "updateTransitionMatrices", "updateTransitionMatricesWithMultipleModels", "setTransitionMatrix", "convolveTransitionMatrices",
    "addTransitionMatrices", "transposeTransitionMatrices", "getTransitionMatrix",
    "updatePartials:none", "updatePartials:write", "updatePartials:read", "updatePartials:cumulative", "waitForPartials",
    "resetScaleFactors", "accumulateScaleFactors", "removeScaleFactors", "copyScaleFactors", "getLogScaleFactors",
    "calculateRootLogLikelihoods:root", "calculateRootLogLikelihoods:other", "calculateRootLogLikelihoods:cumulative",
    "getSiteLogLikelihoods", "getPartials", "getPartials:scaled", "getPartialsBatch",
    "setRootPrePartials", "updatePrePartials", "setDifferentialMatrix", "calculateEdgeDifferentials",
    "calculateCrossProductDifferentials", "getPartials:pre",
)
# profile "extensions": the one-call entry points of include/beagle_mi355.h that sit on top of the deferral logic
ACTIONS_EXT = ("sampleAncestralStates", "sampleMarkovJumps", "simulateSequences", "nodeHeightDerivatives", "updateDifferentialMatrices",
               "setReversibleModels", "getEigenDecomposition")
# profile "queries": the five one-call entry points merged after that profile was written (setReversibleModels rides along, so that
# eigen slots the device wrote are in play for the epoch call)
ACTIONS_Q = ("updateTransitionMatricesFromGenerators", "updateTransitionMatricesWithEpochs", "nodePosteriors", "nodePatternLikelihoods",
             "placementScores")
PROFILES = ("base", "extensions", "queries")
EXT_MAX_STATES = 64                        # several of them answer NO_IMPLEMENTATION above 64 states
EMISSION_STATES = (4, 20)                  # setTipEmission: 4- and 20-state shapes only
MOTIFS = "abcdefghi"
MOTIFS_EXT = "jklm"
MOTIFS_Q = "nopqr"
N_VARIANTS = ("flipped", "set_pre")
O_VARIANTS = ("plain", "raw", "log", "emission")
P_VARIANTS = ("generators", "epochs", "generators_spare", "epochs_spare")
Q_VARIANTS = ("plain", "emission")
R_VARIANTS = ("plain", "reupload")
MISSING_CODE = 255                         # placementScores: a query's code at a site it does not cover
MAP_MARGIN = 1e-8                          # nodePosteriors: a pattern is undecided where the two largest posteriors lie this close
J_VARIANTS = ("updateDifferentialMatrices", "setReversibleModels", "nodeHeightDerivatives", "sampleAncestralStates", "simulateSequences")
K_VARIANTS = ("plain", "reupload")
L_VARIANTS = ("ancestral", "jumps", "emission_ancestral", "emission_jumps")
SITE_COUNTS = (1, 5, 130, 259)             # simulateSequences: across the four-sites-per-thread word and a workgroup
JUMPS_REWARDS, JUMPS_SCALE_BY_TIME = 1, 2
UNDECIDED_CAP = 0.01                       # of a sequence's (sampler call, pattern) pairs
D_VARIANTS = ("getPartials", "getPartialsBatch", "getSiteLogLikelihoods", "getLogScaleFactors", "resetScaleFactors", "copyScaleFactors",
              "setTransitionMatrix", "setCategoryWeights")
F_VARIANTS = ("read_pre", "read_post", "write_post", "write_matrix", "write_pre", "scale_call", "model_call", "root_call")
QUERY_FILL = 40                            # drawn calls between the motifs of a query sequence, at the least
HOST_COPY_MAX = 12                         # uploads one launch carries (motif c queues more)


def actions_for(S, profile="base"):
    base = tuple(a for a in ACTIONS if a != "setTipEmission" or S in EMISSION_STATES)
    if profile == "queries":
        return base + ("setReversibleModels",) + ACTIONS_Q
    return base + ACTIONS_EXT if profile == "extensions" else base


def motifs_for(profile="base"):
    if profile == "queries":
        return MOTIFS + MOTIFS_Q
    return MOTIFS + MOTIFS_EXT if profile == "extensions" else MOTIFS


def o_variants(S):
    return O_VARIANTS if S in EMISSION_STATES else O_VARIANTS[:3]


def q_variants(S):
    return Q_VARIANTS if S in EMISSION_STATES else Q_VARIANTS[:1]


def variants_for(S, profile="base"):
    """every (motif, variant) that a 4-state shape's seeds hold together: of motifs (d) and (f) over the base profile's 8 seeds, of (j),
    (k) and (l) over the extension profile's 4 (of (l), the two emission variants exist at 4 and 20 states), of (n)-(r) over the
    query profile's 4 (the emission variants of (o) and (q) likewise)"""
    if profile == "queries":
        return (set(("n", v) for v in N_VARIANTS) | set(("o", v) for v in o_variants(S)) | set(("p", v) for v in P_VARIANTS)
                | set(("q", v) for v in q_variants(S)) | set(("r", v) for v in R_VARIANTS))
    if profile != "extensions":
        return set(("d", v) for v in D_VARIANTS) | set(("f", v) for v in F_VARIANTS)
    out = set(("j", v) for v in J_VARIANTS) | set(("k", v) for v in K_VARIANTS)
    return out | set(("l", v) for v in (L_VARIANTS if S in EMISSION_STATES else L_VARIANTS[:2]))


class Layout:
    def __init__(self, shape):
        self.S, self.C, self.T, self.P = shape
        T = self.T
        self.N = 2 * T - 1
        self.root = self.N - 1
        self.pre_base = T + 2 * (T - 1)
        self.partials_count = self.pre_base + self.N
        self.matrix_count = 2 * self.N + 4
        self.spare = [2 * self.N + k for k in range(4)]        # [0], [1]: probabilities; [2], [3]: differential matrices
        self.cum = [2 * (T - 1), 2 * (T - 1) + 1]
        self.scale_count = 2 * (T - 1) + 2
        self.eigen_count = 2

    def post(self, n, j):
        return n if n < self.T else self.T + j * (self.T - 1) + (n - self.T)

    def pre(self, n):
        return self.pre_base + n

    def matrix(self, n, j):
        return j * self.N + n

    def scale(self, n, j):
        return j * (self.T - 1) + (n - self.T)

    def create_args(self):
        return (self.T, self.partials_count, self.T, self.S, self.P, self.eigen_count, self.matrix_count, self.C, self.scale_count)


def _lst(a):
    return np.asarray(a).tolist()


def reversible_model(rng, S):
    """(eigenvectors, inverse, eigenvalues, frequencies, Q) of a random reversible model at one substitution per unit time, from the
    symmetric form D^1/2 Q D^-1/2"""
    pi = rng.dirichlet(np.full(S, 20.0))
    r = rng.uniform(0.5, 1.5, size=(S, S))
    r = np.triu(r, 1)
    r = r + r.T
    return decompose_reversible(r, pi)


def decompose_reversible(r, pi):
    """the same from symmetric exchange rates r [S][S] and frequencies: numpy's eigh of the symmetric form"""
    q = r * pi[None, :]
    q -= np.diag(q.sum(axis=1))
    q /= -np.dot(pi, np.diag(q))
    d = np.sqrt(pi)
    lam, v = np.linalg.eigh(d[:, None] * q / d[None, :])
    return v / d[:, None], v.T * d[None, :], lam, pi, q


def symmetric_rates(upper, S):
    """the upper triangle in row order (what setReversibleModels takes) -> symmetric [S][S], zero diagonal"""
    r = np.zeros((S, S))
    r[np.triu_indices(S, 1)] = np.asarray(upper, dtype=float)
    return r + r.T


class Generator:
    def __init__(self, shape, seed, length, profile="base"):
        if profile not in PROFILES or (profile != "base" and shape[0] > EXT_MAX_STATES):
            raise ValueError("profile %r at %d states" % (profile, shape[0]))
        self.profile = profile
        self.L = L = Layout(shape)
        self.shape, self.seed, self.length = tuple(shape), seed, length
        self.rng = np.random.default_rng([seed, L.S, L.C, L.T, L.P])
        self.rec = []
        self.motif = self.variant = None
        T, N = L.T, L.N
        rng = self.rng
        # the tree: nodes joined pairwise, children before parents, the root last
        self.left, self.right, self.parent = [NONE] * N, [NONE] * N, [NONE] * N
        live = list(range(T))
        for n in range(T, N):
            a = live.pop(int(rng.integers(len(live))))
            b = live.pop(int(rng.integers(len(live))))
            self.left[n], self.right[n], self.parent[a], self.parent[b] = a, b, n, n
            live.append(n)
        self.level = [0] * N
        for n in range(T, N):
            self.level[n] = 1 + max(self.level[self.left[n]], self.level[self.right[n]])
        self.internal = list(range(T, N))
        self.length_of = rng.uniform(0.01, 1.0, size=N)
        # model state
        self.cur = [0] * N                      # buffer set holding node n's current partials
        self.mcur = [0] * N                     # matrix set holding node n's current branch matrix
        self.pdef = [False] * L.partials_count
        self.pscale = [NONE] * L.partials_count
        self.mdef = [None] * L.matrix_count     # None, "prob" or "diff"
        self.sdef = [None] * L.scale_count      # None, "raw" or "log"
        self.accumulated = {c: [] for c in L.cum}
        self.tipkind = ["compact" if rng.random() < 2.0 / 3.0 else "partials" for _ in range(T)]
        if "compact" not in self.tipkind:
            self.tipkind[0] = "compact"
        if "partials" not in self.tipkind:
            self.tipkind[T - 1] = "partials"
        self.models = [None, None]
        self.rates = [None, None]
        self.root_done = False
        self.last_list = None
        self.last_pre = None
        self.d_count = self.f_count = 0
        # what the extension actions need to know (no random number is drawn for it: the base profile's records do not depend on it)
        self.eigen_version = [0, 0]             # bumped whenever an eigen slot's content may have changed
        self.rates_version = [0, 0]
        self.mfrom = [None] * L.matrix_count    # (eigen slot, its version, rate slot, its version, length) a probability matrix was built from
        self.dkind = {}                         # differential slot -> "Qrate" (Q x category rate), "QQ" or "D" (written by the device)
        # what the query actions need to know (likewise: nothing is drawn for it, and no record of the other two profiles reads it)
        self.tip_sent = {}                      # compact tip -> the states last sent to it
        self.weights_set = False                # setPatternWeights has been called (nodePosteriors' totals)
        self.single_epoch = False               # an epoch entry with one segment has been emitted

    # ---- records ---------------------------------------------------------------------------------------------------------------
    def emit(self, method, args, action):
        self.rec.append({"m": method, "a": args, "action": action, "motif": self.motif, "variant": self.variant})

    # ---- values ------------------------------------------------------------------------------------------------------------------
    def tip_states(self, first_known=False):
        L, rng = self.L, self.rng
        s = rng.integers(0, L.S, size=L.P)
        if not first_known:
            s[rng.random(L.P) < 0.025] = L.S
        return _lst(s)

    def tip_partials(self):
        L, rng = self.L, self.rng
        p = rng.uniform(0.02, 0.1, size=(L.P, L.S))
        p[np.arange(L.P), rng.integers(0, L.S, size=L.P)] = 1.0
        return _lst(p.ravel())

    def node_partials(self):
        L = self.L
        return _lst(self.rng.uniform(0.1, 1.0, size=L.C * L.P * L.S))

    def weights(self):
        return _lst(self.rng.dirichlet(np.full(self.L.C, 5.0)))

    def category_rates(self):
        r = self.rng.uniform(0.3, 2.0, size=self.L.C)
        return _lst(r / r.mean())

    def random_matrix(self):
        L = self.L
        m = self.rng.dirichlet(np.full(L.S, 1.0), size=L.C * L.S)
        return _lst(m.ravel())

    def a_length(self):
        return float(self.rng.uniform(0.01, 1.0))

    # ---- model calls ---------------------------------------------------------------------------------------------------------
    def set_eigen(self, slot, same=False):
        if not same or self.models[slot] is None:
            self.models[slot] = reversible_model(self.rng, self.L.S)
        u, ui, lam, _, _ = self.models[slot]
        self.eigen_version[slot] += 1
        self.emit("setEigenDecomposition", [slot, _lst(u.ravel()), _lst(ui.ravel()), _lst(lam)], "setEigenDecomposition")

    def set_rates(self, slot, indexed):
        self.rates[slot] = self.category_rates()
        self.rates_version[slot] += 1
        if indexed or slot != 0:
            self.emit("setCategoryRatesWithIndex", [slot, self.rates[slot]], "setCategoryRatesWithIndex")
        else:
            self.emit("setCategoryRates", [self.rates[0]], "setCategoryRates")

    def set_weights(self, slot):
        self.emit("setCategoryWeights", [slot, self.weights()], "setCategoryWeights")

    def set_frequencies(self, slot):
        self.emit("setStateFrequencies", [slot, _lst(self.rng.dirichlet(np.full(self.L.S, 20.0)))], "setStateFrequencies")

    def set_pattern_weights(self):
        self.emit("setPatternWeights", [_lst(self.rng.integers(1, 9, size=self.L.P).astype(float))], "setPatternWeights")
        self.weights_set = True

    # ---- data calls ------------------------------------------------------------------------------------------------------------
    def resend_tip(self, t=None):
        t = int(self.rng.integers(self.L.T)) if t is None else t
        if self.tipkind[t] == "compact":
            self.tip_sent[t] = self.tip_states(first_known=(t == self.first_compact))
            self.emit("setTipStates", [t, self.tip_sent[t]], "setTipStates")
        else:
            self.emit("setTipPartials", [t, self.tip_partials()], "setTipPartials")
            self.tipkind[t] = "partials"
        self.pdef[t] = True

    def resend_tip_of_kind(self, kind):
        tips = [t for t in range(self.L.T) if (self.tipkind[t] == "compact") == (kind == "compact")]
        if tips:
            self.resend_tip(tips[int(self.rng.integers(len(tips)))])
        return bool(tips)

    def compact_to_partials(self):
        tips = [t for t in range(self.L.T) if self.tipkind[t] == "compact" and t != self.first_compact]
        if not tips:
            return False
        t = tips[int(self.rng.integers(len(tips)))]
        self.emit("setTipPartials", [t, self.tip_partials()], "compactToPartials")
        self.tipkind[t] = "partials"
        return True

    def set_tip_emission(self):
        """engine: setTipEmission(tip, codes, table); oracle: setTipPartials of the expanded table.  4 states: the sequence-error
        model's table (every base read correctly with 1 - e, as any other with e / 3; tests/tip_models_reference.py expands it pattern
        by pattern); 20 states: K rows (K <= S folds into the tip's matrix, K > S is expanded on the device)."""
        L, rng = self.L, self.rng
        if L.S not in EMISSION_STATES:
            return False
        tips = [t for t in range(L.T) if t != self.first_compact]
        t = tips[int(rng.integers(len(tips)))]
        if L.S == 4:
            e = float(rng.uniform(0.001, 0.05))
            table = np.full((4, 4), (1.0 - (1.0 - e)) / 3.0)
            table[np.arange(4), np.arange(4)] = 1.0 - e
            codes = rng.integers(0, 4, size=L.P)
            codes[rng.random(L.P) < 0.02] = 4
            extra = {"base_rate": e}
        else:
            K = int(rng.choice([L.S - 3, L.S, L.S + 5]))
            table = rng.uniform(0.02, 0.1, size=(K, L.S))
            table[np.arange(K), rng.integers(0, L.S, size=K)] = 1.0
            codes = rng.integers(0, K, size=L.P)
            codes[rng.random(L.P) < 0.02] = K
            extra = {}
        self.emit("setTipEmission", [t, _lst(codes), _lst(table), extra], "setTipEmission")
        self.tipkind[t] = "emission"
        self.pdef[t] = True
        return True

    def set_partials(self, b=None):
        L = self.L
        if b is None:
            n = self.internal[int(self.rng.integers(len(self.internal)))]
            b = L.post(n, int(self.rng.integers(2)))
        self.emit("setPartials", [b, self.node_partials()], "setPartials")
        self.pdef[b] = True
        self.pscale[b] = NONE

    # ---- matrix calls ----------------------------------------------------------------------------------------------------------
    def branches(self):
        return [n for n in range(self.L.N) if n != self.L.root]

    def update_matrices(self, nodes=None, flip=True, slots=None, action="updateTransitionMatrices", multiple=False, eigen=None):
        """new branch lengths for `nodes` into their (flipped) matrix slots, or detached lengths into the spare `slots`"""
        L, rng = self.L, self.rng
        if slots is None:
            if nodes is None:
                kind = rng.random()
                nodes = self.branches()
                if kind > 0.4:
                    k = int(rng.integers(1, len(nodes)))
                    nodes = sorted(_lst(rng.choice(nodes, size=k, replace=False)))
            slots = []
            for n in nodes:
                if flip:
                    self.mcur[n] ^= 1
                slots.append(L.matrix(n, self.mcur[n]))
                self.length_of[n] = self.a_length()
            lengths = [float(self.length_of[n]) for n in nodes]
        else:
            lengths = [self.a_length() for _ in slots]
        if multiple:
            e = _lst(rng.integers(0, 2, size=len(slots)))
            r = _lst(rng.integers(0, 2, size=len(slots)))
            self.emit("updateTransitionMatricesWithMultipleModels", [e, r, slots, None, None, lengths, len(slots)],
                      "updateTransitionMatricesWithMultipleModels")
        else:
            e = [int(rng.integers(2)) if eigen is None else eigen] * len(slots)
            r = [0] * len(slots)
            self.emit("updateTransitionMatrices", [e[0], slots, None, None, lengths, len(slots)], action)
        for k, m in enumerate(slots):
            self.mdef[m] = "prob"
            self.mfrom[m] = (e[k], self.eigen_version[e[k]], r[k], self.rates_version[r[k]], lengths[k])
        return slots

    def prob_slots(self):
        return [m for m in range(self.L.matrix_count) if self.mdef[m] == "prob"]

    def set_transition_matrix(self, m=None):
        if m is None:
            m = self.prob_slots()[int(self.rng.integers(len(self.prob_slots())))] if self.rng.random() < 0.7 else self.L.spare[int(self.rng.integers(2))]
        self.emit("setTransitionMatrix", [m, self.random_matrix(), 1.0], "setTransitionMatrix")
        self.mdef[m] = "prob"
        self.mfrom[m] = None
        return m

    def triples(self, method, result=None):
        """1-3 triples; a later one may read an earlier result (a dependent chain)"""
        L, rng = self.L, self.rng
        k = 1 if result is not None else int(rng.integers(1, 4))
        first, second, res = [], [], []
        for i in range(k):
            src = [m for m in self.prob_slots() if m not in L.spare[:2]] + res
            r = result if result is not None else L.spare[i % 2]
            pool = [m for m in src if m != r]
            if i and rng.random() < 0.5:
                a = res[-1] if res[-1] != r else pool[0]           # dependent on the triple before
            else:
                a = pool[int(rng.integers(len(pool)))]
            b = pool[int(rng.integers(len(pool)))]
            first.append(a); second.append(b); res.append(r)
        n = len(res)
        self.emit(method, [first, second, res, n], method)
        for m in res:
            self.mdef[m] = "prob"
            self.mfrom[m] = None

    def transpose(self):
        L, rng = self.L, self.rng
        src = [m for m in self.prob_slots() if m not in L.spare[:2]]
        k = int(rng.integers(1, 3))
        a = [src[int(rng.integers(len(src)))] for _ in range(k)]
        self.emit("transposeTransitionMatrices", [a, L.spare[:k], k], "transposeTransitionMatrices")
        for m in L.spare[:k]:
            self.mdef[m] = "prob"
            self.mfrom[m] = None

    def get_matrix(self, m=None):
        slots = [m for m in range(self.L.matrix_count) if self.mdef[m]]
        m = slots[int(self.rng.integers(len(slots)))] if m is None else m
        self.emit("getTransitionMatrix", [m], "getTransitionMatrix")

    # ---- operation lists ---------------------------------------------------------------------------------------------------------
    def pick_nodes(self):
        """(nodes in list order): the whole tree, one subtree or one tip-to-root path; post-order or reverse level order"""
        L, rng = self.L, self.rng
        kind = rng.random()
        if kind < 0.45:
            nodes = list(self.internal)
        elif kind < 0.7:
            top = self.internal[int(rng.integers(len(self.internal)))]
            nodes, stack = [], [top]
            while stack:
                n = stack.pop()
                if n >= L.T:
                    nodes.append(n)
                    stack += [self.left[n], self.right[n]]
        else:
            n = self.parent[int(rng.integers(L.T))]
            nodes = []
            while n != NONE:
                nodes.append(n)
                n = self.parent[n]
        if rng.random() < 0.5:
            return self.post_order(nodes)
        return sorted(nodes, key=lambda n: (self.level[n], n))

    def post_order(self, nodes):
        keep, out, stack = set(nodes), [], [(self.L.root, False)]
        while stack:
            n, done = stack.pop()
            if n < self.L.T:
                continue
            if done:
                if n in keep:
                    out.append(n)
            else:
                stack += [(n, True), (self.right[n], False), (self.left[n], False)]
        return out

    def raw_scales(self):
        return [s for s in range(self.L.scale_count) if self.sdef[s] == "raw"]

    def log_scales(self):
        return [s for s in range(self.L.scale_count) if self.sdef[s] == "log"]

    def build_list(self, nodes, mode, flip=True, dest_set=None, again=None):
        """7-int operations for `nodes` in that order; mode "none" / "write" / "read"; dest_set {node: set} overrides the flip.
        `again`: one node of the list recomputed at the end of it into the buffer its parent's operation has read (sequential semantics)."""
        L = self.L
        ops, meta = [], {}
        for k, n in enumerate(list(nodes) + ([again] if again is not None else [])):
            if k >= len(nodes):
                j = self.cur[n]                              # (the buffer it was written to earlier in this list, read since)
            else:
                j = dest_set[n] if dest_set is not None else (self.cur[n] ^ 1 if flip else self.cur[n])
            dest = L.post(n, j)
            l, r = self.left[n], self.right[n]
            cl, cr = L.post(l, self.cur[l]), L.post(r, self.cur[r])
            ws = rs = NONE
            if mode == "write":
                ws = L.scale(n, j)
            elif mode == "read":
                own = L.scale(n, self.cur[n])
                raw = self.raw_scales()
                rs = own if self.sdef[own] == "raw" else raw[int(self.rng.integers(len(raw)))]
            ops += [dest, ws, rs, cl, L.matrix(l, self.mcur[l]), cr, L.matrix(r, self.mcur[r])]
            self.cur[n] = j
            meta[n] = j
            self.pdef[dest] = True
            self.pscale[dest] = ws if ws != NONE else rs
            if ws != NONE:
                self.sdef[ws] = "raw"
        return ops, meta

    def update_partials(self, mode=None, cum_on_call=None, nodes=None, flip=True, dest_set=None, again=False):
        L, rng = self.L, self.rng
        if mode is None:
            mode = ("none", "write", "read")[int(rng.integers(3))]
        if mode == "read" and not self.raw_scales():
            mode = "write"
        nodes = self.pick_nodes() if nodes is None else nodes
        extra = None
        if again and len(nodes) > 1:
            extra = nodes[int(rng.integers(len(nodes) - 1))]
        cum = NONE
        if mode == "write" and (cum_on_call if cum_on_call is not None else rng.random() < 0.35) and self.log_scales():
            logs = [c for c in L.cum if self.sdef[c] == "log"]
            if logs:
                cum = logs[int(rng.integers(len(logs)))]
        ops, meta = self.build_list(nodes, mode, flip=flip, dest_set=dest_set, again=extra)
        count = len(ops) // 7
        if cum != NONE:
            self.accumulated[cum] += [ops[7 * k + 1] for k in range(count)]
        action = "updatePartials:cumulative" if cum != NONE else "updatePartials:" + mode
        self.emit("updatePartials", [ops, count, cum], action)
        self.last_list = {"ops": ops, "count": count, "nodes": list(nodes), "meta": meta, "mode": mode}
        return ops

    def repeat_list(self):
        """the last list again, verbatim (no cumulative index)"""
        ll = self.last_list
        for k in range(ll["count"]):
            op = ll["ops"][7 * k:7 * k + 7]
            self.pdef[op[0]] = True
            if op[1] != NONE:
                self.sdef[op[1]] = "raw"
            self.pscale[op[0]] = op[1] if op[1] != NONE else op[2]
        for n, j in ll["meta"].items():
            self.cur[n] = j
        self.emit("updatePartials", [list(ll["ops"]), ll["count"], NONE], "updatePartials:" + ll["mode"])

    def wait_for_partials(self):
        b = [self.L.post(n, self.cur[n]) for n in self.internal[:2]]
        self.emit("waitForPartials", [b, len(b)], "waitForPartials")

    # ---- scale-buffer calls ----------------------------------------------------------------------------------------------------
    def reset_scale(self, c=None):
        c = self.L.cum[int(self.rng.integers(2))] if c is None else c
        self.emit("resetScaleFactors", [c], "resetScaleFactors")
        self.sdef[c] = "log"
        if c in self.accumulated:
            self.accumulated[c] = []

    def a_log_cum(self):
        logs = [c for c in self.L.cum if self.sdef[c] == "log"]
        return logs[int(self.rng.integers(len(logs)))] if logs else None

    def accumulate(self, c=None, idx=None):
        c = self.a_log_cum() if c is None else c
        src = [s for s in self.raw_scales() if s != c]
        if c is None or not src:
            return False
        if idx is None:
            current = [self.pscale[self.L.post(n, self.cur[n])] for n in self.internal]
            current = [s for s in current if s != NONE and self.sdef[s] == "raw" and s != c]
            pool = current if current and self.rng.random() < 0.7 else src
            k = int(self.rng.integers(1, len(pool) + 1))
            idx = sorted(set(_lst(self.rng.choice(pool, size=k, replace=False))))
        self.emit("accumulateScaleFactors", [idx, len(idx), c], "accumulateScaleFactors")
        self.accumulated.setdefault(c, []).extend(idx)
        return True

    def remove(self):
        """takes out again some of what was accumulated (short chains: at most three buffers a call)"""
        cands = [c for c in self.L.cum if self.sdef[c] == "log" and [s for s in self.accumulated[c] if self.sdef[s] == "raw"]]
        if not cands:
            return False
        c = cands[int(self.rng.integers(len(cands)))]
        have = sorted(set(s for s in self.accumulated[c] if self.sdef[s] == "raw"))
        k = int(self.rng.integers(1, min(3, len(have)) + 1))
        idx = sorted(_lst(self.rng.choice(have, size=k, replace=False)))
        self.emit("removeScaleFactors", [idx, k, c], "removeScaleFactors")
        for s in idx:
            self.accumulated[c].remove(s)
        return True

    def copy_scale(self, dst=None, src=None):
        L = self.L
        defined = [s for s in range(L.scale_count) if self.sdef[s]]
        if src is None:
            src = defined[int(self.rng.integers(len(defined)))]
            dst = L.cum[int(self.rng.integers(2))] if self.sdef[src] == "log" else int(self.rng.integers(L.scale_count - 2))
            if dst == src:
                return False
        self.emit("copyScaleFactors", [dst, src], "copyScaleFactors")
        self.sdef[dst] = self.sdef[src]
        if dst in self.accumulated:
            self.accumulated[dst] = list(self.accumulated.get(src, []))
        return True

    def get_scale(self, s=None):
        defined = [k for k in range(self.L.scale_count) if self.sdef[k]]
        s = defined[int(self.rng.integers(len(defined)))] if s is None else s
        self.emit("getLogScaleFactors", [s], "getLogScaleFactors")

    # ---- root calls and reads ----------------------------------------------------------------------------------------------------
    def root_call(self, where=None, cum=None, b=None):
        L, rng = self.L, self.rng
        if where is None:
            where = "root" if rng.random() < 0.6 else "other"
        if b is None:
            if where == "root":
                b = L.post(L.root, self.cur[L.root])
            else:
                pool = [L.post(n, j) for n in self.internal for j in (0, 1) if self.pdef[L.post(n, j)] and L.post(n, j) != L.post(L.root, self.cur[L.root])]
                b = pool[int(rng.integers(len(pool)))]
        if cum is None:
            cum = rng.random() < 0.4
        c = NONE
        if cum:
            logs = self.log_scales()
            c = logs[int(rng.integers(len(logs)))] if logs else NONE
        action = "calculateRootLogLikelihoods:" + ("cumulative" if c != NONE else where)
        self.emit("calculateRootLogLikelihoods", [[b], [int(rng.integers(2))], [int(rng.integers(2))], [c], 1], action)
        self.root_done = True

    def get_sites(self):
        if not self.root_done:
            self.root_call()
        self.emit("getSiteLogLikelihoods", [], "getSiteLogLikelihoods")

    def readable(self):
        L = self.L
        return [b for b in range(L.pre_base) if self.pdef[b] and not (b < L.T and self.tipkind[b] == "compact")]

    def get_partials(self, b=None, scaled=None):
        rng = self.rng
        pool = self.readable()
        b = pool[int(rng.integers(len(pool)))] if b is None else b
        scaled = rng.random() < 0.4 if scaled is None else scaled
        s = NONE
        if scaled:
            defined = [k for k in range(self.L.scale_count) if self.sdef[k]]
            s = self.pscale[b] if self.pscale[b] != NONE and rng.random() < 0.5 else defined[int(rng.integers(len(defined)))]
        self.emit("getPartials", [b, s], "getPartials:scaled" if s != NONE else "getPartials")

    def get_partials_batch(self):
        rng = self.rng
        pool = self.readable()
        k = int(rng.integers(2, 4))
        b = [pool[int(rng.integers(len(pool)))] for _ in range(k)]
        sc = None
        if rng.random() < 0.4:
            defined = [s for s in range(self.L.scale_count) if self.sdef[s]]
            sc = [NONE if rng.random() < 0.5 else defined[int(rng.integers(len(defined)))] for _ in b]
        self.emit("getPartialsBatch", [b, sc], "getPartialsBatch")

    # ---- gradient calls --------------------------------------------------------------------------------------------------------
    def set_root_pre(self):
        L = self.L
        self.emit("setRootPrePartials", [[L.pre(L.root)], [int(self.rng.integers(2))], 1], "setRootPrePartials")
        self.pdef[L.pre(L.root)] = True

    def update_pre(self, whole=None):
        """pre-order operations from the root down: the whole tree, or the path to one internal node (both children of every node
        on it)"""
        L, rng = self.L, self.rng
        if not self.pdef[L.pre(L.root)]:
            self.set_root_pre()
        whole = rng.random() < 0.6 if whole is None else whole
        if whole:
            parents, stack = [], [L.root]
            while stack:
                n = stack.pop()
                if n >= L.T:
                    parents.append(n)
                    stack += [self.right[n], self.left[n]]
        else:
            n = self.internal[int(rng.integers(len(self.internal)))]
            parents = []
            while n != NONE:
                parents.insert(0, n)
                n = self.parent[n]
        ops = []
        for n in parents:
            l, r = self.left[n], self.right[n]
            for child, sib in ((l, r), (r, l)):
                ops += [L.pre(child), NONE, NONE, L.pre(n), L.matrix(child, self.mcur[child]), L.post(sib, self.cur[sib]),
                        L.matrix(sib, self.mcur[sib])]
                self.pdef[L.pre(child)] = True
        self.emit("updatePrePartials", [ops, len(ops) // 7, NONE], "updatePrePartials")
        self.last_pre = {"ops": ops, "parents": parents}

    def set_differential(self, k=0):
        L = self.L
        slot = int(self.rng.integers(2))
        q = self.models[slot][4]
        if k:
            q = q @ q
        m = np.concatenate([(q * r ** (k + 1)).ravel() for r in self.rates[slot]])
        self.emit("setDifferentialMatrix", [L.spare[2 + k], _lst(m)], "setDifferentialMatrix")
        self.mdef[L.spare[2 + k]] = "diff"
        self.dkind[L.spare[2 + k]] = "QQ" if k else "Qrate"

    def edges_with_pre(self):
        L = self.L
        return [n for n in range(L.N) if n != L.root and self.pdef[L.pre(n)]]

    def edge_differentials(self, want=None, all_edges=False):
        L, rng = self.L, self.rng
        if not self.edges_with_pre():
            self.update_pre()
        diffs = [m for m in L.spare[2:] if self.mdef[m] == "diff"]
        if not diffs:
            self.set_differential(0)
            diffs = [L.spare[2]]
        edges = self.edges_with_pre()
        if not all_edges and rng.random() < 0.5:
            edges = sorted(_lst(rng.choice(edges, size=int(rng.integers(1, len(edges) + 1)), replace=False)))
        post = [L.post(n, self.cur[n]) for n in edges]
        pre = [L.pre(n) for n in edges]
        d = [diffs[int(rng.integers(len(diffs)))]] * len(edges)
        # what is asked for: the sums alone (a held list can answer and stay held), sums of squares as well (it runs together with the
        # derivatives), per-pattern values too (it has to run first)
        want = [[False, False], [False, True], [True, True]][int(rng.integers(3)) if want is None else want]
        self.emit("calculateEdgeDifferentials", [post, pre, d, [int(rng.integers(2))], len(edges), want], "calculateEdgeDifferentials")

    def cross_products(self):
        L, rng = self.L, self.rng
        if not self.edges_with_pre():
            self.update_pre()
        edges = self.edges_with_pre()
        post = [L.post(n, self.cur[n]) for n in edges]
        pre = [L.pre(n) for n in edges]
        self.emit("calculateCrossProductDifferentials", [post, pre, [int(rng.integers(2))], [int(rng.integers(2))],
                                                         [float(self.length_of[n]) for n in edges], len(edges)],
                  "calculateCrossProductDifferentials")

    def get_pre_partials(self):
        L = self.L
        pool = [L.pre(n) for n in range(L.N) if self.pdef[L.pre(n)]]
        if not pool:
            self.update_pre()
            pool = [L.pre(n) for n in range(L.N) if self.pdef[L.pre(n)]]
        self.emit("getPartials", [pool[int(self.rng.integers(len(pool)))], NONE], "getPartials:pre")

    # ---- profile "extensions": the one-call entry points --------------------------------------------------------------------
    def a_seed(self):
        return int(self.rng.integers(1, 2 ** 62))

    def preorder_rows(self, whole=None):
        """-> (nodes, rows {post buffer, branch matrix, parent row}, compact buffers): the pre-order list of the whole tree or of the
        subtree under a random internal node, over the current buffers and matrices (all defined)"""
        L, rng = self.L, self.rng
        whole = rng.random() < 0.5 if whole is None else whole
        top = L.root if whole else self.internal[int(rng.integers(len(self.internal)))]
        nodes, rows, stack = [], [], [(top, NONE)]
        while stack:
            n, parent_row = stack.pop()
            assert self.pdef[L.post(n, self.cur[n])] and (n == top or self.mdef[L.matrix(n, self.mcur[n])] == "prob")
            nodes.append(n)
            rows.append([L.post(n, self.cur[n]), 0 if n == top else L.matrix(n, self.mcur[n]), parent_row])
            if n >= L.T:
                stack += [(self.right[n], len(rows) - 1), (self.left[n], len(rows) - 1)]
        return nodes, rows, [n for n in nodes if n < L.T and self.tipkind[n] == "compact"]

    def sample_ancestral(self, whole=None):
        rng = self.rng
        _, rows, compact = self.preorder_rows(whole)
        self.emit("sampleAncestralStates", [rows, int(rng.integers(2)), int(rng.integers(2)), self.a_seed(), bool(rng.random() < 1.0 / 3.0),
                                            compact], "sampleAncestralStates")

    def jump_source(self, nodes):
        """the (eigen slot, rate slot) that every branch matrix of `nodes` (the first is the list's root) was built from, at the branch's
        length and unchanged since; else None"""
        L = self.L
        src = set()
        for n in nodes[1:]:
            f = self.mfrom[L.matrix(n, self.mcur[n])]
            if f is None or f[1] != self.eigen_version[f[0]] or f[3] != self.rates_version[f[2]] or f[4] != float(self.length_of[n]):
                return None
            src.add((f[0], f[2]))
        return src.pop() if len(src) == 1 else None

    def prepare_jumps(self, nodes, eigen=None):
        """sampleMarkovJumps forms Q and the times' distances from ONE eigen slot and rate slot: every branch matrix from them, else
        first an updateTransitionMatrices over all branches"""
        src = self.jump_source(nodes)
        if src is None or (eigen is not None and src[0] != eigen):
            self.update_matrices(nodes=self.branches(), eigen=eigen)
            src = self.jump_source(nodes)
        return src

    def sample_jumps(self, whole=None, eigen=None):
        """one count register (every substitution weighted by a random R) and one reward register, scaled by time"""
        L, rng = self.L, self.rng
        nodes, rows, compact = self.preorder_rows(whole)
        src = self.prepare_jumps(nodes, eigen)
        rows = [[r[0], 0 if k == 0 else L.matrix(nodes[k], self.mcur[nodes[k]]), r[2]] for k, r in enumerate(rows)]    # (matrix sets may have flipped)
        times = [0.0] + [float(self.length_of[n]) for n in nodes[1:]]
        registers = [_lst(rng.uniform(0.0, 1.0, size=(L.S, L.S))), _lst(np.diag(rng.uniform(0.0, 2.0, size=L.S)))]
        self.emit("sampleMarkovJumps", [rows, times, src[0], src[1], int(rng.integers(2)), int(rng.integers(2)), registers,
                                        [0, JUMPS_REWARDS | JUMPS_SCALE_BY_TIME], self.a_seed(), bool(rng.random() < 1.0 / 3.0), compact],
                  "sampleMarkovJumps")

    def simulate(self):
        L, rng = self.L, self.rng
        _, rows, _ = self.preorder_rows()
        rows = [[k, r[1], r[2]] for k, r in enumerate(rows)]               # every row's states come back, in row order
        sites = int(SITE_COUNTS[int(rng.integers(len(SITE_COUNTS)))])
        root = cats = None
        if rng.random() < 1.0 / 3.0:
            root, cats = _lst(rng.integers(0, L.S, size=sites)), _lst(rng.integers(0, L.C, size=sites))
        self.emit("simulateSequences", [rows, sites, int(rng.integers(2)), int(rng.integers(2)), self.a_seed(), root, cats],
                  "simulateSequences")

    def node_height(self):
        """one row per internal node whose pre-order partial is defined; the differential slot holds Q x category rate"""
        L, rng = self.L, self.rng
        if self.dkind.get(L.spare[2]) != "Qrate":
            self.set_differential(0)
        if not [i for i in self.internal if self.pdef[L.pre(i)]]:
            self.update_pre()
        dq = L.spare[2]
        rows, rates, compact = [], [], []
        for i in self.internal:
            if not self.pdef[L.pre(i)]:
                continue
            j, k = self.left[i], self.right[i]
            rows.append([L.pre(i), L.post(j, self.cur[j]), L.matrix(j, self.mcur[j]), dq, L.post(k, self.cur[k]), L.matrix(k, self.mcur[k]),
                         dq, NONE if i == L.root else dq])
            rates.append(_lst(rng.uniform(0.5, 2.0, size=3)))
            compact += [t for t in (j, k) if t < L.T and self.tipkind[t] == "compact"]
        first, second = [(True, False), (False, True), (True, True)][int(rng.integers(3))]
        self.emit("nodeHeightDerivatives", [rows, rates, int(rng.integers(2)), first, second, sorted(set(compact))], "nodeHeightDerivatives")

    def update_differential(self, slots=None, lengths=None):
        """D of dQ = the derivative of the eigen slot's unnormalised generator in one exchange rate (rows sum to zero) into differential
        slots, at lengths of the tree's branches; EXACT inputs are kept away from the 1e-10 thresholds (another exchange rate is drawn
        until differential_matrices_reference.assert_guard holds)"""
        import differential_matrices_reference as dm
        L, rng = self.L, self.rng
        if slots is None:
            slots = [[L.spare[2]], [L.spare[3]], L.spare[2:]][int(rng.integers(3))]
        e = _lst(rng.integers(0, 2, size=len(slots)))
        r = _lst(rng.integers(0, 2, size=len(slots)))
        mode = dm.EXACT if rng.random() < 2.0 / 3.0 else dm.FIRST_ORDER
        dqs = []
        for slot in sorted(set(e)):
            u, ui, lam, pi, _ = self.models[slot]
            for attempt in range(20):
                a, b = sorted(_lst(rng.choice(L.S, size=2, replace=False)))
                dq = np.zeros((L.S, L.S))
                dq[a, b], dq[b, a] = pi[b], pi[a]
                dq -= np.diag(dq.sum(axis=1))
                if mode != dm.EXACT:
                    break
                try:
                    dm.assert_guard(dm.rotate(u, ui, dq)[1], lam, L.S)
                    break
                except AssertionError:
                    continue
            else:
                mode = dm.FIRST_ORDER
            dqs.append(_lst(dq))
        d = [sorted(set(e)).index(x) for x in e]
        if lengths is None:
            lengths = [float(self.length_of[self.branches()[int(rng.integers(L.N - 1))]]) for _ in slots]
        self.emit("updateDifferentialMatrices", [e, r, dqs, d, list(slots), lengths, int(mode)], "updateDifferentialMatrices")
        for m in slots:
            self.mdef[m] = "diff"
            self.mfrom[m] = None
            self.dkind[m] = "D"

    def set_reversible(self, slots=None):
        """one or both eigen slots decomposed on the device; everything set_eigen keeps is kept here"""
        L, rng = self.L, self.rng
        if slots is None:
            slots = [[0], [1], [0, 1], [1, 0]][int(rng.integers(4))]
        rates, freqs = [], []
        for slot in slots:
            upper = rng.uniform(0.5, 1.5, size=L.S * (L.S - 1) // 2)
            pi = rng.dirichlet(np.full(L.S, 20.0))
            self.models[slot] = decompose_reversible(symmetric_rates(upper, L.S), pi)
            self.eigen_version[slot] += 1
            rates.append(_lst(upper))
            freqs.append(_lst(pi))
        self.emit("setReversibleModels", [list(slots), rates, freqs], "setReversibleModels")

    def get_eigen(self, slot=None):
        self.emit("getEigenDecomposition", [int(self.rng.integers(2)) if slot is None else slot], "getEigenDecomposition")

    def gradient_set_up(self, mode="none"):
        """what motifs (j) and (m) — and (n), (o), (p) — start from: a whole-tree list, a root call, the differential slot, a held
        whole-tree pre-order list"""
        self.update_partials(mode=mode, cum_on_call=False, nodes=self.post_order(self.internal))
        self.root_call("root", cum=False)
        self.set_differential(0)
        self.set_root_pre()
        self.update_pre(whole=True)

    def motif_j(self):
        """a whole-tree updatePrePartials (held back on 4 states), one of the calls that decide for themselves whether the list runs,
        the edge derivatives' sums (which a list still held answers); two variants per sequence"""
        L = self.L
        for k in (0, 1):
            self.variant = v = J_VARIANTS[(2 * self.seed + k) % len(J_VARIANTS)]
            self.gradient_set_up()
            if v == "updateDifferentialMatrices":
                self.update_differential(slots=[L.spare[3]])
            elif v == "setReversibleModels":
                self.set_reversible([int(self.rng.integers(2))])
            elif v == "nodeHeightDerivatives":
                self.node_height()
            elif v == "sampleAncestralStates":
                self.sample_ancestral(whole=True)
            elif v == "simulateSequences":
                self.simulate()
            self.edge_differentials(want=0, all_edges=True)

    def motif_k(self):
        """a model move on the device: setReversibleModels(slot), every branch matrix from that slot, the partials, a root call, the
        Markov jumps on that slot (Q from an eigen system the device wrote); variant "reupload": the slot's PREVIOUS values are
        uploaded behind the device's write — an upload that a stale host shadow would skip"""
        slot = int(self.rng.integers(2))
        self.variant = v = K_VARIANTS[self.seed % 2]
        previous = self.models[slot]
        self.set_reversible([slot])
        if v == "reupload":
            self.models[slot] = previous
            self.set_eigen(slot, same=True)
        self.update_matrices(nodes=self.branches(), eigen=slot)
        self.update_partials(mode="none", nodes=self.post_order(self.internal))
        self.root_call("root", cum=False)
        self.sample_jumps(whole=True, eigen=slot)
        self.get_eigen(slot)

    def motif_l(self):
        """a sampler right behind a whole-tree list with flipped buffers and no root call (unstored nodes, a held walk); at 4 and 20
        states also with a tip's emission table set first (a folded tip that the sampler has to demote)"""
        L = self.L
        pool = L_VARIANTS if L.S in EMISSION_STATES else L_VARIANTS[:2]
        self.variant = v = pool[self.seed % len(pool)]
        if v.startswith("emission"):
            self.set_tip_emission()
        if v.endswith("jumps"):
            self.prepare_jumps([L.root] + self.branches())
        self.update_partials(mode="none", nodes=self.post_order(self.internal))
        if v.endswith("jumps"):
            self.sample_jumps(whole=True)
        else:
            self.sample_ancestral(whole=True)

    def motif_m(self):
        """a differential matrix written over a branch matrix that the held pre-order list reads (the list has to run first), the
        branch's matrix put back, the child's pre-order partial read"""
        L = self.L
        self.gradient_set_up()
        child = self.left[L.root]
        m = L.matrix(child, self.mcur[child])
        self.update_differential(slots=[m], lengths=[float(self.length_of[child])])
        self.dkind.pop(m, None)
        self.update_matrices(nodes=[child], flip=False)
        self.emit("getPartials", [L.pre(child), NONE], "getPartials:pre")

    # ---- profile "queries": the five entry points merged after the extension profile -------------------------------------------
    def pick(self, pool):
        return pool[int(self.rng.integers(len(pool)))]

    def generator_matrices(self, slots=None, lengths=None):
        """exp(Q d) from one or two generators, each the Q of an eigen slot's model, into one to four slots: current branch matrices at
        their branches' lengths, or the two spare product slots at the length of some branch"""
        L, rng = self.L, self.rng
        models = [[0], [1], [0, 1]][int(rng.integers(3))]
        if slots is None:
            pool = [L.matrix(n, self.mcur[n]) for n in self.branches()] + L.spare[:2]
            slots = sorted(_lst(rng.choice(pool, size=int(rng.integers(1, 5)), replace=False)))
        if lengths is None:
            lengths = [float(self.length_of[m % L.N if m < 2 * L.N else self.pick(self.branches())]) for m in slots]
        g = _lst(rng.integers(0, len(models), size=len(slots)))
        r = _lst(rng.integers(0, 2, size=len(slots)))
        self.emit("updateTransitionMatricesFromGenerators", [[_lst(self.models[s][4]) for s in models], g, r, list(slots), list(lengths),
                                                             len(slots)], "updateTransitionMatricesFromGenerators")
        for m in slots:
            self.mdef[m] = "prob"
            self.mfrom[m] = None

    def epoch_matrices(self, nodes=None, slots=None, lengths=None, flip=False, must=None):
        """One to three entries (or one per node of `nodes`), each the left fold of one to three segments over the two eigen slots whose
        lengths add up to the branch's; one rate set per entry.  The first entry of a sequence has a single segment (the oracle side
        makes such an entry with its own updateTransitionMatricesWithMultipleModels).  `must`: an eigen slot every entry reads (and
        with two segments or more the other one as well)."""
        L, rng = self.L, self.rng
        if nodes is None:
            nodes = sorted(_lst(rng.choice(self.branches(), size=int(rng.integers(1, 4)), replace=False)))
            spare = list(L.spare[:2])
            slots = [spare.pop(0) if spare and rng.random() < 0.3 else L.matrix(n, self.mcur[n]) for n in nodes]
        elif slots is None:
            slots = []
            for n in nodes:
                if flip:
                    self.mcur[n] ^= 1
                slots.append(L.matrix(n, self.mcur[n]))
        offsets, eig, seg, rate = [0], [], [], []
        for i, n in enumerate(nodes):
            k = 1 if (i == 0 and not self.single_epoch) else int(rng.integers(1, 4))
            self.single_epoch = self.single_epoch or k == 1
            e = _lst(rng.integers(0, 2, size=k))
            if must is not None:
                e[0] = must
                if k > 1:
                    e[1] = 1 - must
            t = float(self.length_of[n]) if lengths is None else lengths[i]
            eig += e
            seg += [t] if k == 1 else _lst(rng.dirichlet(np.full(k, 2.0)) * t)
            offsets.append(len(eig))
            rate.append(int(rng.integers(2)))
        self.emit("updateTransitionMatricesWithEpochs", [offsets, eig, seg, rate, list(slots), len(slots)], "updateTransitionMatricesWithEpochs")
        for m in slots:
            self.mdef[m] = "prob"
            self.mfrom[m] = None

    def nodes_with_pre(self):
        return [n for n in range(self.L.N) if self.pdef[self.L.pre(n)]]

    def compact_among(self, buffers):
        return sorted(set(b for b in buffers if 0 <= b < self.L.T and self.tipkind[b] == "compact"))

    def node_posteriors(self, nodes=None):
        """rows {post, pre} over nodes whose pre-order buffer is defined (tips of every kind among them); at least one output"""
        L, rng = self.L, self.rng
        if not self.nodes_with_pre():
            self.update_pre()
        if nodes is None:
            pool = self.nodes_with_pre()
            if rng.random() < 0.6:
                pool = sorted(_lst(rng.choice(pool, size=int(rng.integers(1, len(pool) + 1)), replace=False)))
            nodes = pool
        rows = [[L.post(n, self.cur[n]), L.pre(n)] for n in nodes]
        full, use_map, totals, cats = (bool(x) for x in rng.random(4) < np.array([0.7, 0.5, 0.4, 0.4]))
        totals = totals and self.weights_set
        if not (full or use_map or totals or cats):
            full = True
        self.emit("nodePosteriors", [rows, int(rng.integers(2)), full, use_map, totals, cats, self.compact_among(r[0] for r in rows)],
                  "nodePosteriors")

    def death_states(self, tips):
        """the states d for which every pattern has a compact tip among `tips` whose state is known and is not d"""
        L = self.L
        sent = [np.asarray(self.tip_sent[t]) for t in tips if self.tipkind[t] == "compact"]
        if not sent:
            return []
        sent = np.stack(sent)
        return [d for d in range(L.S) if np.all(np.any((sent < L.S) & (sent != d), axis=0))]

    def node_pattern(self, whole=None, scale=None):
        """the post-order rows {buffer, scale buffer or -1, child rows} of the whole tree or of a subtree.  An internal row's scale
        buffer: -1, the buffer its partials were last written with while that holds raw factors, or a defined buffer of logarithms
        (`scale`: "raw" — the first of these where there is one —, or {node: buffer}, -1 for the others)."""
        L, rng = self.L, self.rng
        whole = rng.random() < 0.6 if whole is None else whole
        top = L.root if whole else self.pick(self.internal)
        while True:
            nodes, stack = [], [(top, False)]
            while stack:
                n, done = stack.pop()
                if done or n < L.T:
                    nodes.append(n)
                else:
                    stack += [(n, True), (self.right[n], False), (self.left[n], False)]
            death = self.death_states([n for n in nodes if n < L.T])
            if death or top == L.root:
                break
            top = L.root
        if not death:
            return False
        row_of = {n: k for k, n in enumerate(nodes)}
        rows = []
        for n in nodes:
            if n < L.T:
                rows.append([n, NONE, NONE, NONE])
                continue
            own = self.pscale[L.post(n, self.cur[n])]
            options = [NONE] + ([own] if own != NONE and self.sdef[own] == "raw" else [])
            if isinstance(scale, dict):
                sc = scale.get(n, NONE)
            elif scale == "raw":
                sc = options[-1]
            else:
                sc = self.pick(options + ([self.pick(self.log_scales())] if self.log_scales() else []))
            rows.append([L.post(n, self.cur[n]), sc, row_of[self.left[n]], row_of[self.right[n]]])
        self.emit("nodePatternLikelihoods", [rows, _lst(rng.uniform(-3.0, 0.0, size=len(rows))), int(self.pick(death)), int(rng.integers(2)),
                                             int(rng.integers(2)), bool(rng.random() < 0.5), self.compact_among(r[0] for r in rows)],
                  "nodePatternLikelihoods")

    def code_table(self):
        """S + 1 codes as tests/test_gpu_placement.py code_table builds them: the states 0 .. S - 2, a partially ambiguous row (the last
        two states), a real-valued emission row"""
        S = self.L.S
        return [np.eye(S)[s] for s in range(S - 1)] + [np.r_[np.zeros(S - 2), 1.0, 1.0], self.rng.uniform(0.05, 1.0, size=S)]

    def placement(self, tip_child=None):
        """two to six candidates: the first above the root, the second with a tip as its child (`tip_child`: that one), the others
        on any branch under a parent whose pre-order buffer is defined; lower, upper and pendant matrices from the spare slots or from
        any slot that holds probabilities"""
        L, rng = self.L, self.rng
        if not self.pdef[L.pre(L.root)]:
            self.set_root_pre()

        def pool():
            return [n for n in self.branches() if self.pdef[L.pre(self.parent[n])]]
        if not [n for n in pool() if n < L.T] or (tip_child is not None and tip_child not in pool()):
            self.update_pre(whole=True)
        tip = self.pick([n for n in pool() if n < L.T]) if tip_child is None else tip_child
        where = [L.root, tip] + [self.pick(pool() + [L.root]) for _ in range(int(rng.integers(0, 5)))]
        spare = [m for m in L.spare[:2] if self.mdef[m] == "prob"]

        def matrix():
            return self.pick(spare) if spare and rng.random() < 0.6 else self.pick(self.prob_slots())
        rows = []
        for n in where:
            if n == L.root:
                rows.append([L.pre(n), NONE, NONE, L.post(n, self.cur[n]), NONE, matrix(), matrix()])
                continue
            p = self.parent[n]
            s = self.right[p] if self.left[p] == n else self.left[p]
            assert self.mdef[L.matrix(s, self.mcur[s])] == "prob"
            rows.append([L.pre(p), L.post(s, self.cur[s]), L.matrix(s, self.mcur[s]), L.post(n, self.cur[n]),
                         NONE if rng.random() < 0.25 else matrix(), matrix(), matrix()])
        sites = int(self.pick(SITE_COUNTS))
        patterns = rng.integers(0, L.P, size=sites)
        patterns[rng.random(sites) < 0.05] = NONE
        queries = int(rng.integers(1, 4))
        codes = rng.integers(0, L.S + 1, size=(queries, sites))
        codes[rng.random((queries, sites)) < 0.05] = MISSING_CODE
        self.emit("placementScores", [rows, _lst(patterns), _lst(codes), _lst(np.stack(self.code_table())), int(rng.integers(2)),
                                      bool(rng.random() < 0.5), self.compact_among([r[1] for r in rows] + [r[3] for r in rows])],
                  "placementScores")

    def motif_n(self):
        """nodePosteriors behind a held whole-tree pre-order list (it always runs the list), over every internal node, then the edge
        derivatives' sums.  Variant "flipped": the post-order buffers freshly flipped by a whole-tree list with no root call behind it
        (unstored at 4 states); "set_pre": setPartials into one listed pre-order buffer between the list and the call (the list has
        to run before the setPartials, the call has to read what was set)"""
        L = self.L
        self.variant = v = N_VARIANTS[self.seed % 2]
        self.gradient_set_up()
        if v == "flipped":
            self.update_partials(mode="none", nodes=self.post_order(self.internal))
        else:
            inner = [n for n in self.internal if n != L.root]
            self.set_partials(L.pre(inner[len(inner) // 2]))
        self.node_posteriors(nodes=list(self.internal))
        self.edge_differentials(want=0, all_edges=True)

    def motif_o(self):
        """nodePatternLikelihoods over the whole tree behind a held whole-tree pre-order list that does not write its buffers (on 4
        states the list may stay held, or run late because something is materialised), then the edge derivatives' sums.  Variants:
        "plain"; "emission" (4 and 20 states): setTipEmission on a tip before the set-up, so the call demotes a folded tip under the
        list; "raw": the partials written with scale factors, every row naming its raw buffer; "log": likewise, the root's row naming
        a cumulative buffer that holds them all"""
        L = self.L
        pool = o_variants(L.S)
        self.variant = v = pool[self.seed % len(pool)]
        if v == "emission":
            self.set_tip_emission()
        if v == "log":
            self.update_partials(mode="write", cum_on_call=False, nodes=self.post_order(self.internal))
            self.reset_scale(L.cum[1])
            self.accumulate(L.cum[1], [L.scale(n, self.cur[n]) for n in self.internal])
            self.root_call("root", cum=False)
            self.set_differential(0)
            self.set_root_pre()
            self.update_pre(whole=True)
        else:
            self.gradient_set_up(mode="write" if v == "raw" else "none")
        self.node_pattern(whole=True, scale={"raw": "raw", "log": {L.root: L.cum[1]}}.get(v))
        self.edge_differentials(want=0, all_edges=True)

    def motif_p(self):
        """a branch matrix rewritten on the device behind a held whole-tree pre-order list — the matrix of the root's left child, which
        the list reads (it has to run first, over the old matrix), at another branch's length; variants "_spare": a spare slot
        (the list stays held) —, the edge derivatives' sums, the child's pre-order partial, the matrix put back"""
        L = self.L
        self.variant = v = P_VARIANTS[self.seed % len(P_VARIANTS)]
        self.gradient_set_up()
        child = self.left[L.root]
        m = L.spare[0] if v.endswith("_spare") else L.matrix(child, self.mcur[child])
        other = max(self.branches(), key=lambda n: abs(self.length_of[n] - self.length_of[child]))
        if v.startswith("generators"):
            self.generator_matrices(slots=[m], lengths=[float(self.length_of[other])])
        else:
            self.epoch_matrices(nodes=[child], slots=[m], lengths=[float(self.length_of[other])])
        self.edge_differentials(want=0, all_edges=True)
        self.emit("getPartials", [L.pre(child), NONE], "getPartials:pre")
        self.update_matrices(nodes=[child], flip=False)

    def motif_q(self):
        """placementScores right behind a whole-tree list with flipped buffers and no root call (motif (l)'s situation); at 4 and 20
        states also with a tip's emission table set first, that tip being the child of one candidate; then a root call: what
        materialising and demoting left behind must still evaluate"""
        L = self.L
        pool = q_variants(L.S)
        self.variant = v = pool[(self.seed // 2) % len(pool)]
        tip = None
        if v == "emission":
            self.set_tip_emission()
            tip = self.rec[-1]["a"][0]
        if len(self.nodes_with_pre()) < L.N:
            self.update_pre(whole=True)
        self.update_partials(mode="none", nodes=self.post_order(self.internal))
        self.placement(tip_child=tip)
        self.root_call("root", cum=False)
        self.get_sites()

    def motif_r(self):
        """epochs over an eigen slot the device wrote: setReversibleModels(slot), every branch's matrix from segments over both slots,
        the partials, a root call; variant "reupload": the slot's previous values uploaded behind the device's write and in front
        of the epoch call — motif (k)'s upload that must not be skipped"""
        slot = int(self.rng.integers(2))
        self.variant = v = R_VARIANTS[(self.seed // 2) % 2]
        previous = self.models[slot]
        self.set_reversible([slot])
        if v == "reupload":
            self.models[slot] = previous
            self.set_eigen(slot, same=True)
        self.epoch_matrices(nodes=self.branches(), flip=True, must=slot)
        self.update_partials(mode="none", nodes=self.post_order(self.internal))
        self.root_call("root", cum=False)
        self.get_sites()

    # ---- the set-up every sequence starts with -------------------------------------------------------------------------------
    def prelude(self):
        L = self.L
        self.first_compact = self.tipkind.index("compact")       # known in every pattern: no pattern is ambiguous at every tip
        for slot in (0, 1):
            self.set_eigen(slot)
            self.set_rates(slot, indexed=True)
            self.set_weights(slot)
            self.set_frequencies(slot)
        self.set_pattern_weights()
        for t in range(L.T):
            self.resend_tip(t)
        for j in (0, 1):
            self.mcur = [j] * L.N
            self.update_matrices(nodes=self.branches(), flip=False)
        self.update_matrices(slots=L.spare[:2])
        self.mcur = [0] * L.N
        self.cur = [1] * L.N
        self.update_partials(mode="write", cum_on_call=False, nodes=self.post_order(self.internal))
        self.reset_scale(L.cum[0])
        self.accumulate(L.cum[0], [L.scale(n, 0) for n in self.internal])
        self.reset_scale(L.cum[1])
        self.root_call("root", cum=False)
        self.set_differential(0)
        self.prelude_end = len(self.rec)
        self.gave_up = set()

    # ---- motifs: the call orders the engine's deferral logic branches on -------------------------------------------------------
    def motif_a(self):
        """the same eigen slot set twice, then updateTransitionMatrices (the earlier of two queued copies is dropped)"""
        slot = int(self.rng.integers(2))
        self.mcur_reads(1)                                   # (a read first: nothing else is queued when the two uploads are)
        self.set_eigen(slot)
        self.set_eigen(slot, same=self.seed % 4 == 0)
        self.update_matrices(nodes=self.branches()[:3], eigen=slot)
        self.mcur_reads(3)

    def mcur_reads(self, k):
        for n in self.branches()[:k]:
            self.get_matrix(self.L.matrix(n, self.mcur[n]))

    def motif_b(self):
        """setTransitionMatrix(m) then updateTransitionMatrices including m (the later call has to win), and the reverse order"""
        n = self.branches()[int(self.rng.integers(len(self.branches())))]
        m = self.L.matrix(n, self.mcur[n])
        self.set_transition_matrix(m)
        self.update_matrices(nodes=[n] + [x for x in self.branches()[:2] if x != n], flip=False)
        self.get_matrix(m)
        self.update_matrices(nodes=[n], flip=False)
        self.set_transition_matrix(m)
        self.get_matrix(m)

    def motif_c(self):
        """13 or more small uploads with no launch between them, then a launch"""
        k = 0
        while k < HOST_COPY_MAX + 1 + int(self.seed % 3):
            pick = k % 5
            if pick == 0:
                self.set_weights(k // 5 % 2)
            elif pick == 1:
                self.set_frequencies(k // 5 % 2)
            elif pick == 2:
                self.set_rates(k // 5 % 2, indexed=True)
            elif pick == 3:
                self.set_pattern_weights()
            else:
                self.set_eigen(k // 5 % 2)
            k += 1
        self.update_matrices(nodes=self.branches())
        self.update_partials(mode="none", nodes=self.post_order(self.internal))
        self.root_call("root", cum=False)
        self.get_sites()

    def motif_d(self):
        """updatePartials, then one kind of other call (by seed: over a shape's seeds every kind), then the root"""
        L = self.L
        self.variant = v = D_VARIANTS[(self.seed + 3 * self.d_count) % len(D_VARIANTS)]
        self.d_count += 1
        write = v in ("getLogScaleFactors", "resetScaleFactors", "copyScaleFactors")
        self.update_matrices(nodes=self.branches())
        self.update_partials(mode="write" if write else "none", cum_on_call=False, nodes=self.post_order(self.internal))
        mid = self.internal[len(self.internal) // 2]
        if v == "getPartials":
            self.get_partials(L.post(mid, self.cur[mid]), scaled=False)
        elif v == "getPartialsBatch":
            self.emit("getPartialsBatch", [[L.post(L.root, self.cur[L.root]), L.post(mid, self.cur[mid])], None], "getPartialsBatch")
        elif v == "getSiteLogLikelihoods":
            self.get_sites()
        elif v == "getLogScaleFactors":
            self.get_scale(L.scale(mid, self.cur[mid]))
        elif v == "resetScaleFactors":
            self.reset_scale(L.cum[0])
            self.accumulate(L.cum[0], [L.scale(n, self.cur[n]) for n in self.internal])
        elif v == "copyScaleFactors":
            self.reset_scale(L.cum[1])
            self.accumulate(L.cum[1], [L.scale(n, self.cur[n]) for n in self.internal])
            self.copy_scale(L.cum[0], L.cum[1])
        elif v == "setTransitionMatrix":
            self.set_transition_matrix(L.matrix(self.left[L.root], self.mcur[self.left[L.root]]))
        elif v == "setCategoryWeights":
            self.set_weights(0)
            self.set_weights(1)
        c = L.cum[0] if write else NONE
        self.emit("calculateRootLogLikelihoods", [[L.post(L.root, self.cur[L.root])], [0], [0], [c], 1],
                  "calculateRootLogLikelihoods:" + ("cumulative" if write else "root"))
        self.root_done = True
        self.get_sites()

    def motif_e(self):
        """root / site read three times in a row (the prefetch starts after two), a root whose site values are not read, a read"""
        for k in range(3):
            self.update_matrices(nodes=[self.branches()[k]])
            self.update_partials(mode="none", nodes=self.post_order(self.internal))
            self.root_call("root", cum=False)
            self.get_sites()
        self.update_matrices(nodes=[self.branches()[3]])
        self.update_partials(mode="none", nodes=self.post_order(self.internal))
        self.root_call("root", cum=False)
        self.update_partials(mode="none", nodes=self.post_order(self.internal))
        self.root_call("root", cum=False)
        self.get_sites()

    def motif_f(self):
        """updatePrePartials and the edge derivatives, then with one call between them that reads, writes or leaves alone the list's
        buffers and matrices (by seed)"""
        L = self.L
        self.variant = v = F_VARIANTS[(self.seed + 3 * self.f_count) % len(F_VARIANTS)]
        self.f_count += 1
        self.update_partials(mode="none", nodes=self.post_order(self.internal))
        self.root_call("root", cum=False)
        self.set_root_pre()
        self.update_pre(whole=True)
        # the order of a gradient evaluation first: setDifferentialMatrix leaves the list alone and the derivatives are answered from it
        # — the sums alone (it stays held back) or with their squares (it runs together with them and is sent again)
        self.set_differential(0)
        first = (self.seed + self.f_count) % 2
        self.edge_differentials(want=first, all_edges=True)
        if first == 1:
            self.update_pre(whole=True)
        child = self.left[L.root]
        inner = [n for n in self.internal if n != L.root]
        node = inner[len(inner) // 2]
        if v == "read_pre":
            self.emit("getPartials", [L.pre(node), NONE], "getPartials:pre")
        elif v == "read_post":
            self.get_partials(L.post(node, self.cur[node]), scaled=False)
        elif v == "write_post":
            self.set_partials(L.post(node, self.cur[node]))
        elif v == "write_matrix":
            self.update_matrices(nodes=[child], flip=False)
        elif v == "write_pre":
            self.set_partials(L.pre(child))
        elif v == "scale_call":
            self.reset_scale(L.cum[1])
        elif v == "model_call":
            self.set_weights(0)
            self.set_weights(1)
        elif v == "root_call":
            self.root_call("root", cum=False)
            self.get_sites()
        self.edge_differentials(want=(self.seed // 2 + self.f_count) % 2, all_edges=True)
        self.edge_differentials(want=int(self.rng.integers(3)), all_edges=True)
        if v == "scale_call":
            self.get_scale(L.cum[1])
        self.cross_products()
        self.get_pre_partials()

    def motif_g(self):
        """the identical operation list twice with only matrices changed (a plan replayed from the cache), then the same list with
        one buffer index flipped"""
        L = self.L
        nodes = self.post_order(self.internal)
        self.update_partials(mode="none", nodes=nodes)
        self.root_call("root", cum=False)
        self.update_matrices(nodes=self.branches(), flip=False)
        self.repeat_list()
        self.root_call("root", cum=False)
        meta = dict(self.last_list["meta"])
        n = nodes[len(nodes) // 2]
        meta[n] ^= 1
        self.update_partials(mode="none", nodes=nodes, dest_set=meta)
        self.root_call("root", cum=False)
        self.get_partials(L.post(n, self.cur[n]), scaled=False)

    def motif_h(self):
        """copyScaleFactors raw -> cumulative slot and cumulative -> raw slot, then a read-mode list and an accumulate"""
        L = self.L
        nodes = self.post_order(self.internal)
        self.update_partials(mode="write", cum_on_call=False, nodes=nodes)
        a, b = nodes[0], nodes[1]
        self.reset_scale(L.cum[0])
        self.accumulate(L.cum[0], [L.scale(n, self.cur[n]) for n in nodes])
        self.copy_scale(L.cum[1], L.scale(a, self.cur[a]))                     # raw factors into a cumulative slot
        spare_raw = L.scale(b, self.cur[b] ^ 1)
        self.copy_scale(spare_raw, L.cum[0])                                    # logarithms into a per-node slot
        self.get_scale(L.cum[1])
        self.get_scale(spare_raw)
        self.update_matrices(nodes=self.branches()[:4])
        self.update_partials(mode="read", nodes=nodes)
        self.reset_scale(L.cum[0])
        self.accumulate(L.cum[0], [L.scale(n, 0) for n in nodes if self.sdef[L.scale(n, 0)] == "raw"] + [L.cum[1]])
        self.root_call("root", cum=True)
        self.get_scale(L.cum[0])

    def motif_i(self):
        """convolve into a slot that the last list used as a branch matrix, then that list again"""
        L = self.L
        nodes = self.post_order(self.internal)
        self.update_partials(mode="none", nodes=nodes)
        self.root_call("root", cum=False)
        child = self.left[nodes[-1]]
        self.triples("convolveTransitionMatrices", result=L.matrix(child, self.mcur[child]))
        self.repeat_list()
        self.root_call("root", cum=False)
        self.get_sites()

    # ---- the weighted draw -----------------------------------------------------------------------------------------------------
    def table(self):
        rng = self.rng
        return [
            (2, "setEigenDecomposition", lambda: self.set_eigen(int(rng.integers(2)), same=rng.random() < 0.25)),
            (1, "setCategoryRates", lambda: self.set_rates(0, indexed=False)),
            (1, "setCategoryRatesWithIndex", lambda: self.set_rates(int(rng.integers(2)), indexed=True)),
            (1, "setCategoryWeights", lambda: self.set_weights(int(rng.integers(2)))),
            (1, "setStateFrequencies", lambda: self.set_frequencies(int(rng.integers(2)))),
            (1, "setPatternWeights", self.set_pattern_weights),
            (2, "setTipStates", lambda: self.resend_tip_of_kind("compact")),
            (2, "setTipPartials", lambda: self.resend_tip_of_kind("partials")),
            (2, "setPartials", self.set_partials),
            (0.5, "compactToPartials", self.compact_to_partials),
            (1.5, "setTipEmission", self.set_tip_emission),
            (4, "updateTransitionMatrices", lambda: self.update_matrices(slots=self.L.spare[:int(rng.integers(1, 3))] if rng.random() < 0.2 else None)),
            (2, "updateTransitionMatricesWithMultipleModels", lambda: self.update_matrices(multiple=True)),
            (2, "setTransitionMatrix", self.set_transition_matrix),
            (2, "convolveTransitionMatrices", lambda: self.triples("convolveTransitionMatrices")),
            (2, "addTransitionMatrices", lambda: self.triples("addTransitionMatrices")),
            (1.5, "transposeTransitionMatrices", self.transpose),
            (3, "getTransitionMatrix", self.get_matrix),
            (3, "updatePartials:none", lambda: self.update_partials(mode="none", again=rng.random() < 0.15)),
            (3, "updatePartials:write", lambda: self.update_partials(mode="write", cum_on_call=False, again=rng.random() < 0.15)),
            (3, "updatePartials:read", lambda: self.update_partials(mode="read")),
            (2, "updatePartials:cumulative", lambda: self.update_partials(mode="write", cum_on_call=True)),
            (1, "waitForPartials", self.wait_for_partials),
            (2, "resetScaleFactors", self.reset_scale),
            (3, "accumulateScaleFactors", self.accumulate),
            (2, "removeScaleFactors", self.remove),
            (2, "copyScaleFactors", self.copy_scale),
            (3, "getLogScaleFactors", self.get_scale),
            (4, "calculateRootLogLikelihoods:root", lambda: self.root_call("root", cum=False)),
            (2, "calculateRootLogLikelihoods:other", lambda: self.root_call("other", cum=False)),
            (3, "calculateRootLogLikelihoods:cumulative", lambda: self.root_call(cum=True)),
            (3, "getSiteLogLikelihoods", self.get_sites),
            (3, "getPartials", lambda: self.get_partials(scaled=False)),
            (2, "getPartials:scaled", lambda: self.get_partials(scaled=True)),
            (2, "getPartialsBatch", self.get_partials_batch),
            (1.5, "setRootPrePartials", self.set_root_pre),
            (3, "updatePrePartials", self.update_pre),
            (1, "setDifferentialMatrix", lambda: self.set_differential(int(rng.integers(2)))),
            (3, "calculateEdgeDifferentials", self.edge_differentials),
            (1.5, "calculateCrossProductDifferentials", self.cross_products),
            (2, "getPartials:pre", self.get_pre_partials),
        ] + ([
            (4, "sampleAncestralStates", self.sample_ancestral),
            (4, "sampleMarkovJumps", self.sample_jumps),
            (3, "simulateSequences", self.simulate),
            (4, "nodeHeightDerivatives", self.node_height),
            (4, "updateDifferentialMatrices", self.update_differential),
            (3, "setReversibleModels", self.set_reversible),
            (3, "getEigenDecomposition", self.get_eigen),
        ] if self.profile == "extensions" else []) + ([
            (3, "setReversibleModels", self.set_reversible),
            (4, "updateTransitionMatricesFromGenerators", self.generator_matrices),
            (4, "updateTransitionMatricesWithEpochs", self.epoch_matrices),
            (4, "nodePosteriors", self.node_posteriors),
            (4, "nodePatternLikelihoods", self.node_pattern),
            (4, "placementScores", self.placement),
        ] if self.profile == "queries" else [])

    def draw(self, lacking_only=False):
        """one drawn action: one this sequence has not made yet while there is any (every sequence makes every action), else by weight
        (extension profile: half of the draws by weight all the same — what is still lacking at the end is made then)"""
        rng = self.rng
        table = [t for t in self.table() if t[1] in actions_for(self.L.S, self.profile)]
        missing = [t for t in table if t[1] in self.lacking()]
        if missing and (self.profile == "base" or lacking_only or rng.random() < 0.5):
            t = missing[int(rng.integers(len(missing)))]
            if t[2]() is False:
                if t[1] == "removeScaleFactors":
                    c = self.L.cum[0]
                    self.reset_scale(c)
                    if self.accumulate(c) is not False and self.remove() is not False:
                        return
                self.gave_up.add(t[1])                       # (no compact tip left to turn into a partials tip: it has happened)
            return
        w = np.array([t[0] for t in table], dtype=float)
        while True:
            k = int(rng.choice(len(table), p=w / w.sum()))
            if table[k][2]() is not False:
                return

    def lacking(self):
        """the actions this sequence has not made yet (extension profile, whose shapes have fewer seeds: not twice yet) and has not
        given up on"""
        need = 2 if self.profile != "base" else 1
        count = {}
        for r in self.rec[self.prelude_end:]:
            count[r["action"]] = count.get(r["action"], 0) + 1
        return [a for a in actions_for(self.L.S, self.profile) if count.get(a, 0) < need and a not in self.gave_up]

    def run(self):
        self.prelude()
        start = len(self.rec)
        motifs = motifs_for(self.profile)
        order = [motifs[k] for k in self.rng.permutation(len(motifs))]
        budget = self.length
        # the motifs at seeded positions: between two of them a seeded share of the calls the weighted draw fills
        gaps = self.rng.dirichlet(np.full(len(order) + 1, 2.0))
        for k, letter in enumerate(order):
            self.motif, self.variant = letter, None
            getattr(self, "motif_" + letter)()
            self.motif = self.variant = None
        motif_calls = len(self.rec) - start
        # (the 13 motifs of the extension profile and the 14 of the query profile use the budget up)
        fill = max({"base": 4, "extensions": 60}.get(self.profile, QUERY_FILL), budget - motif_calls)
        # (the motifs were generated to learn their size; generate again with the filler between them)
        return motif_calls, [int(round(g * fill)) for g in gaps], order


def generate(shape, seed, length=100, profile="base"):
    """-> records.  `length`: calls after the set-up prelude, motifs included (at least what the motifs and a few drawn calls between
    them need).  `profile`: "base", or "extensions" with ACTIONS_EXT and motifs (j)-(m) in the draw as well."""
    probe = Generator(shape, seed, length, profile)
    _, gaps, order = probe.run()
    g = Generator(shape, seed, length, profile)
    g.rng = np.random.default_rng([seed, g.L.S, g.L.C, g.L.T, g.L.P, 1])
    g.prelude()
    for k, letter in enumerate(order):
        target = len(g.rec) + gaps[k]
        while len(g.rec) < target:
            g.draw()
        g.motif, g.variant = letter, None
        getattr(g, "motif_" + letter)()
        g.motif = g.variant = None
    target = len(g.rec) + gaps[-1]
    while len(g.rec) < target:
        g.draw()
    for _ in range(2 * len(ACTIONS) * (2 if profile != "base" else 1)):          # whatever action the sequence still lacks
        if not g.lacking():
            break
        g.draw(lacking_only=True)
    return g.rec


def dump(path, shape, seed, records, profile="base"):
    """(a base sequence's file is what it always was; another profile's name travels in it)"""
    d = {"shape": list(shape), "seed": seed, "records": records}
    if profile != "base":
        d["profile"] = profile
    with open(path, "w") as f:
        json.dump(d, f)


def load(path, with_profile=False):
    with open(path) as f:
        d = json.load(f)
    out = (tuple(d["shape"]), d["seed"], d["records"])
    return out + (d.get("profile", "base"),) if with_profile else out


# ---- running records on a binding object ---------------------------------------------------------------------------------------

def create(shape, factory, **kw):
    """factory: beagle.Beagle (or a callable with its signature) -> the instance of this shape's layout"""
    return factory(*Layout(shape).create_args(), **kw)


def expanded_emission(S, P, codes, table, extra):
    """[P][S] partials of a tip with an emission table: row codes[p], all ones for a code outside the table; 4 states: the sequence-error
    model restated pattern by pattern (tests/tip_models_reference.py)"""
    codes, table = np.asarray(codes), np.asarray(table, dtype=float)
    if S == 4 and "base_rate" in extra:
        import tip_models_reference
        return tip_models_reference.sequence_error_partials(codes, "all", extra["base_rate"], None, 0.0, False, 0.0, False)
    out = np.ones((P, S))
    ok = (codes >= 0) & (codes < len(table))
    out[ok] = table[codes[ok]]
    return out


def sent(b):
    """What the host has handed to the instance behind `b` and a restatement needs again: eigen systems, category rates and weights,
    frequencies, pattern weights, compact tip states — kept on the binding object by ``execute``, on every side alike."""
    if not hasattr(b, "_sent"):
        b._sent = {"eigen": {}, "rates": {}, "weights": {}, "freqs": {}, "pattern_weights": None, "tips": {}}
    return b._sent


def remember(b, m, a):
    S = b.stateCount
    if m == "setEigenDecomposition":
        sent(b)["eigen"][a[0]] = (np.array(a[1], dtype=float).reshape(S, S), np.array(a[2], dtype=float).reshape(S, S), np.array(a[3], dtype=float))
    elif m == "setCategoryRates":
        sent(b)["rates"][0] = np.array(a[0], dtype=float)
    elif m == "setCategoryRatesWithIndex":
        sent(b)["rates"][a[0]] = np.array(a[1], dtype=float)
    elif m == "setCategoryWeights":
        sent(b)["weights"][a[0]] = np.array(a[1], dtype=float)
    elif m == "setStateFrequencies":
        sent(b)["freqs"][a[0]] = np.array(a[1], dtype=float)
    elif m == "setPatternWeights":
        sent(b)["pattern_weights"] = np.array(a[0], dtype=float)
    elif m == "setTipStates":
        sent(b)["tips"][a[0]] = np.array(a[1], dtype=np.int32)
    elif m == "setReversibleModels":
        for slot, upper, pi in zip(*a):
            sent(b)["eigen"][slot] = decompose_reversible(symmetric_rates(upper, S), np.array(pi, dtype=float))[:3]


def packed_eigen(u, ui, lam):
    return np.concatenate([np.ravel(u), np.ravel(ui), np.ravel(lam)])


def execute_extension(b, rec, side, info):
    """One call of ACTIONS_EXT or ACTIONS_Q (the latter: the module docstring's paragraph on the "queries" profile; nodePosteriors reads
    its operands back on every side, the other four on the oracle's side only).  side "oracle": made from the oracle's own calls and the numpy restatements the extensions' tests use
    (updateDifferentialMatrices: differential_matrices_reference.slot, then setDifferentialMatrix; setReversibleModels: numpy's eigh
    of the symmetric form, then setEigenDecomposition; the five calls that return values: ancestral_reference.sample,
    simulate_reference.simulate, node_height_reference.row_derivatives, markov_jumps_reference.tables and site_values over the
    oracle's getPartials and getTransitionMatrix and the tip states it was sent; getEigenDecomposition: what was sent).

    The two samplers and the Markov-jump call: right after the call EVERY side reads back what the restatement needs from its own
    instance (so the three stay in step, and the call itself ran in whatever deferred state the sequence left) and restates the
    draw; read "exact" is the number of bytes in which the device's states and categories differ from that restatement (0 on the
    oracle, which has nothing else).  info["undecided"]: the patterns (sites) on which some draw of the restatement lies next to a
    boundary; info["device"] (oracle side): the engine's reads of the same record — the Markov-jump values are restated for the
    device's own states and categories, so that a legitimately different draw does not show as a numeric error."""
    import ancestral_reference
    import differential_matrices_reference
    import markov_jumps_reference
    import node_height_reference
    import simulate_reference
    m, a = rec["m"], rec["a"]
    S, C, P = b.stateCount, b.categoryCount, b.patternCount
    have = sent(b)
    cache = {}

    def matrix_of(slot):
        if slot not in cache:
            cache[slot] = np.asarray(b.getTransitionMatrix(slot), dtype=float).reshape(C, S, S)
        return cache[slot]

    def tip_states_of(t):                                    # (the oracle has no getTipStates: a compact tip's states are what it was sent)
        return b.getTipStates(t) if b.lib.has("GetTipStates") else have["tips"][t]

    def post_of(buf, compact):
        if buf in compact:
            return node_height_reference.expand_states(tip_states_of(buf), S, C)
        return b.getPartials(buf, NONE)

    reads = []
    if m in ("sampleAncestralStates", "sampleMarkovJumps"):
        if m == "sampleAncestralStates":
            rows, w, f, seed, use_map, compact = a
        else:
            rows, times, e, r, w, f, registers, flags, seed, use_map, compact = a
        st = ca = res = None
        if side != "oracle" and m == "sampleAncestralStates":
            st, ca = b.sampleAncestralStates(rows, w, f, seed, map=use_map)
        elif side != "oracle":
            res = b.sampleMarkovJumps(rows, times, None, e, r, w, f, registers, flags, seed, map=use_map, states=True, jumps=True)
            st, ca = res["states"], res["categories"]
        und = np.zeros(P, dtype=bool)
        rs, rc, bad = ancestral_reference.sample(rows, b.getPartials, matrix_of, tip_states_of, lambda x: x in compact, have["weights"][w],
                                                 have["freqs"][f], seed, use_map=use_map, undecided=und)
        if bad:
            return -8, []
        info["undecided"] = und
        if side == "oracle":
            st, ca = rs, rc
        reads += [("states", st), ("cats", ca), ("exact", np.array([float(np.sum(st != rs) + np.sum(ca != rc))]))]
        if m == "sampleMarkovJumps":
            if side == "oracle":
                dev = info.get("device")
                vs, vc = (dev[0][1], dev[1][1]) if dev else (rs, rc)
                u, ui, lam = have["eigen"][e]
                mats = np.stack([np.zeros((C, S, S))] + [matrix_of(row[1]) for row in rows[1:]])
                kinds = ["rewards" if fl & JUMPS_REWARDS else "counts" for fl in flags]
                cond = markov_jumps_reference.tables(u, ui, lam, [np.array(x, dtype=float) for x in registers], kinds,
                                                     [bool(fl & JUMPS_SCALE_BY_TIME) for fl in flags], times, None, have["rates"][r], mats)
                vals, tot, row_tot = markov_jumps_reference.site_values(cond, np.asarray(vs), [row[2] for row in rows], vc)
            else:
                vals, tot, row_tot = res["jumps"], res["pattern_totals"], res["row_totals"]
            reads += [("jumps", vals), ("jumps", tot), ("jumps", row_tot)]
    elif m == "simulateSequences":
        rows, sites, w, f, seed, root, cats = a
        st = ca = None
        if side != "oracle":
            st, ca = b.simulateSequences(rows, sites, w, f, seed, root_states=root, rate_categories=cats)
        und = np.zeros(sites, dtype=bool)
        rs, rc, bad = simulate_reference.simulate(rows, matrix_of, have["weights"][w], have["freqs"][f], seed, sites, root_states=root,
                                                  rate_categories=cats, undecided=und)
        if bad:
            return -8, []
        info["undecided"] = und
        if side == "oracle":
            st, ca = rs, rc
        reads += [("states", st), ("cats", ca), ("exact", np.array([float(np.sum(st != rs) + np.sum(ca != rc))]))]
    elif m == "nodeHeightDerivatives":
        rows, rates, w, first, second, compact = a
        if side == "oracle":
            o1, o2 = node_height_reference.row_derivatives(rows, rates, lambda buf: post_of(buf, compact), lambda buf: b.getPartials(buf, NONE),
                                                           matrix_of, have["weights"][w], have["pattern_weights"], first, second)
            if not all(np.isfinite(x).all() for x in (o1, o2) if x is not None):
                return -8, []
        else:
            o1, o2 = b.nodeHeightDerivatives(rows, rates, w, first=first, second=second)
        reads += [("deriv", x) for x in (o1, o2) if x is not None]
    elif m == "updateDifferentialMatrices":
        e, r, dqs, d, slots, lengths, mode = a
        if side == "oracle":
            for k, slot in enumerate(slots):
                u, ui, lam = have["eigen"][e[k]]
                D = differential_matrices_reference.slot(u, ui, lam, np.array(dqs[d[k]], dtype=float), lengths[k], have["rates"][r[k]], mode)
                b.setDifferentialMatrix(slot, D.ravel())
        else:
            b.updateDifferentialMatrices(e, r, dqs, d, slots, lengths, len(slots), mode)
    elif m == "setReversibleModels":
        if side == "oracle":
            for slot, upper, pi in zip(*a):
                u, ui, lam = decompose_reversible(symmetric_rates(upper, S), np.array(pi, dtype=float))[:3]
                b.setEigenDecomposition(slot, u.ravel(), ui.ravel(), lam)
        else:
            b.setReversibleModels(*a)
    elif m == "getEigenDecomposition":
        reads.append(("eigen", packed_eigen(*(have["eigen"][a[0]] if side == "oracle" else b.getEigenDecomposition(a[0])))))
    elif m == "updateTransitionMatricesFromGenerators":
        gens, g, r, slots, lengths, count = a
        if side == "oracle":
            import generator_matrices_reference
            for k, slot in enumerate(slots):
                q = np.array(gens[g[k]], dtype=float)
                mat = [generator_matrices_reference.yardstick(q, float(np.float64(lengths[k]) * np.float64(rate))) for rate in have["rates"][r[k]]]
                b.setTransitionMatrix(slot, np.stack(mat).astype(np.float64).ravel(), 1.0)
        else:
            b.updateTransitionMatricesFromGenerators(gens, g, r, slots, lengths, count)
    elif m == "updateTransitionMatricesWithEpochs":
        offsets, eig, seg, rate, slots, count = a
        if side == "oracle":
            import epoch_matrices_reference
            systems = {k: types.SimpleNamespace(evec=e[0], ievc=e[1], evals=e[2]) for k, e in have["eigen"].items()}
            for k, slot in enumerate(slots):
                entry = [(eig[j], seg[j]) for j in range(offsets[k], offsets[k + 1])]
                if len(entry) == 1:                          # (exactly what the oracle's own call leaves in the slot)
                    b.updateTransitionMatricesWithMultipleModels([entry[0][0]], [rate[k]], [slot], None, None, [entry[0][1]], 1)
                else:
                    mat = [epoch_matrices_reference.yardstick(systems, entry, x) for x in have["rates"][rate[k]]]
                    b.setTransitionMatrix(slot, np.stack(mat).astype(np.float64).ravel(), 1.0)
        else:
            b.updateTransitionMatricesWithEpochs(offsets, eig, seg, rate, slots, count)
    elif m == "nodePosteriors":
        import node_posteriors_reference
        rows, w, full, use_map, totals, cats, compact = a
        out = None
        if side != "oracle":
            out, rc = b.nodePosteriors(rows, w, full=full, map=use_map, totals=totals, categories=cats)
            if rc:
                return rc, []
        pre = np.stack([b.getPartials(row[1], NONE) for row in rows])
        post = np.stack([post_of(row[0], compact) for row in rows])
        ref, _, bad = node_posteriors_reference.posteriors(pre, post, have["weights"][w])
        if side == "oracle":
            if bad.any():
                return -8, []
            out = {"posteriors": ref, "categories": node_posteriors_reference.category_posteriors(pre[0], post[0], have["weights"][w])}
            out["map_states"], out["map_probabilities"] = node_posteriors_reference.map_states(ref)
            if totals:
                out["totals"] = np.asarray(node_posteriors_reference.state_totals(ref, have["pattern_weights"]), dtype=np.float64)
            if use_map:
                top = np.sort(ref, axis=2)[:, :, -2:]
                info["undecided"] = np.any(top[:, :, 1] - top[:, :, 0] <= MAP_MARGIN, axis=0)
        if full:
            reads += [("posterior", out["posteriors"]),
                      ("exact", np.array([0.0 if side == "oracle" else float(np.sum(out["posteriors"] != ref))]))]
        if use_map:
            reads += [("states", out["map_states"]), ("posterior", out["map_probabilities"])]
        if totals:
            reads.append(("posterior", out["totals"] / float(np.sum(have["pattern_weights"]))))
        if cats:
            reads.append(("posterior", out["categories"]))
    elif m == "nodePatternLikelihoods":
        rows, logw, death, w, f, node_terms, compact = a
        if side != "oracle":
            logp, terms, total, rc = b.nodePatternLikelihoods(rows, logw, death, w, f, node_terms=node_terms)
            if rc:
                return rc, []
        else:
            import stochastic_dollo_reference as sd
            # the restatement numbers tips first: the tip rows in list order, then the internal rows in list order (still post-order)
            tip_rows = [k for k, row in enumerate(rows) if row[2] < 0]
            number = {k: i for i, k in enumerate(tip_rows + [k for k, row in enumerate(rows) if row[2] >= 0])}
            R, T = len(rows), len(tip_rows)
            left, right = np.full(R, NONE), np.full(R, NONE)
            partials, own = [None] * R, np.zeros((R, P))
            states, as_partials = np.zeros((T, P), dtype=np.int64), {}
            weights_by_node = np.zeros(R)
            for k, row in enumerate(rows):
                n = number[k]
                partials[n] = post_of(row[0], compact)
                weights_by_node[n] = logw[k]
                if row[2] < 0 and row[0] in compact:
                    states[n] = tip_states_of(row[0])
                elif row[2] < 0:
                    as_partials[n] = partials[n][0]
                else:
                    left[n], right[n] = number[row[2]], number[row[3]]
                    if row[1] != NONE:
                        own[n] = b.getLogScaleFactors(row[1])
            tree = types.SimpleNamespace(node_count=R, tip_count=T, left=left, right=right, postorder=lambda: range(R))
            _, incl = sd.inclusion(tree, sd.tip_extant(states, as_partials, S, death))
            by_node, _ = sd.log_terms(tree, [number[k] for k in range(R)], np.stack(partials), own, incl, have["freqs"][f], have["weights"][w],
                                      weights_by_node, np.float64)
            logp, terms = sd.log_cum(by_node, np.float64), by_node
            total = float(np.sum(have["pattern_weights"] * logp))
            if not np.isfinite(total):
                return -8, []
        reads.append(("logval", logp))
        if node_terms:                                       # (a row that is not included has the term -inf: compared as a mask)
            there = np.asarray(terms) != -np.inf
            reads += [("states", there.astype(np.uint8)), ("logval", np.where(there, terms, 0.0))]
        reads.append(("sum", np.array([total])))
    elif m == "placementScores":
        rows, patterns, codes, table, w, log_table, compact = a
        if side != "oracle":
            scores, logs, rc = b.placementScores(rows, patterns, codes, table, w, log_table=log_table)
            if rc:
                return rc, []
        else:
            import placement_reference
            operands = [(b.getPartials(pre, NONE), None if sib == NONE else post_of(sib, compact), None if sib == NONE else matrix_of(m_sib),
                         post_of(child, compact), None if m_up == NONE else matrix_of(m_up), matrix_of(m_low), matrix_of(m_pend))
                        for pre, sib, m_sib, child, m_up, m_low, m_pend in rows]
            logs = placement_reference.log_tables(operands, have["weights"][w], np.array(table, dtype=float).reshape(-1, S))
            scores = placement_reference.scores(logs, patterns, codes)
            if not (np.isfinite(logs).all() and np.isfinite(scores).all()):
                return -8, []
        reads += ([("logval", logs)] if log_table else []) + [("logval", scores)]
    else:
        raise ValueError(m)
    return 0, reads


def execute(b, rec, side="engine", info=None):
    """One call.  side "oracle": the three calls the oracle has no entry point for are made from its own ones (setTipEmission: setTipPartials
    of the expanded table; addTransitionMatrices: the numpy sum of its two matrices, then setTransitionMatrix; getPartialsBatch: single
    getPartials calls; waitForPartials: nothing to wait for), and so are those of ACTIONS_EXT (``execute_extension``; `info`: a dict
    it reads "device" from and writes "undecided" into).  -> (return code, [(kind, array), ...])"""
    m, a = rec["m"], rec["a"]
    reads = []
    try:
        if m in ACTIONS_EXT or m in ACTIONS_Q:
            rc, reads = execute_extension(b, rec, side, {} if info is None else info)
            if rc:
                return rc, []
        elif m == "calculateRootLogLikelihoods":
            out = [0.0]
            b.calculateRootLogLikelihoods(a[0], a[1], a[2], a[3], a[4], out)
            reads.append(("sum", np.array(out)))
        elif m == "getSiteLogLikelihoods":
            reads.append(("site", b.getSiteLogLikelihoods()))
        elif m == "getLogScaleFactors":
            reads.append(("scale", b.getLogScaleFactors(a[0])))
        elif m == "getTransitionMatrix":
            reads.append(("matrix", b.getTransitionMatrix(a[0])))
        elif m == "getPartials":
            reads.append(("partials", b.getPartials(a[0], a[1])))
        elif m == "getPartialsBatch":
            if side == "oracle":
                for k, buf in enumerate(a[0]):
                    reads.append(("partials", b.getPartials(buf, NONE if a[1] is None else a[1][k])))
            else:
                reads += [("partials", p) for p in b.getPartialsBatch(a[0], a[1])]
        elif m == "calculateEdgeDifferentials":
            s1, s2, per = b.calculateEdgeDifferentials(a[0], a[1], a[2], a[3], a[4], want_per_pattern=a[5][0], want_squared=a[5][1])
            reads += [("deriv", x) for x in (s1, s2, per) if x is not None]
        elif m == "calculateCrossProductDifferentials":
            reads.append(("deriv", b.calculateCrossProductDifferentials(*a)))
        elif m == "setTipEmission":
            if side == "oracle":
                b.setTipPartials(a[0], expanded_emission(b.stateCount, b.patternCount, a[1], a[2], a[3]))
            else:
                b.setTipEmission(a[0], a[1], a[2])
        elif m == "addTransitionMatrices" and side == "oracle":
            for f, s, r in zip(*a[:3]):
                b.setTransitionMatrix(r, b.getTransitionMatrix(f) + b.getTransitionMatrix(s), 1.0)
        elif m == "waitForPartials" and side == "oracle":
            pass
        else:
            getattr(b, m)(*a)
    except Exception as e:                                   # beagle.BeagleException
        if not hasattr(e, "code"):
            raise
        return e.code, []
    remember(b, m, a)
    return 0, reads


def deviation(kind, got, want, undecided=None):
    """The error of a read, normalised so that the project's bound is 1e-10 for every kind: sums and site values relative; log scale
    factors relative, against 1 where the value is smaller (a factor near 1 has a logarithm near 0); node partials against each
    pattern's largest entry (tests/test_gpu_parity.py test_engine_matches_oracle), a transition matrix likewise against the largest entry
    of each category's matrix; derivative outputs against max(1, largest value) (tests/test_gpu_gradients.py), and so the node-height
    derivatives and the Markov-jump values (tests/test_gpu_gradients.py ``close``).  An eigen system (U, U^-1, lambda packed) is not
    unique: the larger of |U diag(lambda) U^-1 - Q| / max |Q|, Q the other side's reconstruction, and |U U^-1 - I|.  States and
    categories of a draw: the number of entries that differ on the patterns (last axis) outside `undecided`; "exact": the number of
    bytes by which a side differed from the restatement over its own reads.  Any count above 0 is above the bound."""
    if kind in ("states", "cats"):
        got, want = np.asarray(got), np.asarray(want)
        if got.shape != want.shape:
            return float("inf")
        differ = got != want
        if undecided is not None:
            differ = differ & ~np.asarray(undecided, dtype=bool)
        return float(np.sum(differ))
    got, want = np.asarray(got, dtype=float), np.asarray(want, dtype=float)
    if got.shape != want.shape:
        return float("inf")
    if not (np.isfinite(got).all() and np.isfinite(want).all()):
        return float("nan")
    if kind in ("sum", "site"):
        return float(np.max(np.abs(got - want) / np.maximum(np.abs(want), 1e-300)))
    if kind in ("scale", "logval"):
        return float(np.max(np.abs(got - want) / np.maximum(np.abs(want), 1.0)))
    if kind == "posterior":
        return float(np.max(np.abs(got - want)))
    if kind == "partials":
        scale = np.maximum(np.abs(want).max(axis=(0, 2), keepdims=True), 1e-300)
        return float(np.max(np.abs(got - want) / scale))
    if kind == "matrix":
        scale = np.maximum(np.abs(want).max(axis=(1, 2), keepdims=True), 1e-300)
        return float(np.max(np.abs(got - want) / scale))
    if kind in ("deriv", "jumps"):
        return float(np.max(np.abs(got - want)) / max(1.0, float(np.max(np.abs(want)))))
    if kind == "exact":
        return float(np.max(np.abs(got - want)) + np.max(np.abs(got)))
    if kind == "eigen":
        S = int(round((np.sqrt(1.0 + 8.0 * got.size) - 1.0) / 4.0))
        (ug, ig, lg), (uw, iw, lw) = ((x[:S * S].reshape(S, S), x[S * S:2 * S * S].reshape(S, S), x[2 * S * S:]) for x in (got, want))
        q = (uw * lw[None, :]) @ iw
        return float(max(np.max(np.abs((ug * lg[None, :]) @ ig - q)) / np.max(np.abs(q)), np.max(np.abs(ug @ ig - np.eye(S)))))
    raise ValueError(kind)


def describe(rec):
    def short(x):
        s = json.dumps(x)
        return s if len(s) <= 60 else s[:57] + "..."
    return "%s(%s)" % (rec["m"], ", ".join(short(x) for x in rec["a"]))


def replay(path, upto=None, out=print):
    """Engine and oracle side by side up to step `upto` (inclusive); prints the first diverging read and stops at the first non-zero
    return code or exception.  -> the step it stopped at, or None."""
    import os
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    for p in (here, os.path.dirname(here)):
        if p not in sys.path:
            sys.path.insert(0, p)
    import beast_mcmc_amd as bm
    import helpers
    shape, seed, records = load(path)
    eng = create(shape, bm.beagle.Beagle)
    ora = create(shape, bm.beagle.Beagle, library=helpers.oracle_library())
    stopped = None
    try:
        for step, rec in enumerate(records if upto is None else records[:upto + 1]):
            rc_e, reads_e = execute(eng, rec, "engine")
            info = {"device": reads_e}
            rc_o, reads_o = execute(ora, rec, "oracle", info)
            if rc_e or rc_o:
                out("step %d %s: return codes engine %d, oracle %d" % (step, describe(rec), rc_e, rc_o))
                stopped = step
                break
            worst = max([deviation(k, g, w, undecided=info.get("undecided")) for (k, g), (_, w) in zip(reads_e, reads_o)] + [0.0],
                        key=lambda x: (x != x, x))
            if not worst <= BOUND:
                out("step %d %s: first diverging read, deviation %.3e (bound %.0e)" % (step, describe(rec), worst, BOUND))
                stopped = step
                break
        else:
            out("shape %s seed %d: no read diverges in %d steps" % (shape, seed, step + 1))
    finally:
        eng.finalize()
        ora.finalize()
    return stopped


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser(description="replay a recorded call sequence on the engine and the oracle")
    ap.add_argument("--replay", required=True, metavar="FILE")
    ap.add_argument("--upto", type=int, default=None, metavar="N")
    args = ap.parse_args()
    replay(args.replay, args.upto)
