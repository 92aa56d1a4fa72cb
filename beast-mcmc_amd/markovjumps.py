"""Markov-jump counts and rewards on the device: the caller-side mirror of
``dr.evomodel.treelikelihood.MarkovJumpsBeagleTreeLikelihood`` (src/dr/evomodel/treelikelihood/MarkovJumpsBeagleTreeLikelihood.java)
with ``useUniformization = false`` (expectations) and ``true`` (sampled histories, complete histories included).

The reference extends the ancestral sampler: inside ``traverseSample`` its ``hookCalculation`` (:429-567) turns every branch's drawn
(parent, child) state pair into the expected number of registered substitutions, or the expected reward, on that branch.  Here the
draw and all of that are ONE engine call (include/beagle_mi355.h ``beagleMi355SampleMarkovJumps``); this class only builds the node
list (``AncestralStateSampler.node_list``), the branch times and rates, and the registers, and hands the results back per tree node.

Sample after ``getLogLikelihood``, as for the ancestral sampler: the states are drawn from the partials of the last evaluation and
the branch quantities are the host driver's current ones.  ``marginal_rate`` / ``unconditioned`` read the substitution and site
models last set through ``set_substitution_model`` / ``set_site_model``.
"""
import numpy as np

from .ancestral import AncestralStateSampler

JUMPS_REWARDS = 1
JUMPS_SCALE_BY_TIME = 2


class MarkovJumpsSampler:
    """Registers of a ``treelikelihood.BeagleTreeLikelihood`` (the C++ caller stand-in) and one call that samples them all."""

    def __init__(self, tree_likelihood):
        self.tl = tree_likelihood
        self.ancestral = AncestralStateSampler(tree_likelihood)
        self.beagle = self.ancestral.beagle
        self.tags, self.kinds, self.scale_by_time, self.registers = [], [], [], []

    def add_register(self, tag, values, kind="counts", scale_by_time=False):
        """``values``: an S x S registration matrix for counts (its diagonal is ignored: setRegistration), an S-vector of rewards
        (MarkovJumpsSubstitutionModel.setRegistration, REWARDS).  Returns the register's index k."""
        S = self.tl.state_count
        if kind == "counts":
            R = np.array(values, dtype=np.float64).reshape(S, S)
            np.fill_diagonal(R, 0.0)
        elif kind == "rewards":
            R = np.diag(np.asarray(values, dtype=np.float64).reshape(S))
        else:
            raise ValueError("kind must be 'counts' or 'rewards'")
        if len(self.registers) >= 8:
            raise ValueError("at most 8 registers")
        self.tags.append(tag)
        self.kinds.append(kind)
        self.scale_by_time.append(bool(scale_by_time))
        self.registers.append(R)
        return len(self.registers) - 1

    def flags(self):
        return np.array([(JUMPS_REWARDS if kind == "rewards" else 0) | (JUMPS_SCALE_BY_TIME if sc else 0)
                         for kind, sc in zip(self.kinds, self.scale_by_time)], dtype=np.int32)

    def branch_times(self, order):
        """(times, rates) per row of the node list, row 0 (the root) 0 and 1, read from the host driver (the Python tree's heights
        are not kept current after set_node_height)."""
        times, rates = np.zeros(len(order)), np.ones(len(order))
        for r, n in enumerate(order):
            if r > 0:
                times[r], rates[r] = self.tl.node_branch_time(int(n))
        return times, rates

    def node_heights(self, order):
        """height per row of the node list, read from the host driver (the Python tree's heights go stale)."""
        return np.array([self.tl.node_height(int(n)) for n in order], dtype=np.float64)

    def infinitesimal_matrix(self):
        """Q from the driver's eigen system (as marginal_rate forms it)."""
        eig = self.tl.eig
        return (eig.evec * eig.evals[None, :]) @ eig.ievc

    def sample(self, seed, map=False, per_site=False, states=False, category_weights_index=0, state_frequencies_index=0,
               category_rates_index=0, uniformization=False, simulants=1, history=False, infinitesimal_matrix=None):
        """With ``uniformization``: sampled histories (include/beagle_mi355.h beagleMi355SampleMarkovJumpsUniformized), the mean
        over ``simulants``; ``infinitesimal_matrix`` Q (default: from the driver's eigen system); ``history`` (one simulant) adds
        "event_counts" [nodeCount, P] by node and the event list "events" (rows as tree nodes), read by ``histories``.
        -> dict indexed by tree node number:
          "branch"  [K, nodeCount]  per-branch totals over patterns (the <tag>_sum trait; the root's row is 0)
          "pattern" [K, P]          per-pattern totals over branches (the c_<tag>[p] columns)
          "tree"    [K]             the sum of "branch" (the register-parameter trait)
          "site"    [K, nodeCount, P]  per branch and pattern (the <tag>_base trait), when ``per_site``
          "states"  uint8 [nodeCount, P], "categories" int32 [P], when ``states``."""
        if not self.registers:
            raise ValueError("no register")
        rows, order = self.ancestral.node_list()
        times, rates = self.branch_times(order)
        if uniformization:
            Q = self.infinitesimal_matrix() if infinitesimal_matrix is None else np.asarray(infinitesimal_matrix, dtype=np.float64)
            heights = self.node_heights(order) if history else None
            res = self.beagle.sampleMarkovJumpsUniformized(rows, times, rates, heights, Q, category_rates_index, category_weights_index,
                                                           state_frequencies_index, np.stack(self.registers), self.flags(), seed,
                                                           simulants=simulants, map=map, states=states, jumps=per_site,
                                                           history=history)
        else:
            res = self.beagle.sampleMarkovJumps(rows, times, rates, self.tl.eigen_index(), category_rates_index, category_weights_index,
                                                state_frequencies_index, np.stack(self.registers), self.flags(), seed, map=map,
                                                states=states, jumps=per_site)
        out = {"pattern": res["pattern_totals"]}
        branch = np.empty_like(res["row_totals"])
        branch[:, order] = res["row_totals"]
        out["branch"] = branch
        out["tree"] = res["row_totals"].sum(axis=1)
        self.categories = None
        if per_site:
            site = np.empty_like(res["jumps"])
            site[:, order] = res["jumps"]
            out["site"] = site
        if uniformization:
            out["fallbacks"] = res["fallbacks"]
        if history:
            counts = np.empty_like(res["event_counts"])
            counts[order] = res["event_counts"]
            out["event_counts"] = counts
            row_of = np.repeat(np.tile(np.arange(len(order)), res["event_counts"].shape[1]), res["event_counts"].T.ravel())
            pattern_of = np.repeat(np.arange(res["event_counts"].shape[1]), res["event_counts"].sum(axis=0))
            out["events"] = {"node": np.asarray(order)[row_of], "pattern": pattern_of, "height": res["event_heights"],
                             "states": res["event_states"]}
        if states:
            st = np.empty_like(res["states"])
            st[order] = res["states"]
            out["states"] = st
            out["categories"] = res["categories"]
            self.categories = res["categories"]
        return out

    def marginal_rate(self, k):
        """MarkovJumpsSubstitutionModel.getMarginalRate: sum_i pi_i sum_j rateReg[i][j] (host only)."""
        eig, pi = self.tl.eig, self.tl.freqs
        if self.kinds[k] == "counts":
            Q = (eig.evec * eig.evals[None, :]) @ eig.ievc
            rate_reg = Q * self.registers[k]
        else:
            rate_reg = self.registers[k]
        return float(np.sum(pi[:, None] * rate_reg))

    def expected_tree_length(self):
        """Sum over non-root nodes of branchRate * branch length (UnconditionedCountColumn.getExpectedTreeLength, :675-686)."""
        total = 0.0
        for n in range(self.tl.node_count):
            if self.tl.tree.parent[n] >= 0:
                t, r = self.tl.node_branch_time(n)
                total += r * t
        return total

    def unconditioned(self, k, categories=None):
        """The u_<tag> column(s) (UnconditionedCountColumn, :656-686): marginal rate x expected tree length; with more than one
        rate category, one value per pattern, times the rate of the pattern's category (``categories``: those of a sample)."""
        value = self.marginal_rate(k) * self.expected_tree_length()
        if self.tl.category_count == 1:
            return value
        cats = self.categories if categories is None else categories
        if cats is None:
            raise ValueError("several rate categories: pass the categories of a sample (sample(..., states=True))")
        return value * self.tl.cat_rates[np.asarray(cats)]

    def histories(self, sample, codes=None, compact=False):
        """[node][pattern] -> the reference's history string for a ``sample(..., history=True)`` (the history / history_all traits:
        StateHistory.toStringChanges, addEventToStringBuilder; with ``compact`` the 1-based site leads every event).  ``codes``:
        the data type's code per state (default "ACGT" for 4 states, else the state numbers)."""
        S = self.tl.state_count
        if codes is None:
            codes = "ACGT" if S == 4 else [str(i) for i in range(S)]
        ev = sample["events"]
        counts = sample["event_counts"]
        out = [["{}"] * counts.shape[1] for _ in range(counts.shape[0])]
        parts = {}
        for node, p, h, (a, b) in zip(ev["node"], ev["pattern"], ev["height"], ev["states"]):
            body = "{" + ("%d," % (p + 1) if compact else "") + java_double(h) + "," + codes[a] + "," + codes[b] + "}"
            parts.setdefault((int(node), int(p)), []).append(body)
        for (node, p), v in parts.items():
            out[node][p] = "{" + ",".join(v) + "}"
        return out


def java_double(x):
    """Double.toString: the shortest repr, as d.ddd for 1e-3 <= |x| < 1e7 and d.dddE[-]n otherwise."""
    x = float(x)
    if x == 0.0 or 1e-3 <= abs(x) < 1e7:
        r = repr(x)
        return r if "." in r else r + ".0"
    mant, exp = np.format_float_scientific(x, unique=True, trim="-").split("e")
    if "." not in mant:
        mant += ".0"
    return "%sE%d" % (mant, int(exp))
