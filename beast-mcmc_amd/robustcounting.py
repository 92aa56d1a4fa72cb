"""Codon robust counting ("renaissance counting") on the device: the caller-side mirror of
``dr.evomodel.substmodel.CodonPartitionedRobustCounting`` (src/dr/evomodel/substmodel/CodonPartitionedRobustCounting.java).

The reference keeps one ``AncestralStateBeagleTreeLikelihood`` per codon position, reads the three draws back, joins them into
codon states and, per branch and labelling, forms a Minin-Suchard conditional-mean table of the 64-state product chain of the three
nucleotide models (``ProductChainSubstitutionModel``) that every site then reads (:216-307); the "unconditioned" counts are one
simulated history per site of the same chain (:619-647).  Here the three draws, the tables and the gather are ONE engine call
(include/beagle_mi355.h ``beagleMi355RobustCounts``) and the simulation is another (``beagleMi355SimulateUnconditionedCounts``);
this class builds the product chain, the registers and the node lists, and hands the results back per tree node.

Sample after ``getLogLikelihood`` on all three tree likelihoods, as for the ancestral sampler.  The three tree likelihoods share
one tree and one pattern count (patterns are sites: the reference requires uncompressed patterns, :138-146); the product chain
takes each position's site rate ``getRateForCategory(0)``, and more than one category is not supported there
(ProductChainSubstitutionModel.java:81-87) — the instances' categories are drawn and otherwise unused.

Out of scope: ``useUniformization="true"`` (sampled codon histories), sharded and partitioned instances, product chains other than
4 x 4 x 4.
"""
import numpy as np

from .ancestral import AncestralStateSampler

UNIVERSAL_CODE = "KNKNTTTTRSRSIIMIQHQHPPPPRRRRLLLLEDEDAAAAGGGGVVVV*Y*YSSSS*CWCLFLF"     # codon i * 16 + j * 4 + k over A, C, G, T


def codon_registers(code_table=UNIVERSAL_CODE):
    """-> (syn, nonsyn), each [64][64] of 0 / 1: CodonLabeling.getRegisterMatrix over Codons.constructRateMap's classes
    (CodonLabeling.java:59-98, Codons.java:331-406) — a change at exactly one position between two sense codons, synonymous when
    the amino acid stays the same; nothing into or out of a stop codon."""
    syn, non = np.zeros((64, 64)), np.zeros((64, 64))
    for u in range(64):
        for v in range(64):
            if u == v or code_table[u] == "*" or code_table[v] == "*":
                continue
            differing = sum(1 for shift in (4, 2, 0) if ((u >> shift) & 3) != ((v >> shift) & 3))
            if differing != 1:
                continue
            (syn if code_table[u] == code_table[v] else non)[u, v] = 1.0
    return syn, non


def product_chain(eigs, site_rates):
    """The 64-state product chain of three nucleotide models (ProductChainSubstitutionModel.computeKroneckerSumsAndProducts,
    :301-362): every base model's Q and eigenvalues times its site rate (scaleForProductChain, :188-202), Q the Kronecker sum,
    the eigenvalues added, the eigenvectors Kronecker-multiplied with the first position most significant, the inverse through
    the transpose as there.  ``eigs``: three inputs.substmodel.EigenDecomposition.  -> (U, U^-1, lambda, Q)."""
    U, UiT, lam, Q = None, None, None, None
    for eig, rate in zip(eigs, site_rates):
        evec, ievc, evals = np.asarray(eig.evec, dtype=np.float64), np.asarray(eig.ievc, dtype=np.float64), \
            np.asarray(eig.evals, dtype=np.float64)
        q = (evec * evals[None, :]) @ ievc
        if rate != 1.0:
            q, evals = rate * q, rate * evals
        if U is None:
            U, UiT, lam, Q = evec, ievc.T, evals, q
            continue
        m, n = Q.shape[0], q.shape[0]
        Q = np.kron(Q, np.eye(n)) + np.kron(np.eye(m), q)
        lam = np.kron(lam, np.ones(n)) + np.kron(np.ones(m), evals)
        U = np.kron(U, evec)
        UiT = np.kron(UiT, ievc.T)
    return np.ascontiguousarray(U), np.ascontiguousarray(UiT.T), np.ascontiguousarray(lam), np.ascontiguousarray(Q)


class CodonPartitionedRobustCounting:
    """Robust counts of three ``treelikelihood.BeagleTreeLikelihood``s (codon positions 1, 2, 3 over one tree)."""

    LABELINGS = ("syn", "nonsyn")

    def __init__(self, tl0, tl1, tl2, labelings=("syn", "nonsyn"), include_external=True, include_internal=True):
        self.tls = (tl0, tl1, tl2)
        if len({tl.pattern_count for tl in self.tls}) != 1 or any(tl.state_count != 4 for tl in self.tls):
            raise ValueError("three 4-state tree likelihoods with one pattern count")
        self.samplers = [AncestralStateSampler(tl) for tl in self.tls]
        self.beagle = self.samplers[0].beagle
        syn, non = codon_registers()
        known = {"syn": syn, "nonsyn": non}
        self.labelings = tuple(labelings)
        self.registers = np.stack([known[name] for name in self.labelings])
        self.include_external, self.include_internal = bool(include_external), bool(include_internal)

    def chain(self):
        """(U, U^-1, lambda, Q, frequencies) of the product chain from the models last set on the three tree likelihoods."""
        U, Ui, lam, Q = product_chain([tl.eig for tl in self.tls], [float(tl.cat_rates[0]) for tl in self.tls])
        pi = np.kron(np.kron(self.tls[0].freqs, self.tls[1].freqs), self.tls[2].freqs)
        return U, Ui, lam, Q, pi

    def node_lists(self):
        """-> (rows int32 [3, node_count, 3], tree node of each row): a node list per position, the same pre-order."""
        lists = [s.node_list() for s in self.samplers]
        return np.stack([rows for rows, _ in lists]), lists[0][1]

    def branch_lengths(self, order):
        """branch rate x time per row of the node list (row 0: 0), read from position 1's host driver."""
        out = np.zeros(len(order))
        for r, n in enumerate(order):
            if r > 0:
                t, rate = self.tls[0].node_branch_time(int(n))
                out[r] = rate * t
        return out

    def include_rows(self, order):
        tips = np.asarray(order) < self.tls[0].tip_count
        return np.where(tips, self.include_external, self.include_internal).astype(np.uint8)

    def sample(self, seed, map=False, per_branch_site=False, states=False):
        """``seed``: one integer (positions get seed, seed + 1, seed + 2) or three.  -> dict indexed by tree node number:
          "site"    [K, P]             per-site totals over the included branches (the c_<labeling>[site] columns)
          "branch"  [K, node_count]    per-branch totals over the sites (the root's row is 0)
          "tree"    [K]                the sum of "site"
          "branch_site" [K, node_count, P]  when ``per_branch_site``
          "states"  uint8 [3, node_count, P]  when ``states``."""
        seeds = [seed, seed + 1, seed + 2] if np.isscalar(seed) else list(seed)
        rows, order = self.node_lists()
        U, Ui, lam, Q, _ = self.chain()
        res = self.beagle.robustCounts([s.beagle for s in self.samplers[1:]], rows, self.branch_lengths(order), U, Ui, lam, Q,
                                       self.registers, seeds, map=map, include_rows=self.include_rows(order), states=states,
                                       counts=per_branch_site)
        out = {"site": res["site_totals"], "tree": res["site_totals"].sum(axis=1)}
        branch = np.empty_like(res["branch_totals"])
        branch[:, order] = res["branch_totals"]
        out["branch"] = branch
        if per_branch_site:
            bs = np.empty_like(res["counts"])
            bs[:, order] = res["counts"]
            out["branch_site"] = bs
        if states:
            st = np.empty_like(res["states"])
            st[:, order] = res["states"]
            out["states"] = st
        return out

    def marginal_rate(self, k):
        """MarkovJumpsSubstitutionModel.getMarginalRate of labelling k on the product chain: sum_i pi_i sum_j (Q o R_k)[i][j]."""
        _, _, _, Q, pi = self.chain()
        R = self.registers[k].copy()
        np.fill_diagonal(R, 0.0)
        return float(np.sum(pi[:, None] * (Q * R)))

    def expected_tree_length(self):
        """Sum over non-root nodes of branch rate x branch length (getExpectedTreeLength, :675-686)."""
        tl = self.tls[0]
        total = 0.0
        for n in range(tl.node_count):
            if tl.tree.parent[n] >= 0:
                t, r = tl.node_branch_time(n)
                total += r * t
        return total

    def unconditioned(self, seed, per_branch=False):
        """Simulated unconditioned counts (fillInUnconditionalTraitValues, :619-647): one history per site over the expected tree
        length -> [K, P]; with ``per_branch`` one per (branch, site) over each branch's length -> [K, node_count, P] by tree node
        (doUnconditionedPerBranch; the root's row is 0)."""
        _, _, _, Q, pi = self.chain()
        P = self.tls[0].pattern_count
        if not per_branch:
            res = self.beagle.simulateUnconditionedCounts(Q, pi, [self.expected_tree_length()], P, self.registers, seed, totals=False)
            return res["counts"][:, 0]
        _, order = self.node_lists()
        res = self.beagle.simulateUnconditionedCounts(Q, pi, self.branch_lengths(order), P, self.registers, seed, totals=False)
        out = np.empty_like(res["counts"])
        out[:, order] = res["counts"]
        return out
