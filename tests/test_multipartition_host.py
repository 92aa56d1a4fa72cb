"""Host logic of the partitioned caller (beast_mcmc_amd/multipartition.py) on the CPU oracle: buffer-offset bookkeeping of full
evaluations, node-height moves and their rejection (MultiPartitionDataLikelihoodDelegate's call sequence with BufferIndexHelper
flips).  The oracle restates no pattern-partition call, so the harness runs with ONE partition here — the sequence is the same,
updatePartials instead of updatePartialsByPartition; real partitions are covered on the GPU (tests/test_gpu_configs.py)."""
import numpy as np

import helpers
from beast_mcmc_amd.inputs import synth
from beast_mcmc_amd.inputs.synth import PartitionedWorkload
from beast_mcmc_amd.multipartition import MultiPartitionTreeLikelihood
from beast_mcmc_amd.treelikelihood import BeagleTreeLikelihood, RESCALE_NONE


def fresh(w, lib):
    o = BeagleTreeLikelihood(w, library=lib, rescaling=RESCALE_NONE, delay_rescaling=False)
    v = o.getLogLikelihood()
    o.close()
    return v


def test_moves_and_rejections_on_one_partition(oracle_lib):
    pw0 = synth.config_e(scale=0.02)
    pw = PartitionedWorkload("one partition", pw0.tree, pw0.parts[2:3])
    tree = pw.tree
    tl = MultiPartitionTreeLikelihood(pw, library=oracle_lib)
    by, total = tl.calculate()
    assert helpers.rel_err(total, fresh(pw.parts[0], oracle_lib)) <= 1e-13 and by.shape == (1,)
    rng = np.random.default_rng(3)
    accepted = []
    for it in range(12):
        node = tree.root if it == 4 else int(rng.integers(tree.tip_count, tree.node_count))
        lo = max(tree.height[int(tree.left[node])], tree.height[int(tree.right[node])])
        hi = tree.height[tree.parent[node]] if node != tree.root else tree.height[node] * 1.2
        before = (float(tree.height[node]), tl.flip.copy(), tl.mf.copy())
        _, v = tl.move_node_height(node, lo + (hi - lo) * float(rng.uniform(0.1, 0.9)))
        assert helpers.rel_err(v, fresh(pw.parts[0], oracle_lib)) <= 1e-13, (it, node)      # the moved tree, evaluated from scratch
        if it % 2:
            tl.restore_move()
            assert tree.height[node] == before[0] and np.array_equal(tl.flip, before[1]) and np.array_equal(tl.mf, before[2])
        else:
            accepted.append(node)
    assert accepted
    # the accepted state in full, on the instance that moved (all offsets flip together again) and from scratch
    _, again = tl.calculate()
    assert helpers.rel_err(again, fresh(pw.parts[0], oracle_lib)) <= 1e-13
    tl.close()


def test_per_partition_references_add_up_to_the_unpartitioned_one(oracle_lib):
    """The reference of tests/test_gpu_partition_sequences.py: with one model shared by every partition, the per-partition oracle
    instances' log-likelihoods add up to — and their site values in a row are — those of one unpartitioned instance over all
    patterns, with and without write-mode rescaling.  (A wrong reference must not pass a wrong engine.)"""
    import beast_mcmc_amd as bm
    from beast_mcmc_amd.inputs.synth import Workload
    NONE = bm.beagle.NONE
    for S, sizes in ((4, [37, 5, 130, 64, 1, 77, 33, 129, 20]), (20, [150, 77])):
        tree, wls = helpers.two_partitions(S, 10, sizes, seed=5 + S)
        m = wls[0]
        wls = [Workload(w.name, w.tree, m.eig, m.freqs, m.cat_rates, m.cat_weights, w.tip_states, w.weights, S) for w in wls]
        T, nodes = 10, 19
        internal = [n for n in tree.postorder() if n >= T]
        branches = [n for n in range(nodes) if n != tree.root]
        for scaling in (False, True):
            def evaluate(tips, weights):
                b = bm.beagle.Beagle(T, nodes, T, S, len(weights), 1, nodes, 4, T, library=oracle_lib)
                try:
                    for t in range(T):
                        b.setTipStates(t, tips[t])
                    b.setPatternWeights(weights)
                    b.setEigenDecomposition(0, m.eig.evec, m.eig.ievc, m.eig.evals)
                    b.setCategoryRates(m.cat_rates)
                    b.setCategoryWeights(0, m.cat_weights)
                    b.setStateFrequencies(0, m.freqs)
                    b.updateTransitionMatrices(0, branches, None, None, [tree.branch_length(n) for n in branches], len(branches))
                    ops = []
                    for n in internal:
                        l, r = int(tree.left[n]), int(tree.right[n])
                        ops += [n, n - T if scaling else NONE, NONE, l, l, r, r]
                    if scaling:
                        b.resetScaleFactors(T - 1)
                    b.updatePartials(ops, len(internal), T - 1 if scaling else NONE)
                    v = [0.0]
                    b.calculateRootLogLikelihoods([tree.root], [0], [0], [T - 1 if scaling else NONE], 1, v)
                    return v[0], b.getSiteLogLikelihoods()
                finally:
                    b.finalize()
            parts = [evaluate(w.tip_states, w.weights) for w in wls]
            whole = evaluate(np.concatenate([w.tip_states for w in wls], axis=1), np.concatenate([w.weights for w in wls]))
            assert helpers.rel_err(sum(v for v, _ in parts), whole[0]) <= 1e-12, (S, scaling)
            site = np.concatenate([s for _, s in parts])
            assert np.max(np.abs(site - whole[1]) / np.abs(whole[1])) <= 1e-12, (S, scaling)
