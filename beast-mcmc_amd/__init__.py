"""MI355X-native tree-likelihood engine behind BEAST's ``beagle.Beagle`` surface.

Layout (only what the hot path needs — SURVEY.md §8):
  csrc/     hand-written gfx950 HIP kernels, the C ABI (include/beagle_mi355.h) and the JNI shim
  (the C++ mirror of the reference's BEAGLE caller — BeagleTreeLikelihood / BufferIndexHelper — is harness, not package:
   tools/host/tree_likelihood.cpp, built into lib/libbeast_host.so)
  beagle.py           ctypes binding with the ``beagle.Beagle`` method set
  treelikelihood.py   ctypes handle on the C++ host driver
  ancestral.py        ancestral-state draws on the device (AncestralStateBeagleTreeLikelihood's caller side)
  markovjumps.py      Markov-jump counts and rewards on the device (MarkovJumpsBeagleTreeLikelihood's caller side)
  simulate.py         sequence simulation down the tree on the device (BeagleSequenceSimulator / Partition's caller side)
  completehistory.py  complete substitution histories down the tree on the device (CompleteHistorySimulator's caller side)
  robustcounting.py   codon robust counts over three position instances (CodonPartitionedRobustCounting's caller side)
  nodeheight.py       node-height gradients and diagonal Hessians in one call (DiscreteTraitNodeHeightDelegate's caller side)
  nodeposteriors.py   marginal node state posteriors on the device in one call (NodePosteriorTreeLikelihood's caller side)
  placement.py        scores of attaching new sequences on every branch in one call (CheckPointTreeModifier's caller side)
  regraft.py          scores of every regraft point of a pruned subtree in one call (GibbsPruneAndRegraft's caller side)
  substgradient.py    substitution-parameter gradients through differential matrices formed on the device (BranchSubstitutionParameterDelegate's caller side)
  eigensystems.py     eigen systems of a set of reversible models decomposed on the device in one call (SubstitutionModelDelegate's caller side)
  generators.py       branch matrices straight from generators, no eigen system, in one call (SubstitutionModelDelegate's caller side for models without one)
  epochs.py           branch matrices of epoch models: the product of a branch's per-epoch matrices in one call (EpochBranchModel and SubstitutionModelDelegate's caller side)
  stochasticdollo.py  the stochastic Dollo (ALS) likelihood: node-pattern likelihoods on the device in one call (ALSTreeLikelihood's caller side)
  tipmodels.py        tip error models as emission tables folded into the tip branch matrices (SequenceErrorModel's caller side)
  basta.py            the BASTA structured-coalescent likelihood on the device (BeagleBastaLikelihoodDelegate's caller side)
  mds.py              multidimensional scaling on the device (MultiDimensionalScalingLikelihood's caller side, libmds2_jni.so)
  inputs/   what feeds the engine: eigen systems, gamma rate categories, site patterns, trees, synthetic workloads
  sharding.py         pattern-block sharding across GPUs + the single lnL all-reduce

The directory name contains a hyphen, so import it through the root-level shim: ``import beast_mcmc_amd``.
"""
from . import ancestral, basta, beagle, completehistory, eigensystems, epochs, generators, markovjumps, mds, multipartition, nodeheight, nodeposteriors, placement, regraft, robustcounting, simulate, stochasticdollo, substgradient, tipmodels, treelikelihood     # noqa: F401
from .inputs import patterns, siterates, substmodel, synth, trees   # noqa: F401
