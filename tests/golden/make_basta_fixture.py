"""Writes tests/golden/basta.json: inputs and restated results of two BASTA evaluations.

  four_taxa   the inputs of the reference's ci/TestXML/testAmbiguity_4taxa.xml: the tree ((A:0.1,B:0.2):0.3,(C:0.4,D:0.5):0.6)
              with node heights taken from its branch lengths, demes Asia, West_Medit, African (A, D in Asia; B in West_Medit;
              C in African), six unit migration rates (not normalised), population sizes 0.01 0.05 0.001, rate 1
  fifty_one   a seeded 51-tip serially sampled coalescent tree, four demes, random rates and sizes, two sub-intervals

The reference asserts no value for that file (it is a report-only XML) and its native BASTA library is not available, so
the numbers below do not come from the reference: they are what tests/basta_reference.py computes, and the fixture pins that
restatement (operation lists, per-interval coalescent probabilities, log-density) against regressions.  What ties the
restatement to something outside itself are the closed forms of tests/test_basta_host.py.

Run from the repository root:  python tests/golden/make_basta_fixture.py
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import basta_reference as ref                      # noqa: E402
from beast_mcmc_amd.inputs import trees            # noqa: E402


def case(left, right, height, tip_count, demes, q, sizes, rate, sub_intervals):
    s = len(sizes)
    ops, intervals, lengths, mats, n_buffers, n_intervals = ref.traverse(left, right, height, tip_count, rate, sub_intervals)
    w, v = np.linalg.eig(np.asarray(q).T)
    vi = np.linalg.inv(v)
    matrices = {m: np.abs(np.real((v * np.exp(w * t)[None, :]) @ vi)) for m, t in mats}
    tips = np.zeros((tip_count, s))
    tips[np.arange(tip_count), demes] = 1.0
    logl, _, probabilities = ref.evaluate(tips, ops, intervals, lengths, matrices, sizes, n_buffers, n_intervals)
    return {"state_count": s, "tip_count": tip_count, "left": [int(x) for x in left], "right": [int(x) for x in right],
            "height": [float(x) for x in height], "demes": [int(x) for x in demes], "rates": np.asarray(q).tolist(),
            "sizes": [float(x) for x in sizes], "rate": rate, "sub_intervals": sub_intervals, "tips": tips.reshape(-1).tolist(),
            "operations": ops.reshape(-1).tolist(), "intervals": intervals.tolist(), "lengths": lengths.tolist(),
            "matrix_lengths": [[int(m), float(t)] for m, t in mats],
            "matrices": {str(m): matrices[m].reshape(-1).tolist() for m in matrices},
            "buffer_count": int(n_buffers), "interval_count": int(n_intervals),
            "coalescent_probabilities": probabilities.tolist(), "log_likelihood": float(logl)}


def main():
    # tips A, B, C, D = 0..3; node 4 = (A, B), node 5 = (C, D), node 6 = the root; D is the most recent tip
    left, right = [-1, -1, -1, -1, 0, 2, 4], [-1, -1, -1, -1, 1, 3, 5]
    height = [0.7, 0.6, 0.1, 0.0, 0.8, 0.5, 1.1]
    q = np.ones((3, 3)) - 3.0 * np.eye(3)
    four = case(left, right, height, 4, [0, 1, 2, 0], q, [0.01, 0.05, 0.001], 1.0, 1)
    rng = np.random.default_rng(20240051)
    tree = trees.heterochronous_coalescent_tree(51, rng, sampling_span=1.0, population=3.0)
    q = rng.gamma(2.0, 0.5, size=(4, 4)) / 4
    np.fill_diagonal(q, 0.0)
    np.fill_diagonal(q, -q.sum(axis=1))
    fifty = case(tree.left, tree.right, tree.height, 51, rng.integers(0, 4, size=51), q, rng.gamma(4.0, 0.5, size=4) + 0.05, 0.8, 2)
    with open(os.path.join(HERE, "basta.json"), "w") as fh:
        json.dump({"_header": __doc__.split("\n\nRun from")[0], "four_taxa": four, "fifty_one": fifty}, fh)
        fh.write("\n")


if __name__ == "__main__":
    main()
