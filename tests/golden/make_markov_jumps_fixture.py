#!/usr/bin/env python3
"""Transcribe the reference's Markov-jumps known answers into tests/golden/markov_jumps.json.

Run in the build container only (reads the reference tree, which the GPU box does not have):

    python tests/golden/make_markov_jumps_fixture.py

Data only, each entry with its file:line:
  hky_r              src/test/dr/evomodel/substmodel/MarkovJumpsSubstitutionModelTest.java: the HKY model (:46-48), time (:60),
                     register A->C (:61-63), rewards (:108), and the R package's J / C matrices (:161-187) and marginal rate
                     (:189), all in R's A,G,C,T order (MarkovJumpsCore.makeComparableToRPackage)
  two_tips           src/test/dr/app/beagle/MarkovJumpsTest.java: HKY kappa and frequencies (:71-72), mu (:78), the tree (:66),
                     the three registers, their kinds and scaleByTime (:151-177) and valuesFromR (:171)
"""
import json
import os
import re

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))


def numbers(text):
    return [float(x) for x in re.findall(r"-?\d+\.?\d*(?:[eE][-+]?\d+)?", text)]


def array_after(src, name):
    """The literal after `name = {` up to the matching `}` (one level of nesting allowed)."""
    i = src.index(name)
    i = src.index("{", i)
    depth, j = 0, i
    while True:
        if src[j] == "{":
            depth += 1
        elif src[j] == "}":
            depth -= 1
            if depth == 0:
                break
        j += 1
    return src[i:j + 1]


def main():
    sm = open(os.path.join(REF, "src/test/dr/evomodel/substmodel/MarkovJumpsSubstitutionModelTest.java")).read()
    mj = open(os.path.join(REF, "src/test/dr/app/beagle/MarkovJumpsTest.java")).read()
    marginal = re.search(r"rMarkovMarginalRate\s*=\s*([0-9.]+)\s*\*\s*([0-9.]+)", sm)
    regs_src = array_after(mj, "registerValues =")
    regs = [numbers(block) for block in re.findall(r"\{([^{}]*)\}", regs_src)]
    out = {
        "hky_r": {
            "source": "src/test/dr/evomodel/substmodel/MarkovJumpsSubstitutionModelTest.java",
            "kappa": 2.0, "frequencies_acgt": [0.3, 0.2, 0.25, 0.25], "time": 1.0,
            "register_from_to_acgt": [0, 1], "rewards": [1.0, 1.0, 1.0, 1.0],
            "order": "R package: A,G,C,T (rows and columns 1 and 2 of the A,C,G,T matrices swapped)",
            "tolerance": 1e-6,
            "rMarkovJumpsJ": numbers(array_after(sm, "rMarkovJumpsJ =")),
            "rMarkovJumpsC": numbers(array_after(sm, "rMarkovJumpsC =")),
            "rMarkovRewardsJ": numbers(array_after(sm, "rMarkovRewardsJ =")),
            "rMarkovRewardsC": numbers(array_after(sm, "rMarkovRewardsC =")),
            "rMarkovMarginalRate": float(marginal.group(1)) * float(marginal.group(2)),
        },
        "two_tips": {
            "source": "src/test/dr/app/beagle/MarkovJumpsTest.java",
            "kappa": 10.0, "frequencies_acgt": [0.40, 0.25, 0.25, 0.10], "mu": 0.5,
            "tree": "(human:1,chimp:1)", "tip_state_acgt": 0,
            "registers": regs, "tags": ["jump", "upper", "reward"], "kinds": ["counts", "counts", "rewards"],
            "scale_by_time": [False, False, True],
            "valuesFromR": numbers(re.search(r"valuesFromR\s*=\s*\{([^}]*)\}", mj).group(1)),
            "tolerance": 1e-2,
        },
    }
    assert len(out["hky_r"]["rMarkovJumpsJ"]) == 16 and len(out["hky_r"]["rMarkovRewardsC"]) == 16
    assert [len(r) for r in regs] == [16, 16, 4] and out["two_tips"]["valuesFromR"] == [0.782, 0.225, 1.777]
    with open(os.path.join(HERE, "markov_jumps.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
