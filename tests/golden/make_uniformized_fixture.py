#!/usr/bin/env python3
"""Transcribe the reference's uniformization known answers into tests/golden/uniformized_jumps.json.

Run in the build container only (reads the reference tree, which the GPU box does not have):

    python tests/golden/make_uniformized_fixture.py

Data only, from src/test/dr/math/UniformizedStateHistoryTest.java: the HKY model (kappa, frequencies: setUp), the R package's
one- and three-step chain matrices (testSubordinatedProcessGeneration) and next-state pdf (testComputePdfForNextDraw, start 1,
end 0, n 4, i 1), all in R's A,G,C,T order (MarkovJumpsCore.makeComparableToRPackage), and the Poisson-draw cases of
testTotalChangesSamplingMethods: (start, end, time, [(number of pdf terms summed, offset, expected draw)]).
"""
import json
import os
import re

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))


def numbers(text):
    return [float(x) for x in re.findall(r"-?\d+\.?\d*(?:[eE][-+]?\d+)?", text)]


def literal(src, name):
    i = src.index(name)
    return numbers(src[src.index("{", i):src.index("}", i) + 1])


def main():
    path = "src/test/dr/math/UniformizedStateHistoryTest.java"
    src = open(os.path.join(REF, path)).read()
    kappa = numbers(re.search(r"Parameter kappa = new Parameter.Default\(1, ([^)]*)\)", src).group(1))[0]
    pi = literal(src, "double[] pi =")
    out = {
        "source": path,
        "order": "R package A,G,C,T (swap states 1 and 2 for A,C,G,T)",
        "kappa": kappa,
        "frequencies_acgt": pi,
        "r_one_step": literal(src, "double[] rOneStep ="),
        "r_three_step": literal(src, "double[] rThreeStep ="),
        "next_state": {"start": 1, "end": 0, "n": 4, "i": 1, "pdf_r": literal(src, "double[] rPDF = new double[]")},
        "poisson_draws": [
            {"start": 1, "end": 0, "time": 0.5, "cases": [[2, -1e-6, 1], [2, 1e-6, 2], [3, 1e-6, 3]]},
            {"start": 1, "end": 1, "time": 0.75, "cases": [[3, -1e-6, 2], [3, 1e-6, 3]]},
        ],
        "tolerance": 1e-6,
    }
    with open(os.path.join(HERE, "uniformized_jumps.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
