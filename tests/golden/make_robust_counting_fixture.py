#!/usr/bin/env python3
"""Transcribe the reference's robust-counting known answers into tests/golden/robust_counting.json.

Run in the build container only (reads the reference tree, which the GPU box does not have):

    python tests/golden/make_robust_counting_fixture.py

Data only, each entry with its file:line:
  register_sums      src/test/dr/evomodel/substmodel/CodonPartitionedRobustCountingTest.java: the sums of the 64 x 64 synonymous
                     and non-synonymous register matrices (:99, :108)
  conditional_means  the same file: three HKY kappa 2 models with equal frequencies (:56-65), time 1.0 (:155), AAA -> AAC and
                     AAA -> AAG (:153-154, :168), the three conditional means and their tolerance (:166-178)
  universal_code     src/dr/evolution/datatype/GeneticCode.java: the universal table string (:68), codon i * 16 + j * 4 + k over A, C, G, T
"""
import json
import os
import re

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
TEST = "src/test/dr/evomodel/substmodel/CodonPartitionedRobustCountingTest.java"
CODE = "src/dr/evolution/datatype/GeneticCode.java"


def main():
    src = open(os.path.join(REF, TEST)).read()
    code = open(os.path.join(REF, CODE)).read()
    sums = [int(x) for x in re.findall(r"assertEquals\((\d+), \(int\) total", src)]
    means = re.findall(r"assertEquals\(([0-9.]+), c\[from \* 64 \+ to\], ([0-9.Ee-]+)\)", src)
    kappas = [float(x) for x in re.findall(r"new HKY\(([0-9.]+),", src)]
    freqs = [[float(v) for v in m.split(",")] for m in re.findall(r"new double\[\]\{([0-9., ]+)\}", src)]
    time = float(re.search(r"double time = ([0-9.]+);", src).group(1))
    states = re.findall(r"codons\.getState\('(\w)', '(\w)', '(\w)'\)", src[src.index("testCounts"):])
    table = re.search(r'"([A-Z*]{64})"', code).group(1)
    out = {
        "register_sums": {"source": TEST + ":99,108", "syn": sums[0], "nonsyn": sums[1]},
        "conditional_means": {
            "source": TEST + ":56-65,153-178",
            "kappa": kappas, "frequencies_acgt": freqs, "time": time,
            "from": "".join(states[0]), "to": ["".join(states[1]), "".join(states[2]), "".join(states[2])],
            "labeling": ["syn", "syn", "nonsyn"],
            "values": [float(v) for v, _ in means], "tolerance": float(means[0][1]),
        },
        "universal_code": {"source": CODE + ":68", "order": "codon i * 16 + j * 4 + k over A, C, G, T", "table": table},
    }
    assert out["register_sums"]["syn"] == 134 and out["register_sums"]["nonsyn"] == 392
    assert out["conditional_means"]["values"] == [0.525401, 0.970012, 1.099807] and len(kappas) == 3 and len(freqs) == 3
    assert out["conditional_means"]["from"] == "AAA" and out["conditional_means"]["to"] == ["AAC", "AAG", "AAG"]
    with open(os.path.join(HERE, "robust_counting.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
