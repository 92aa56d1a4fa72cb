"""Slices cut by what compression leaves of a list (beast-mcmc_amd/csrc/planner.h WalkPlanner::repeatWeights) on the CPU.

tests/native/plan_check_slicing.cpp plans every list of random and caterpillar trees of 24, 48 and 200 tips and of one seeded random tree
of 1 000 tips twice — a plain definition weighed as its steps, and as the one gather it becomes once its clade is taken from a class
table — under definition caps 8 and 24 and memory-definition caps 0 and 8, and checks the second plan: stored buffers with the bits of
list-order evaluation (within 1e-12 with folded reciprocals), the payments of the compressed plan, the slices a forest in launch order
and none of them empty, the stored set of the first plan, no peeled slice over its chunk, fewer slices on the large tree, and the
weighting as part of a cached plan's identity."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_slices_by_compressed_weight(tmp_path):
    exe = str(tmp_path / "plan_check_slicing")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-fsanitize=address,undefined",
                           os.path.join(ROOT, "tests", "native", "plan_check_slicing.cpp"),
                           os.path.join(ROOT, "beast-mcmc_amd", "csrc", "planner.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "plan_check_slicing: OK" in out.stdout
