"""The walk planner's memory definitions (beast-mcmc_amd/csrc/planner.h memStepCap) against list-order evaluation, on the CPU.

tests/native/plan_check_memdefs.cpp drives the planner as tests/native/plan_check.cpp does — same worlds, same index-level interpreter of
the walk kernel's register model — with WalkPlanner::memStepCap on: full evaluations with BufferIndexHelper flips, branch moves with
rejections, rescaling cycles, a 200-tip caterpillar (every spine node over one stored child), a list that rewrites a stored operand
without redefining its reader, a changed tip below a memory definition.  Every real buffer and scale buffer must agree bitwise with
list-order evaluation; no definition reads two stored nodes or exceeds the cap; no full-evaluation program reads back what its own
slice stores, but for a storing parent's first child; fewer nodes are stored than with the feature off."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_memory_definitions_equal_list_order_evaluation(tmp_path):
    exe = str(tmp_path / "plan_check_memdefs")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-fsanitize=address,undefined",
                           os.path.join(ROOT, "tests", "native", "plan_check_memdefs.cpp"),
                           os.path.join(ROOT, "beast-mcmc_amd", "csrc", "planner.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "plan_check_memdefs: OK" in out.stdout
