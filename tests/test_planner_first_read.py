"""The walk planner's two memory-definition caps and the long definitions a list only reads (beast-mcmc_amd/csrc/planner.h memStepCapSeen,
longMemoryOperands), on the CPU.

tests/native/plan_check_first_read.cpp drives the planner as tests/native/plan_check.cpp does — same worlds, same index-level interpreter
of the walk kernel's register model — through chains of full evaluations and branch moves, half of them rejected, the way the engine
drives it: a closed list is planned under the short cap when it is first seen and once more under the long one when it comes again; before
a move's list is planned, the memory definitions longer than the threshold that it reads without producing their stored operand are named
(exactly those, checked against the definitions) and materialised.  Every materialised buffer, and after every list every real buffer and
scale buffer, must agree bitwise with list-order evaluation; a list stores fewer nodes from its second coming on and is replayed from its
third; no move makes a definition over the short cap; a stored definition is not named again before its buffer is defined again; the moves
never walk more micro-operations than with the threshold at the cap."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_two_caps_and_first_read_storing_equal_list_order_evaluation(tmp_path):
    exe = str(tmp_path / "plan_check_first_read")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-fsanitize=address,undefined",
                           os.path.join(ROOT, "tests", "native", "plan_check_first_read.cpp"),
                           os.path.join(ROOT, "beast-mcmc_amd", "csrc", "planner.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "plan_check_first_read: OK" in out.stdout
