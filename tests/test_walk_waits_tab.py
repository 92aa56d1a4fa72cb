"""The stage waits of the assembly walk loop with class-table children (beast-mcmc_amd/csrc/kernels.h walkStageWaits, tableIds) on the CPU.

tests/native/walk_waits_tab_check.cpp models the loop's loads in issue order — a table child's class ids are requested by the fetch, its
rows where the operand is consumed — over seeded random and directed slices, checks that every stage finds its own small loads and the
next micro-operation's table ids landed behind its wait, and that the six-argument call returns what it returned before the mode existed."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_stage_waits_with_table_ids_in_the_fetch(tmp_path):
    exe = str(tmp_path / "walk_waits_tab_check")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"),
                           os.path.join(ROOT, "tests", "native", "walk_waits_tab_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "walk_waits_tab_check: OK" in out.stdout
