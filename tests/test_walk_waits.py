"""The stage waits of the walk kernels (beast-mcmc_amd/csrc/kernels.h walkStageWaits) on the CPU.

tests/native/walk_waits_check.cpp runs seeded random slices of valid flags words through it — both pipelines, both BEAGLE_MI355_STRICT_WAITS
values, the three padding modes — and checks every wait against the documented issue order of the kernels' vector-memory instructions."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_stage_waits_against_the_issue_order(tmp_path):
    exe = str(tmp_path / "walk_waits_check")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"),
                           os.path.join(ROOT, "tests", "native", "walk_waits_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "walk_waits_check: OK" in out.stdout
