"""Repeated sub-patterns (beast-mcmc_amd/csrc/planner.h RepeatIndex, findRepeatRuns, emitRepeatPlan, RepeatRows) on the CPU.

tests/native/plan_check_repeats.cpp checks the class index against a brute-force count of distinct sub-patterns on random data (classes,
class count, representatives, determinism, the class limit, what a subtree swap rebuilds), the row allocator of the class tables, and —
on tests/native/plan_check.cpp's harness — the compressed plan: every table operand names a clade evaluated in the same plan, the
class-table programs pay no scale factors, the payments of the whole plan are those of the uncompressed plan, and every stored buffer
ends up with the bits the uncompressed plan gives it, with folded reciprocals at two caps and without folding."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_repeat_index_and_compressed_plans(tmp_path):
    exe = str(tmp_path / "plan_check_repeats")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-fsanitize=address,undefined",
                           os.path.join(ROOT, "tests", "native", "plan_check_repeats.cpp"),
                           os.path.join(ROOT, "beast-mcmc_amd", "csrc", "planner.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "plan_check_repeats: OK" in out.stdout
