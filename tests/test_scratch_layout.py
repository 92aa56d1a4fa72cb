"""What is inside the samplers' device scratch buffers (beast-mcmc_amd/csrc/scratch_layout.h) on the CPU.

tests/native/scratch_layout_check.cpp builds every layout — ancestral draws, Markov jumps, uniformized jumps, the event list, sequence
simulation, robust counts (conditional and unconditioned), complete histories — over a grid of shapes (rows x patterns that are no
multiple of 256, one pattern, 1 and MAX_JUMP_REGISTERS registers, a stage of 0, 1 and fewer rows than the list, histories / values / row
totals on and off, row structs whose size is no multiple of 8) and checks each section's offset and the total against the formulas the
samplers used before the carver, that sections are disjoint and ascending, that each is aligned for its element type, and that a section
the call does not ask for resolves to null."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_scratch_layouts(tmp_path):
    exe = str(tmp_path / "scratch_layout_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
                           os.path.join(ROOT, "tests", "native", "scratch_layout_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "scratch_layout_check: OK" in out.stdout
