"""csrc/msr_stream_plan.h (the streaming dense pass: what a binding allocates, and per call the width, the groups per launch,
the rows and the kernel instance of every launch, the sample and the emit pass' cut) on the CPU: tests/stream_plan_check.cpp
enumerates engine sizes, grids, the two optional copies of the rows and every query count against a table of its own; built
with the host compiler and its address / undefined-behaviour sanitizers and run as a program of its own.  No GPU, no ROCm
runtime."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "modern-search-engines-project_amd", "csrc")


def build_stream_plan_check(tmp_path):
    """Compiles tests/stream_plan_check.cpp; returns the program's path."""
    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    exe = str(tmp_path / "stream_plan_check")
    # (the sanitizer runtime linked statically: the program starts the same whatever else the environment preloads)
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-static-libasan", "-I" + CSRC, os.path.join(ROOT, "tests", "stream_plan_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    return exe


def test_stream_plan_over_its_whole_input_space(tmp_path):
    r = subprocess.run([build_stream_plan_check(tmp_path)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "stream plan ok" in r.stdout
