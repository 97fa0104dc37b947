"""csrc/msr_dense_plan.h (which dense sweep kernel serves a slice of queries, the slice width, the query padding) on the CPU:
tests/dense_plan_check.cpp enumerates every binding, row limit and query count against a table of its own; built with the
host compiler and its address / undefined-behaviour sanitizers and run as a program of its own.  No GPU, no ROCm runtime."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "modern-search-engines-project_amd", "csrc")


def test_dense_plan_over_its_whole_input_space(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    exe = str(tmp_path / "dense_plan_check")
    # (the sanitizer runtime linked statically: the program starts the same whatever else the environment preloads)
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-static-libasan", "-I" + CSRC, os.path.join(ROOT, "tests", "dense_plan_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "dense plan ok" in r.stdout
