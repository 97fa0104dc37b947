"""csrc/msr_devmem.h (the engine's lifetime groups of device allocations) on the CPU: tests/devmem_check.cpp instantiates the
group with a counting host allocator; built with the host compiler and its address / undefined-behaviour sanitizers and run
as a program of its own.  No GPU, no ROCm runtime."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "modern-search-engines-project_amd", "csrc")


def test_lifetime_groups_under_a_counting_allocator(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    exe = str(tmp_path / "devmem_check")
    # (the sanitizer runtime linked statically: the program starts the same whatever else the environment preloads)
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-static-libasan", "-I" + CSRC, os.path.join(ROOT, "tests", "devmem_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "devmem ok" in r.stdout
