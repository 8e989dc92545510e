"""The dense r-cell grid's index arithmetic (csrc/grid_dense.h) on the CPU:
tests/cpp/grid_dense_check.cpp builds bitmap, rank and start arrays on the host
for random and adversarial clouds and checks that every query's candidate
ranges are valid and hold every point within r.  Compiled with
-fsanitize=address,undefined and run as a plain executable."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dense_index_arithmetic_under_sanitizers(tmp_path):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "grid_dense_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "pointcloudregistration_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "grid_dense_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok:"), r.stdout
