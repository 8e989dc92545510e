"""The fit rule of a grid's LDS copy (csrc/lds_fit.h) on the CPU:
tests/cpp/lds_fit_check.cpp checks that it refuses more than 65535 points,
more than 65536 slot starts and a budget one byte too small, and that the C4
cloud (8192 points, 8192 slots) takes 147,458 B rounded to 16.  Compiled with
-fsanitize=address,undefined and run as a plain executable."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pointcloudregistration_amd", "csrc")


def test_lds_fit_rule_under_sanitizers(tmp_path):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "lds_fit_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "lds_fit_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok:"), r.stdout


def test_the_grid_consumers_share_the_rule():
    """grid.h's grid_lds4_bytes (RANSAC, ICP) and the Chamfer's dispatch both
    go through lds4_fit_bytes."""
    with open(os.path.join(CSRC, "grid.h")) as f:
        assert "return lds4_fit_bytes(mstride, S, budget);" in f.read()
    with open(os.path.join(CSRC, "nnd_grid.hip")) as f:
        assert "lds4_fit_bytes(a.nmax, S, " in f.read()
