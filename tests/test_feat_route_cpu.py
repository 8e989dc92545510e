"""The route of the mutual feature path (csrc/featnn_route.h) on the CPU:
tests/cpp/feat_route_check.cpp includes only that host header and checks the
route table for S = 1..4 under each PCR_FEAT_* hook (featnn_row9 falling off
above kRegroupMaxSteps column steps, the compact image only under the threshold
route and not under PCR_FEAT_IMAGE=full), the column slices at 1, 32, 256 and
257 pairs and the tile padding at counts 1, 32, 33, 512 and 513.  Compiled with
-fsanitize=address,undefined and run as a plain executable."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pointcloudregistration_amd", "csrc")
HOOKS = ("PCR_FEAT_ONE", "PCR_FEAT_ROW9", "PCR_FEAT_THRESH", "PCR_FEAT_IMAGE")


def test_feature_route_under_sanitizers(tmp_path):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "feat_route_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "feat_route_check.cpp"), "-o", exe], check=True)
    env = {k: v for k, v in os.environ.items() if k not in HOOKS}
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok:"), r.stdout


def test_the_driver_reads_no_hook_itself():
    """featnn.hip takes the route from feat_route: no getenv of its own, and the
    host header stays free of HIP."""
    with open(os.path.join(CSRC, "featnn.hip")) as f:
        src = f.read()
    assert "getenv" not in src and "feat_route(" in src
    with open(os.path.join(CSRC, "featnn_route.h")) as f:
        hdr = f.read()
    assert "#include \"" not in hdr and "hip_runtime" not in hdr and "__device__" not in hdr
