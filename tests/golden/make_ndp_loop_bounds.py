"""Record the f32 noise floor of the NDP warp: tests/golden/ndp_loop_bounds.npz.

For every case of tests/test_ndp_warp_edges_gpu.py (tests/ndp_loop_ref.py:
WARP_CASES) run the mirror pyramid (ndp_opt.NDPLayer, f32, CPU) and measure it
against the f64 oracle (oracle.ndp_warp): the largest absolute distance over
every level's points, and over every level's nonrigidity.  The GPU test bounds
pcr_ndp_warp by 4 x the floors pooled over the case list.  CPU only; recorded
numbers only.

Keys:
  <case name> (2) f64     the case's (points, nonrigidity) error
  floor_xyz, floor_s      the largest of each over the cases

    python tests/golden/make_ndp_loop_bounds.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.dirname(HERE), ROOT, os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)
import ndp_loop_ref as ref  # noqa: E402
import oracle  # noqa: E402

OUT = os.path.join(HERE, "ndp_loop_bounds.npz")


def measure(c):
    levels, x = ref.make_warp_case(c)
    _, data = oracle.ndp_warp(levels, x)
    want = [data[i] for i in range(len(levels))]
    return ref.warp_errors(ref.mirror_warp(levels, x), want)


def main():
    rec = {c["name"]: np.array(measure(c)) for c in ref.WARP_CASES}
    fx = max(v[0] for v in rec.values())
    fs = max(v[1] for v in rec.values())
    np.savez(OUT, floor_xyz=np.float64(fx), floor_s=np.float64(fs), **rec)
    worst = sorted(rec, key=lambda n: -rec[n][0])[:3]
    print(f"floor_xyz {fx:.3e}  floor_s {fs:.3e}  largest: " + ", ".join(f"{n} {rec[n][0]:.2e}" for n in worst))


if __name__ == "__main__":
    main()
