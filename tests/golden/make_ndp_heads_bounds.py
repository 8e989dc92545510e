"""Record the f32 noise floor of one NDP level step for the eight heads beyond
SE3 / axis_angle: tests/golden/ndp_heads_bounds.npz.

For every case of tests/ndp_heads_ref.py (CASES) run f32 torch autograd of
ndp_opt.NDPLayer on the CPU and measure it against the f64 restatement
(ndp_heads_ref.level_step): per tensor group, the largest |f32 - f64| relative
to the largest |entry| of that tensor in the f64 reference.  The GPU tests bound
the kernels by 4 x the pooled floor of each group (ndp_train_ref.bounds).  CPU
only; recorded numbers only.

Keys:
  cases (C) str, groups (G) str       row / column names of `floor`
  floor (C, G) f64                    the f32-autograd error of each case and group
                                      (0 for a group the case's head does not have)
  min_preact (C) f64                  the f64 minimum |pre-activation| (>= GUARD)
  min_norm (C) f64                    the smallest norm a normalising format divides
                                      by (inf for euler and sflow; >= NORM_GUARD)

    python tests/golden/make_ndp_heads_bounds.py            # writes the file
    python tests/golden/make_ndp_heads_bounds.py --seeds    # lists guard-holding seeds
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import ndp_heads_ref as ref  # noqa: E402

OUT = os.path.join(HERE, "ndp_heads_bounds.npz")


def measure(c):
    d = ref.make_case(c)
    want = ref.level_step(d["P"], d["x"], d["g"], d["bce_scale"])
    L = ref.make_layer(d["P"], torch.float32)
    got = ref.autograd_step(L, torch.from_numpy(d["x"]), torch.from_numpy(d["g"]), d["bce_scale"])
    return ref.group_errors(got, want, c["motion"], c["rotation_format"]), want


def seeds():
    for i, c in enumerate(ref.CASES):
        s = 100 * i
        while True:
            d = ref.make_case(dict(c, seed=s))
            want = ref.level_step(d["P"], d["x"], d["g"], d["bce_scale"])
            if ref.guards_hold(want):
                break
            s += 1
        note = "" if s == c["seed"] else f"   <-- SEED_BUMP[{c['name']!r}] = {s - 100 * i}"
        print(f"{c['name']:24s} seed {s:5d} (listed {c['seed']:5d}) min|preact| {want['min_preact']:.3e}{note}")


def main():
    cases = ref.CASES
    floor = np.zeros((len(cases), len(ref.GROUPS)))
    mp, mn = np.zeros(len(cases)), np.zeros(len(cases))
    for i, c in enumerate(cases):
        err, want = measure(c)
        floor[i] = [err.get(g, 0.0) for g in ref.GROUPS]
        mp[i], mn[i] = want["min_preact"], min(want["norms"].values(), default=np.inf)
        assert ref.guards_hold(want), (c["name"], mp[i], want["norms"])
    assert np.isfinite(floor).all()
    np.savez(OUT, cases=np.array([c["name"] for c in cases]), groups=np.array(ref.GROUPS),
             floor=floor, min_preact=mp, min_norm=mn)
    for j, g in enumerate(ref.GROUPS):
        print(f"{g:8s} floor {floor[:, j].max():.3e}")


if __name__ == "__main__":
    seeds() if "--seeds" in sys.argv[1:] else main()
