"""Record the f32 noise floor of one NDP level step: tests/golden/ndp_train_bounds.npz.

For every case of the GPU tests (tests/ndp_train_ref.py: CASES, and BIG_CASES of
test_ndp_train_gpu.py) run f32 torch autograd of ndp_opt.NDPLayer on the CPU and
measure it against the f64 restatement (ndp_train_ref.level_step): per tensor
group, the largest |f32 - f64| relative to the largest |entry| of that tensor
in the f64 reference.  The GPU tests bound the kernels by 4 x the pooled floor
of each group (ndp_train_ref.bounds).  CPU only; recorded numbers only.

Keys:
  cases (C) str, groups (G) str       row / column names of `floor`
  floor (C, G) f64                    the f32-autograd error of each case and group
  min_preact (C) f64                  the f64 minimum |pre-activation| (>= GUARD)

    python tests/golden/make_ndp_train_bounds.py            # writes the file
    python tests/golden/make_ndp_train_bounds.py --seeds    # lists guard-holding seeds
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import ndp_train_ref as ref  # noqa: E402

OUT = os.path.join(HERE, "ndp_train_bounds.npz")


def measure(c):
    d = ref.make_case(c)
    want = ref.level_step(d["P"], d["x"], d["g"], d["bce_scale"])
    L = ref.make_layer(d["P"], torch.float32)
    got = ref.autograd_step(L, torch.from_numpy(d["x"]), torch.from_numpy(d["g"]), d["bce_scale"])
    return ref.group_errors(got, want), want["min_preact"]


def seeds():
    for c in ref.CASES + ref.BIG_CASES:
        s = c["seed"]
        while True:
            d = ref.make_case(dict(c, seed=s))
            mp = ref.level_step(d["P"], d["x"], d["g"], d["bce_scale"])["min_preact"]
            if mp >= ref.GUARD:
                break
            s += 1
        print(f"{c['name']:10s} seed {s:5d} (listed {c['seed']:5d}) min|preact| {mp:.3e}")


def main():
    cases = ref.CASES + ref.BIG_CASES
    floor = np.zeros((len(cases), len(ref.GROUPS)))
    mp = np.zeros(len(cases))
    for i, c in enumerate(cases):
        err, mp[i] = measure(c)
        floor[i] = [err.get(g, 0.0) for g in ref.GROUPS]  # depth 1 has no hidden layer
        assert mp[i] >= ref.GUARD, (c["name"], mp[i])
    assert np.isfinite(floor).all()
    np.savez(OUT, cases=np.array([c["name"] for c in cases]), groups=np.array(ref.GROUPS),
             floor=floor, min_preact=mp)
    edge = floor[:len(ref.CASES)].max(0)
    for j, g in enumerate(ref.GROUPS):
        print(f"{g:8s} edge floor {edge[j]:.3e}  all {floor[:, j].max():.3e}")


if __name__ == "__main__":
    seeds() if "--seeds" in sys.argv[1:] else main()
