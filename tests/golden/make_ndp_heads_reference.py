"""Record what the reference's own NDPLayer computes for every head:
tests/golden/ndp_heads_reference.npz.

Run where the reference tree is present (PCR_REFERENCE, default /root/reference);
never run by a test.  For each of the nine (motion, rotation format) heads the
reference module (c2p-net/deformationpyramid/model/nets.py: NDPLayer) is built
in f64 with the parameters of the case generator (tests/ndp_heads_ref.py:
make_case of `fixture_case(head)`: 33 points, depth 3, level 1, so the
nonrigidity branch is there) and run once.  Nothing from the reference is
stored except these numbers.

Keys: heads (9) str; x_out (9, 33, 3) f64; nonrigidity (9, 33) f64.

    python tests/golden/make_ndp_heads_reference.py
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import ndp_heads_ref as ref  # noqa: E402

REF = os.environ.get("PCR_REFERENCE", "/root/reference")
OUT = os.path.join(HERE, "ndp_heads_reference.npz")


def main():
    sys.modules.setdefault("open3d", types.ModuleType("open3d"))
    sys.path.insert(0, f"{REF}/c2p-net/deformationpyramid")
    from model.nets import NDPLayer
    names, xs, nrs = [], [], []
    for motion, fmt in ref.HEADS:
        d = ref.make_case(ref.fixture_case(motion, fmt))
        P = d["P"]
        layer = NDPLayer(3, ref.WIDTH, P["k0"], P["m"], rotation_format=fmt, nonrigidity_est=True, motion=motion)
        layer.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in ref.state_dict_of(P).items()})
        with torch.no_grad():
            xo, nr = layer.double()(torch.from_numpy(d["x"]).double())
        names.append(ref.head_name(motion, fmt))
        xs.append(xo.numpy().reshape(33, 3))
        nrs.append(nr.numpy().reshape(33))
    np.savez(OUT, heads=np.array(names), x_out=np.stack(xs), nonrigidity=np.stack(nrs))
    print("wrote", OUT, [f"{n}: |x'| max {np.abs(x).max():.3f}" for n, x in zip(names, xs)])


if __name__ == "__main__":
    main()
