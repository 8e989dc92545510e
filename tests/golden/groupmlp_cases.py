"""The inputs and weights of tests/golden/groupmlp_golden.npz, regenerated from
seeds: the npz holds only what the reference returned.

GCN cases run the reference's whole ``GCN.forward`` (and ``GGE`` is ``GCN`` next
to ``PPF``; its two halves are pinned separately).  MLP cases run the
reference's own ``LocalFeatureFused`` -- taken from inside a reference ``PPF``
(InstanceNorm2d) or a ROPNet ``LocalFeatue`` (GroupNorm with affine) -- on the
group the library's front end produces (tests/grouping_ref.py restates it on
the CPU), so that what is pinned is the MLP and not the front end's roundings,
which tests/test_grouping_*.py pin.

Clouds are uniform in [-1, 1]^3 (floats, no exact ties): their k-NN sets equal
the library order's; make_golden_groupmlp.py asserts it.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import grouping_ref as gr  # noqa: E402

SEED = 20241020
EPS = 1e-5
GCN_SLOPE = 0.2

# name -> (B, N, feats_dim, k)
GCN_CASES = {"gcn32": (2, 129, 32, 10), "gcn_small": (1, 7, 32, 10)}

# name -> (kind, B, N, K, radius, widths); kind "ppf": NgeNet PPF (instance norm, normals);
# "rop10" / "rop6": ROPNet LocalFeatue with / without normals (group norm, affine)
MLP_CASES = {
    "ppf": ("ppf", 2, 70, 16, 0.6, (32, 64, 32)),
    "ppf_wide": ("ppf", 1, 40, 32, 0.8, (256, 512, 256)),
    "ppf_bottleneck": ("ppf", 1, 33, 8, 0.5, (128, 256, 128)),
    "rop10": ("rop10", 2, 70, 16, 0.6, (32, 64, 32)),
    "rop6_wide": ("rop6", 1, 40, 32, 0.8, (256, 512, 192)),
}


def _rng(*key):
    return np.random.default_rng((SEED,) + tuple(int.from_bytes(str(k).encode(), "little") % (2 ** 32) for k in key))


def weight(rng, out, inp):
    return (rng.standard_normal((out, inp)) / np.sqrt(inp)).astype(np.float32)


def gcn_case(name):
    """coords (B, 3, N), feats (B, C, N), conv1 (C, 2C), conv2 (2C, 2C), conv3 (C, 4C), k."""
    b, n, c, k = GCN_CASES[name]
    rng = _rng("gcn", name)
    coords = rng.uniform(-1, 1, (b, 3, n)).astype(np.float32)
    feats = rng.standard_normal((b, c, n)).astype(np.float32)
    return {"coords": coords, "feats": feats, "conv1": weight(rng, c, 2 * c), "conv2": weight(rng, 2 * c, 2 * c),
            "conv3": weight(rng, c, 4 * c), "k": k}


def affine(rng, c):
    """GroupNorm gamma with negative, zero and positive entries, and beta."""
    gamma = rng.uniform(-1.5, 1.5, c).astype(np.float32)
    gamma[::7] = 0.0
    gamma[1] = -0.75
    gamma[2] = 1.25
    return gamma, rng.uniform(-0.5, 0.5, c).astype(np.float32)


def mlp_case(name):
    """xyz, normals (B, N, 3) (normals None for rop6), x (B, N, K, cin) the library's group, weights
    [(c_l, c_{l-1})], gammas, betas (None entries for instance norm), norm, radius, K."""
    kind, b, n, k, radius, widths = MLP_CASES[name]
    rng = _rng("mlp", name)
    xyz = rng.uniform(-1, 1, (b, n, 3)).astype(np.float32)
    nrm = rng.standard_normal((b, n, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=-1, keepdims=True)).astype(np.float32)
    normals = None if kind == "rop6" else nrm
    idx, count = gr.ball_query(xyz, xyz, radius, k)
    assert count.min() >= 1   # a point is its own neighbour
    x = gr.group_ppf(xyz, normals, idx).astype(np.float32)
    cin = x.shape[-1]
    weights, gammas, betas, prev = [], [], [], cin
    for c in widths:
        weights.append(weight(rng, c, prev))
        g, be = affine(rng, c) if kind != "ppf" else (None, None)
        gammas.append(g)
        betas.append(be)
        prev = c
    return {"xyz": xyz, "normals": normals, "x": x, "weights": weights, "gammas": gammas, "betas": betas,
            "norm": "instance" if kind == "ppf" else "group", "radius": radius, "K": k, "kind": kind}
