"""The cases of pcr_pointwise_forward and of the ropnet modules: shapes and seeds
only.  Inputs, weights and module parameters are regenerated from the seeds by
the functions below (numpy's generator, so every machine makes the same
arrays); tests/golden/ropnet_golden.npz holds only what the reference returned
for them (make_golden_ropnet.py).

KERNEL  name -> dict(b, n, widths, sub, cout, groups, bias, cbias, act, slope, res)
  widths: channels per source; sub: per source, whether a tensor is subtracted.
POINTNET / CG / OA / NET: the module cases, see each table.
"""
import zlib

import numpy as np

EPS = 1e-5


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def _k(b=2, n=65, widths=(6,), sub=None, cout=48, groups=0, bias=False, cbias=False, act=False, slope=0.0,
       res=False):
    return dict(b=b, n=n, widths=tuple(widths), sub=tuple(sub) if sub else (False,) * len(widths), cout=cout,
                groups=groups, bias=bias, cbias=cbias, act=act, slope=slope, res=res)


KERNEL = {}
# every point count, with a norm of group width 24 (n = 1 included); 4 | 5 is where pass 1 leaves the VALU path
for _n in (1, 2, 4, 5, 63, 64, 65, 129):
    KERNEL[f"n{_n}"] = _k(n=_n, cout=48, groups=2, act=True, slope=0.2, res=True)
for _b in (1, 3):
    KERNEL[f"b{_b}"] = _k(b=_b, widths=(33,), cout=7, bias=True)
for _c in (3, 6, 33):                    # 3: a k-pair tail
    KERNEL[f"cin{_c}"] = _k(widths=(_c,), cout=129)
# two seams inside a k-pair (5 | 6, 6 | 7 .. ), sub on one source only; group width 32
KERNEL["seams"] = _k(n=129, widths=(5, 1, 32), sub=(False, False, True), cout=192, groups=6, act=True, res=True)
KERNEL["cout2"] = _k(cout=2, bias=True, act=True)
KERNEL["cout7"] = _k(cout=7, widths=(33,), cbias=True, act=True, slope=0.2)
KERNEL["cout129"] = _k(n=129, cout=129, widths=(33,), sub=(True,), bias=True, cbias=True, res=True)
KERNEL["cout192"] = _k(n=129, b=3, cout=192, groups=4, act=True, slope=0.2)          # group width 48
KERNEL["bias"] = _k(b=3, widths=(33,), cout=7, bias=True)
KERNEL["cbias"] = _k(b=3, widths=(33,), cout=7, cbias=True)
KERNEL["both"] = _k(b=3, widths=(33,), cout=7, bias=True, cbias=True)
KERNEL["bias_norm"] = _k(b=3, widths=(33,), cout=48, groups=2, bias=True, cbias=True, act=True)
KERNEL["fuse5"] = _k(n=129, widths=(32,) * 5, cout=160, groups=20, act=True, slope=0.2)   # conv_fuse at dim 32
KERNEL["wide3072"] = _k(n=1, widths=(1536, 1536), cout=192, bias=True, act=True)      # decoder_qt's first layer
KERNEL["wide4608"] = _k(n=1, widths=(1536, 1536, 1536), sub=(False, False, True), cout=192, bias=True)  # cloud bias


def weight(rng, cout, cin):
    return (rng.standard_normal((cout, cin)) / np.sqrt(cin)).astype(np.float32)


def affine(rng, c):
    g = rng.uniform(-1.5, 1.5, c).astype(np.float32)
    g[::5] = 0.0
    return g, rng.uniform(-0.5, 0.5, c).astype(np.float32)


def make_kernel(name):
    """The arrays of a KERNEL case (f32): sources, subs (None where none), w, bias, cbias, gamma, beta, res."""
    k = KERNEL[name]
    rng = _rng("kernel", name)
    b, n, cout = k["b"], k["n"], k["cout"]
    d = dict(k)
    d["sources"] = [rng.standard_normal((b, c, n)).astype(np.float32) for c in k["widths"]]
    d["subs"] = [rng.standard_normal((b, c, n)).astype(np.float32) if s else None
                 for c, s in zip(k["widths"], k["sub"])]
    d["w"] = weight(rng, cout, sum(k["widths"]))
    d["bias_v"] = rng.standard_normal(cout).astype(np.float32) if k["bias"] else None
    d["cbias_v"] = rng.standard_normal((b, cout)).astype(np.float32) if k["cbias"] else None
    d["gamma"], d["beta"] = affine(rng, cout) if k["groups"] else (None, None)
    d["res_v"] = rng.standard_normal((b, cout, n)).astype(np.float32) if k["res"] else None
    return d


# ---- module cases ------------------------------------------------------------------------

# name -> (in_dim, gn, out_dims, cls, b, n)
POINTNET = {
    "plain": (3, False, (24, 48), False, 2, 65),
    "gn": (3, True, (24, 48), False, 2, 65),
    "cls": (6, False, (24, 7), True, 2, 65),
    "gn_cls": (6, True, (24, 48, 16), True, 2, 65),
}
# the real widths: encoder 3 -> 192 -> 192 -> 192 -> 384 -> 1536, decoder_ol 6144 -> 1536 -> 1536 -> 768 -> 2,
# decoder_qt 3072 -> 1536 -> 1536 -> 768 -> 7
CG = {"b": 2, "n": 65, "m": 70}
# name -> (dim, b, n)
OA = {"d32": (32, 2, 65), "d192": (192, 1, 65)}
NET = dict(feat_dim=32, num_neighbors=16, radius=0.3, N1=48, M1=56, top_prob=0.4, topk=1, b=2, n=96, num_iter=2,
           use_ppf=True)
NET_SEEDS = range(40)    # make_golden_ropnet.py searches these for the sort-gap conditions; NET_SEED is its find
NET_SEED = 4
GAP_FACTOR = 100


def params(module, *key):
    """A state dict for `module` (any torch module) from a seed: conv / linear weights N(0, 1 / fan_in),
    biases N(0, 0.1^2), norm weights in (0.5, 1.5), norm biases N(0, 0.1^2), each from its own name's seed.
    Tied parameters (q_conv / k_conv) get one array."""
    import torch
    sd, seen = {}, {}
    norms = {n for n, m in module.named_modules() if isinstance(m, torch.nn.GroupNorm)}
    for name, p in module.state_dict(keep_vars=True).items():
        if id(p) in seen:
            sd[name] = sd[seen[id(p)]]
            continue
        seen[id(p)] = name
        owner, leaf = name.rsplit(".", 1) if "." in name else ("", name)
        rng = _rng("params", *key, name)      # per name: the arrays do not depend on the keys' order
        shape = tuple(p.shape)
        if owner in norms:
            a = rng.uniform(0.5, 1.5, shape) if leaf == "weight" else 0.1 * rng.standard_normal(shape)
        elif leaf == "weight":
            a = rng.standard_normal(shape) / np.sqrt(max(1, int(np.prod(shape[1:]))))
        else:
            a = 0.1 * rng.standard_normal(shape)
        sd[name] = torch.from_numpy(a.astype(np.float32))
    return sd


def cloud(b, n, *key, normals=False):
    """(b, n, 3) points in the unit cube's scale (or (b, n, 6) with unit normals)."""
    rng = _rng("cloud", *key)
    p = rng.uniform(-0.5, 0.5, (b, n, 3)).astype(np.float32)
    if not normals:
        return p
    v = rng.standard_normal((b, n, 3))
    return np.concatenate([p, (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(np.float32)], -1)


def pointnet_input(name):
    """x (b, in_dim, n) of a POINTNET case."""
    in_dim, _, _, _, b, n = POINTNET[name]
    return np.ascontiguousarray(_rng("pointnet", name).uniform(-0.5, 0.5, (b, n, in_dim)).astype(np.float32)
                                .transpose(0, 2, 1))


def cg_inputs(m=None):
    """src (b, n, 3), tgt (b, m or n, 3) of the CG case."""
    return cloud(CG["b"], CG["n"], "cg", "src"), cloud(CG["b"], m or CG["n"], "cg", "tgt", m)


def oa_input(name):
    dim, b, n = OA[name]
    return _rng("oa", name).standard_normal((b, dim, n)).astype(np.float32)


def net_inputs(seed):
    """src, tgt (b, n, 6) of the tiny network: tgt is src moved rigidly, reordered and jittered, so that the
    overlap and similarity scores are those of a registration problem."""
    rng = _rng("net", seed)
    b, n = NET["b"], NET["n"]
    src = cloud(b, n, "net", seed, normals=True)
    ang = rng.uniform(-0.4, 0.4, (b, 3))
    out = np.empty_like(src)
    for i in range(b):
        cx, cy, cz = np.cos(ang[i])
        sx, sy, sz = np.sin(ang[i])
        rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
        ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
        rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
        r = rz @ ry @ rx
        perm = rng.permutation(n)
        out[i, :, :3] = (src[i, perm, :3] @ r.T + rng.uniform(-0.2, 0.2, 3) + 0.005 * rng.standard_normal((n, 3)))
        out[i, :, 3:] = src[i, perm, 3:] @ r.T
    return src, out.astype(np.float32)
