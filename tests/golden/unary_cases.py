"""Seeded inputs of the unary golden (tests/golden/unary_golden.npz holds only what
the reference returned for them; make_golden_unary.py records it, test_unary_cpu.py
and test_unary_blocks_gpu.py read it).  Shapes are the smallest that still have
every tail: widths that are no multiple of 2, 4 or 32, an odd concat seam, rows
one past and one short of a 64-row tile.

  UNARY   UnaryBlock: (n, cin, cout, use_bn, relu)
  UPCAT   NearestUpsampleBlock + torch.cat + UnaryBlock: (m0, n, c0, c1, cout, use_bn, relu)
  BLOCKS  SimpleBlock / ResnetBottleneckBlock: (kind, in_dim, out_dim, use_bn); n queries
          among m supports, k neighbour columns, K kernel points
  NET     the tiny network of the wiring test: the MRI architecture's decoder at
          small widths behind a stub encoder
"""
import numpy as np

SEED = 20241021
SLOPE = 0.1
EPS = 1e-5

UNARY = {
    "bn_relu": (65, 129, 34, True, True),
    "bn": (63, 33, 17, True, False),
    "bias_relu": (64, 7, 5, False, True),
    "bias": (130, 3, 34, False, False),
}
UPCAT = {
    "seam_odd": (40, 129, 35, 20, 18, True, True),   # the seam inside a k-pair
    "last": (30, 70, 18, 9, 6, False, False),        # last_unary: bias, no activation
}
BLOCKS = {
    "simple": ("simple", 1, 16, True),
    "simple_bias": ("simple", 3, 10, False),
    "resnet_id": ("resnetb", 16, 16, True),                  # identity shortcut
    "resnet_proj": ("resnetb", 4, 16, True),                 # unary1 an Identity, projected shortcut
    "resnet_strided_id": ("resnetb_strided", 12, 12, True),  # max-pooled identity shortcut
    "resnet_strided_proj": ("resnetb_strided", 8, 20, True),
}
BLOCK_GEOMETRY = dict(m=90, n_strided=41, k=12, K=15, radius=0.3)


def _rng(kind, name):
    names = sorted(list(UNARY) + list(UPCAT) + list(BLOCKS) + ["net"])
    return np.random.default_rng((SEED, ("unary", "upcat", "block", "net").index(kind), names.index(name)))


def _weight(rng, cout, cin):
    return (rng.standard_normal((cout, cin)) / np.sqrt(cin)).astype(np.float32)


def make_unary(name):
    """-> dict(x (n, cin), w (cout, cin), bias (cout,) or None)."""
    n, cin, cout, use_bn, relu = UNARY[name]
    rng = _rng("unary", name)
    return dict(x=rng.standard_normal((n, cin)).astype(np.float32), w=_weight(rng, cout, cin),
                bias=None if use_bn else rng.standard_normal(cout).astype(np.float32))


def make_upcat(name):
    """-> dict(x0 (m0, c0), up (n, 3) int64: the up-sampling table whose column 0 is used, x1 (n, c1),
    w (cout, c0 + c1), bias or None)."""
    m0, n, c0, c1, cout, use_bn, relu = UPCAT[name]
    rng = _rng("upcat", name)
    return dict(x0=rng.standard_normal((m0, c0)).astype(np.float32), up=rng.integers(0, m0, (n, 3)).astype(np.int64),
                x1=rng.standard_normal((n, c1)).astype(np.float32), w=_weight(rng, cout, c0 + c1),
                bias=None if use_bn else rng.standard_normal(cout).astype(np.float32))


def make_block(name):
    """-> dict(batch: points [supports, queries], neighbors [(m, k)], pools [(n, k)] (pad = m);
    f (m, in_dim); kp (K, 3); extent; params: the block's state dict as numpy)."""
    kind, in_dim, out_dim, use_bn = BLOCKS[name]
    g = BLOCK_GEOMETRY
    m, k, K, radius = g["m"], g["k"], g["K"], g["radius"]
    rng = _rng("block", name)
    s = rng.random((m, 3)).astype(np.float32)
    q = s[rng.permutation(m)[:g["n_strided"]]] + (0.02 * rng.standard_normal((g["n_strided"], 3))).astype(np.float32)

    def near(qq):
        d2 = ((qq[:, None].astype(np.float64) - s[None].astype(np.float64)) ** 2).sum(-1)
        order = np.argsort(d2, axis=1, kind="stable")[:, :k]
        return np.where(np.take_along_axis(d2, order, 1) <= radius * radius, order, m).astype(np.int64)

    f = np.abs(rng.standard_normal((m, in_dim))).astype(np.float32) + np.float32(0.05)
    kp = rng.standard_normal((K, 3))
    kp = kp / np.linalg.norm(kp, axis=1, keepdims=True) * rng.random((K, 1)) ** (1 / 3) * 0.66 * radius
    kp[0] = 0.0
    mid = out_dim // 2 if kind == "simple" else out_dim // 4
    conv_in = in_dim if kind == "simple" else mid
    p = {"KPConv.weights": (rng.standard_normal((K, conv_in, mid)) / np.sqrt(K * conv_in)).astype(np.float32),
         "KPConv.kernel_points": kp.astype(np.float32)}
    if not use_bn:
        p["bn.bias"] = rng.standard_normal(mid).astype(np.float32)
    if kind != "simple":
        if in_dim != mid:
            p["unary1.mlp.weight"] = _weight(rng, mid, in_dim)
        p["unary2.mlp.weight"] = _weight(rng, out_dim, mid)
        if in_dim != out_dim:
            p["unary_shortcut.mlp.weight"] = _weight(rng, out_dim, in_dim)
    return dict(batch=dict(points=[s, q], neighbors=[near(s)], pools=[near(q)]), f=f, kp=kp.astype(np.float32),
                extent=float(np.float32(0.5 * radius)), params=p)


# ---- the tiny network ---------------------------------------------------------------------
NET = dict(first=8, gnn=14, final=6, lengths=((70, 60), (40, 35), (22, 20), (12, 10)), k=4)
ENCODER_SKIPS = [2, 5, 8]
DECODER_SKIPS = [12, 14, 16]


def encoder_plan():
    """The stub encoder: per block ("unary", in, out) or ("pool", layer_ind), pools at ENCODER_SKIPS.  The
    widths before the pools are first, 2 first, 4 first, the last width 8 first, as the architecture's."""
    f = NET["first"]
    return [("unary", 1, f // 2), ("unary", f // 2, f), ("pool", 0), ("unary", f, 2 * f), ("unary", 2 * f, 2 * f),
            ("pool", 1), ("unary", 2 * f, 4 * f), ("unary", 4 * f, 4 * f), ("pool", 2), ("unary", 4 * f, 8 * f),
            ("unary", 8 * f, 8 * f)]


def decoder_plan(first=None, gnn=None):
    """The three decoder lists of the MRI architecture (nearest_upsample, unary, nearest_upsample, unary,
    nearest_upsample, last_unary) as block_decider's arguments: per branch a list of
    (block_name, in_dim, out_dim, layer_ind); out_dim -1 on a last_unary: final feats without the two scores.
    With first = 128, gnn = 256 the h branch is 770 -> 129, 385 -> 64, 192 -> 34.  Default: NET's widths."""
    f, g = first or NET["first"], (gnn or NET["gnn"]) + 2
    s = [f, 2 * f, 4 * f]                       # the skips' widths
    d1, d2, d3 = g // 2, g // 4, g // 8
    up = lambda l, d: ("nearest_upsample", d, d, l)  # noqa: E731
    h = [up(2, g), ("unary", g + s[2], d1, 2), up(1, d1), ("unary", d1 + s[1], d2, 1), up(0, d2),
         ("last_unary", d2 + s[0], d3, 0)]
    m = [("unary", s[2], d1, 2), up(1, d1), ("unary", d1 + s[1], d2, 1), up(0, d2), ("last_unary", d2 + s[0], -1, 0)]
    lo = [("unary", s[1], d2, 1), up(0, d2), ("last_unary", d2 + s[0], -1, 0)]
    return h, m, lo


def _out_width(name, out_dim):
    if name != "last_unary":
        return out_dim
    return NET["final"] + (0 if out_dim == -1 else 2)


def make_net():
    """-> dict(inputs: the pyramid as numpy (points, normals, stacked_lengths, pools, upsamples, feats),
    params: the network's state dict as numpy)."""
    rng = _rng("net", "net")
    lengths, k = NET["lengths"], NET["k"]
    tot = [a + b for a, b in lengths]
    inputs = dict(points=[rng.random((n, 3)).astype(np.float32) for n in tot],
                  normals=[rng.standard_normal((n, 3)).astype(np.float32) for n in tot],
                  stacked_lengths=[np.asarray(l, np.int64) for l in lengths],
                  feats=rng.standard_normal((tot[0], 1)).astype(np.float32),   # not the network's ones: the stub's
                  pools=[], upsamples=[], neighbors=[])                        # first block is a Linear, not a KPConv
    for l in range(3):
        pool = rng.integers(0, tot[l], (tot[l + 1], k))
        pool[rng.random(pool.shape) < 0.2] = tot[l]          # pads
        pool[:, 0] = rng.integers(0, tot[l], tot[l + 1])     # every row keeps a real neighbour
        inputs["pools"].append(pool.astype(np.int64))
        inputs["upsamples"].append(rng.integers(0, tot[l + 1], (tot[l], k)).astype(np.int64))
    p = {}
    for i, blk in enumerate(encoder_plan()):
        if blk[0] == "unary":
            p[f"encoder_blocks.{i}.mlp.weight"] = _weight(rng, blk[2], blk[1])
    g, last = NET["gnn"], encoder_plan()[-1][2]
    for name, co, ci in (("bottleneck", g, last), ("info_interative.a", g, g), ("info_interative.b", g, g),
                         ("pro_gnn", g, g), ("attn_score", 1, g)):
        p[f"{name}.weight"] = _weight(rng, co, ci)[:, :, None]
        p[f"{name}.bias"] = (0.1 * rng.standard_normal(co)).astype(np.float32)
    p["epsilon"] = np.float32(-1.0)
    for lst, plan in zip(("decoder_blocks", "decoder_blocks_m", "decoder_blocks_l"), decoder_plan()):
        for i, (name, cin, cout, _l) in enumerate(plan):
            if name == "nearest_upsample":
                continue
            p[f"{lst}.{i}.mlp.weight"] = _weight(rng, _out_width(name, cout), cin)
            if name == "last_unary":
                p[f"{lst}.{i}.bn.bias"] = (0.5 * rng.standard_normal(_out_width(name, cout))).astype(np.float32)
    return dict(inputs=inputs, params=p)
