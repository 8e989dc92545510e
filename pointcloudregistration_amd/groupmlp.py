"""What consumes the grouping front ends, fused for inference: the edge conv of
NgeNet's ``GCN`` and the grouped local-feature MLP behind NgeNet's ``PPF`` and
ROPNet's ``LocalFeatue``.  No ``(B, N, k, 2C)`` or ``(B, C, K, N)`` tensor exists
in global memory.

Mirrors of pcr_edge_conv / pcr_group_mlp (contract in include/pcr_api.h, f64
restatement with the derived bounds in tests/groupmlp_ref.py):

* ``edge_conv``  -- ``Conv2d(2C -> C', bias=False) -> InstanceNorm2d ->
  LeakyReLU -> max over k`` on ``get_graph_features``' tensor, without that
  tensor (c2p-net/ngenet/models/information_interactive.py:107-130);
* ``group_mlp``  -- one to three ``Conv2d 1x1 (bias=False) -> InstanceNorm2d or
  GroupNorm(c // 32, c) -> ReLU`` and the max over the K group members
  (``LocalFeatureFused``: information_interactive.py:26-45, ROPNet/src/models/TFMR.py:17-37);
* ``GCN`` / ``PPF`` / ``LocalFeature`` -- the three modules with the
  reference's forward signature and return layout around the SAME submodules
  as an existing block; ``fuse(model)`` swaps a loaded network's blocks in place.

Both norms take their statistics over the whole cloud, in train and eval mode
alike, so nothing is folded: the weights are read where they are, parameters
stay shared and nothing needs a refresh.

f32, CUDA tensors only (no CPU path), forward only: an input or parameter that
requires grad under grad mode raises.  Two calls return the same bytes, and a
cloud's bytes do not depend on the batch it is in.
"""
from __future__ import annotations

import ctypes

import torch

from . import _front, _lib, grouping

__all__ = ["edge_conv", "group_mlp", "GCN", "PPF", "LocalFeature", "fuse", "MAX_WIDTH", "MAX_GROUP",
           "MAX_GROUP_CHANNELS", "MAX_NEIGHBOURS"]

MAX_WIDTH = 512            # pcr_api.h
MAX_GROUP = 128            # K
MAX_GROUP_CHANNELS = 16    # cin
MAX_NEIGHBOURS = 63        # kk
_MAX_POINTS = 1 << 20
_MAX_BATCH = 65535
_STAGES = {"edge": ("rq", "stats"), "mlp": ("y1", "y2", "y3", "stats1", "stats2", "stats3")}


def _width(name, c):
    if c < 32 or c > MAX_WIDTH or c % 32:
        raise ValueError(f"{name}={c}: widths must be multiples of 32 in 32..{MAX_WIDTH}")


def _sizes(b, n):
    if b > _MAX_BATCH:
        raise ValueError(f"B={b} above {_MAX_BATCH}")
    if not 2 <= n <= _MAX_POINTS:
        raise ValueError(f"N={n} outside 2..{_MAX_POINTS}: the norm needs at least two points")


def _conv_weight(w, name, dev):
    """(out, in) view of a Conv2d / Conv1d 1x1 weight or a matrix, on its own storage."""
    w = _front.tensor(w, name, "(out, in)", None, dev)
    if w.dim() > 2:
        if any(s != 1 for s in w.shape[2:]):
            raise ValueError(f"{name}: only 1x1 kernels, got {tuple(w.shape)}")
        w = w.reshape(w.shape[0], w.shape[1])
    if w.dim() != 2:
        raise ValueError(f"{name} must be (out, in), got {tuple(w.shape)}")
    return w.contiguous()


def edge_conv(feats, inds, weight, slope=0.2, eps=1e-5, channels_first=False, want=()):
    """max over the neighbours of ``lrelu(instance_norm(W [f_i ; f_j - f_i]))``.

    feats ``(B, N, C)``, or ``(B, C, N)`` with ``channels_first`` (taken by
    stride either way, no copy); inds ``(B, N, kk)`` integers in ``[0, N)``, e.g.
    from ``grouping.knn_graph``, ``1 <= kk <= 63``; weight ``(C', 2C)`` (a
    Conv2d 1x1 weight goes in as it is).  Returns ``(B, N, C')``, or
    ``(B, C', N)`` with ``channels_first``.  C, C' multiples of 32, at most 512.
    want: names among "rq" ``(B, N, 2C')`` (``R = P - Q | Q``) and "stats"
    ``(B, C', 2)`` f64 (mean, var), appended to the result."""
    _front.forward_only("groupmlp.edge_conv", feats, weight)
    f = _front.tensor(feats, "feats", "(B, C, N)" if channels_first else "(B, N, C)", 3)
    dev = f.device
    if channels_first:
        f = f.transpose(1, 2)
    b, n, c = f.shape
    w = _conv_weight(weight, "weight", dev)
    co = w.shape[0]
    if w.shape[1] != 2 * c:
        raise ValueError(f"weight {tuple(w.shape)} must be (C', 2C = {2 * c})")
    _width("C", c)
    _width("C'", co)
    _sizes(b, n)
    if not isinstance(inds, torch.Tensor) or inds.dtype.is_floating_point or inds.dtype == torch.bool:
        raise ValueError("inds must be an integer tensor")
    if inds.dim() != 3 or tuple(inds.shape[:2]) != (b, n) or inds.device != dev:
        raise ValueError(f"inds must be ({b}, {n}, kk) on feats' device, got {tuple(inds.shape)}")
    kk = inds.shape[2]
    if not 1 <= kk <= MAX_NEIGHBOURS:
        raise ValueError(f"kk={kk} outside 1..{MAX_NEIGHBOURS}")
    want = _front.wanted(want, _STAGES["edge"])
    idx = inds.to(torch.int32).contiguous()
    out = torch.empty((b, co, n) if channels_first else (b, n, co), dtype=torch.float32, device=dev)
    shapes = {"rq": ((b, n, 2 * co), torch.float32), "stats": ((b, co, 2), torch.float64)}
    outs = {k: torch.empty(shapes[k][0], dtype=shapes[k][1], device=dev) for k in want}
    if b:
        lib = _lib.load()
        with torch.cuda.device(dev):
            ws = _front.scratch(lib.pcr_edge_conv_scratch_bytes(b, n, kk, c, co), dev)
            _lib.call("pcr_edge_conv", _lib.ptr(f), f.stride(0), f.stride(1), f.stride(2), _lib.ptr(idx), b, n, kk,
                      c, co, _lib.ptr(w), float(eps), float(slope), 1 if channels_first else 0, _lib.ptr(out),
                      _lib.ptr(outs.get("rq")), _lib.ptr(outs.get("stats")), _lib.ptr(ws), _lib.stream_handle(dev))
    if want:
        return (out,) + tuple(outs[k] for k in want)
    return out


def group_mlp(x, weights, norm="instance", gammas=None, betas=None, eps=1e-5, slope=0.0, channels_first=True,
              want=()):
    """``max_K act(norm(W_L ... act(norm(W_1 x))))`` for groups x ``(B, N, K, cin)``.

    x is channels last (``grouping.local_ppf_features(..., channels_first=False)``),
    ``1 <= K <= 128``, ``1 <= cin <= 16``; weights: one to three ``(c_l, c_{l-1})``
    matrices or Conv2d 1x1 weights, no bias, widths multiples of 32 up to 512;
    norm "instance" (per channel) or "group" (32 consecutive channels, the
    references' ``GroupNorm(c // 32, c)``); gammas / betas: per layer a ``(c_l,)``
    tensor or None.  Returns ``(B, c_L, N)`` (``channels_first``, the references'
    layout) or ``(B, N, c_L)``.  want: names among "y1".."y3" ``(B, N, K, c_l)``
    (pre-norm activations) and "stats1".."stats3" ``(B, c_l or c_l // 32, 2)`` f64
    (mean, var), appended to the result."""
    weights = list(weights)
    nl = len(weights)
    if not 1 <= nl <= 3:
        raise ValueError(f"{nl} layers: one to three are built")
    gammas = list(gammas) if gammas is not None else [None] * nl
    betas = list(betas) if betas is not None else [None] * nl
    if len(gammas) != nl or len(betas) != nl:
        raise ValueError("gammas and betas must have one entry (a tensor or None) per layer")
    _front.forward_only("groupmlp.group_mlp", x, *weights, *gammas, *betas)
    if norm not in ("instance", "group"):
        raise ValueError(f"norm={norm!r}: 'instance' or 'group'")
    group = 1 if norm == "instance" else 32
    xt = _front.tensor(x, "x", "(B, N, K, cin)", 4).contiguous()
    dev = xt.device
    b, n, k, cin = xt.shape
    _sizes(b, n)
    if not 1 <= k <= MAX_GROUP:
        raise ValueError(f"K={k} outside 1..{MAX_GROUP}")
    if not 1 <= cin <= MAX_GROUP_CHANNELS:
        raise ValueError(f"cin={cin} outside 1..{MAX_GROUP_CHANNELS}")
    want = _front.wanted(want, _STAGES["mlp"])
    net = _lib.GroupMlpNet()
    net.layers = nl
    keep, widths, prev = [], [], cin
    for i in range(nl):
        w = _conv_weight(weights[i], f"weights[{i}]", dev)
        if w.shape[1] != prev:
            raise ValueError(f"weights[{i}] {tuple(w.shape)} must take {prev} inputs")
        _width(f"width of layer {i + 1}", w.shape[0])
        prev = w.shape[0]
        widths.append(prev)
        keep.append(w)
        net.width[i] = prev
        net.w[i] = w.data_ptr()
        for arr, src, what in ((net.gamma, gammas[i], "gammas"), (net.beta, betas[i], "betas")):
            if src is not None:
                t = _front.tensor(src, f"{what}[{i}]", "(c,)", 1, dev).contiguous()
                if t.shape[0] != prev:
                    raise ValueError(f"{what}[{i}] has {t.shape[0]} entries, layer {i + 1} {prev} channels")
                keep.append(t)
                arr[i] = t.data_ptr()
    outs = {}
    for name in want:
        i = int(name[-1]) - 1
        if i >= nl:
            raise ValueError(f"want: {name} of a {nl}-layer call")
        if name[0] == "y":
            outs[name] = torch.empty((b, n, k, widths[i]), dtype=torch.float32, device=dev)
            net.y[i] = outs[name].data_ptr()
        else:
            outs[name] = torch.empty((b, widths[i] // group, 2), dtype=torch.float64, device=dev)
            net.stats[i] = outs[name].data_ptr()
    cl = widths[-1]
    out = torch.empty((b, cl, n) if channels_first else (b, n, cl), dtype=torch.float32, device=dev)
    if b:
        lib = _lib.load()
        c3 = widths + [0, 0]
        with torch.cuda.device(dev):
            ws = _front.scratch(lib.pcr_group_mlp_scratch_bytes(b, n, k, nl, c3[0], c3[1], c3[2]), dev)
            _lib.call("pcr_group_mlp", _lib.ptr(xt), b, n, k, cin, ctypes.byref(net), group, float(eps),
                      float(slope), 1 if channels_first else 0, _lib.ptr(out), _lib.ptr(ws),
                      _lib.stream_handle(dev))
    del keep
    if want:
        return (out,) + tuple(outs[name] for name in want)
    return out


# ---- the blocks' structure ---------------------------------------------------------------

def _cna(block, conv_type, norm_types, who):
    """(conv, norm, slope) of Sequential(conv 1x1 without bias, norm, ReLU or LeakyReLU); raises
    ValueError with the reason where the block is anything else."""
    nn = torch.nn
    mods = list(block.children()) if isinstance(block, nn.Sequential) else None
    if mods is None or len(mods) != 3:
        raise ValueError(f"{who}: expected Sequential(conv, norm, activation)")
    conv, norm, actv = mods
    if not isinstance(conv, conv_type) or any(s != 1 for s in conv.kernel_size) or conv.bias is not None \
            or conv.groups != 1:
        raise ValueError(f"{who}: the first layer must be a 1x1 {conv_type.__name__} without bias")
    if not isinstance(norm, norm_types):
        raise ValueError(f"{who}: the norm is a {type(norm).__name__}")
    if getattr(norm, "track_running_stats", False):
        raise ValueError(f"{who}: the norm tracks running statistics (eval mode would not use the cloud's own)")
    if isinstance(actv, nn.LeakyReLU):
        slope = float(actv.negative_slope)
    elif isinstance(actv, nn.ReLU):
        slope = 0.0
    else:
        raise ValueError(f"{who}: the activation is a {type(actv).__name__}")
    return conv, norm, slope


def _mlp_plan(fused, who):
    """The layers of a LocalFeatureFused (`blocks`: conv, norm, ReLU per layer) as the keyword
    arguments of group_mlp, the tensors being the parameters themselves."""
    nn = torch.nn
    blocks = getattr(fused, "blocks", None)
    mods = list(blocks.children()) if isinstance(blocks, nn.Sequential) else []
    if not mods or len(mods) % 3 or len(mods) > 9:
        raise ValueError(f"{who}.blocks: expected one to three (Conv2d, norm, ReLU) triples")
    weights, gammas, betas, kind, eps = [], [], [], None, None
    for i in range(0, len(mods), 3):
        conv, norm, slope = _cna(nn.Sequential(*mods[i:i + 3]), nn.Conv2d, (nn.InstanceNorm2d, nn.GroupNorm),
                                 f"{who}.blocks[{i}:{i + 3}]")
        if slope != 0.0:
            raise ValueError(f"{who}: LeakyReLU inside the MLP")
        k = "group" if isinstance(norm, nn.GroupNorm) else "instance"
        if k == "group" and norm.num_channels != 32 * norm.num_groups:
            raise ValueError(f"{who}: GroupNorm groups of {norm.num_channels // norm.num_groups} channels, only 32")
        if (kind, eps) != (None, None) and (kind, eps) != (k, norm.eps):
            raise ValueError(f"{who}: the layers' norms differ")
        kind, eps = k, norm.eps
        weights.append(conv.weight)
        gammas.append(getattr(norm, "weight", None))
        betas.append(getattr(norm, "bias", None))
    return dict(weights=weights, norm=kind, gammas=gammas, betas=betas, eps=eps, slope=0.0)


class GCN(torch.nn.Module):
    """The reference's GCN (information_interactive.py:87-130) with its two edge convs fused: the
    graph is built once (``grouping.knn_graph``), ``conv1`` and ``conv2`` run through
    ``edge_conv``, ``conv3`` (point-wise, no large intermediate) stays torch's.  Holds the same
    submodules as `like`: parameters and state-dict keys are shared."""

    def __init__(self, like):
        super().__init__()
        nn = torch.nn
        for name in ("conv1", "conv2"):
            _cna(getattr(like, name), nn.Conv2d, (nn.InstanceNorm2d,), f"GCN.{name}")
            if getattr(like, name)[1].affine:
                raise ValueError(f"GCN.{name}: an affine InstanceNorm2d is not built into edge_conv")
        self.conv1, self.conv2, self.conv3, self.k = like.conv1, like.conv2, like.conv3, like.k

    def _edge(self, block, feats, inds):
        conv, norm, slope = _cna(block, torch.nn.Conv2d, (torch.nn.InstanceNorm2d,), "GCN")
        return edge_conv(feats, inds, conv.weight, slope=slope, eps=norm.eps, channels_first=True)

    def forward(self, coords, feats):
        """coords (B, 3, N), feats (B, C, N) -> (B, C, N)."""
        inds = grouping.knn_graph(coords.permute(0, 2, 1), self.k)
        feats1 = self._edge(self.conv1, feats, inds)
        feats2 = self._edge(self.conv2, feats1, inds)
        return self.conv3(torch.cat([feats, feats1, feats2], dim=1))


class PPF(torch.nn.Module):
    """The reference's PPF (information_interactive.py:48-84): ``local_ppf_features`` into
    ``group_mlp``.  Holds `like`'s ``local_feature_fused``, so parameters are shared."""

    def __init__(self, like):
        super().__init__()
        _mlp_plan(like.local_feature_fused, "PPF.local_feature_fused")
        self.k, self.radius, self.local_feature_fused = like.k, like.radius, like.local_feature_fused

    def forward(self, coords, feats):
        """coords (B, 3, N), feats = normals (B, 3, N) -> (B, C, N)."""
        xyz = coords.permute(0, 2, 1)
        group = grouping.local_ppf_features(xyz, feats.permute(0, 2, 1), self.radius, min(self.k, xyz.shape[1]),
                                            channels_first=False)
        return group_mlp(group, **_mlp_plan(self.local_feature_fused, "PPF.local_feature_fused"))


class LocalFeature(torch.nn.Module):
    """ROPNet's LocalFeatue (TFMR.py:40-73), with normals (``use_ppf``, 10 channels) or without
    a feature (6): ``local_ppf_features`` into ``group_mlp``.  Holds `like`'s
    ``local_feature_fused``, so parameters are shared."""

    def __init__(self, like):
        super().__init__()
        _mlp_plan(like.local_feature_fused, "LocalFeatue.local_feature_fused")
        self.radius, self.K, self.local_feature_fused = like.radius, like.K, like.local_feature_fused

    def forward(self, feature, xyz, permute=False, use_ppf=False):
        """feature (B, N, 3) normals (or (B, 3, N) with `permute`), or None; xyz (B, N, 3)
        -> (B, C, N)."""
        if feature is not None:
            if permute:
                feature = feature.permute(0, 2, 1)
            if not use_ppf:
                raise ValueError("LocalFeature: a feature without use_ppf (raw grouped features as channels) "
                                 "is not built; pass feature=None or use_ppf=True")
        group = grouping.local_ppf_features(xyz, feature, self.radius, self.K, channels_first=False)
        return group_mlp(group, **_mlp_plan(self.local_feature_fused, "LocalFeatue.local_feature_fused"))


def fuse(model, refused=None):
    """Swap a loaded network's blocks for the fused ones, in place: every child of class name
    `GCN` with conv1, conv2, conv3 and k, every `PPF` with k, radius and local_feature_fused,
    every `LocalFeatue` with radius, K and local_feature_fused.  The new blocks hold the SAME
    submodules, so parameters are shared, not copied.  A block whose norm layers track running
    statistics, or whose structure is not conv -> norm -> activation, is left in place; its
    name and the reason are appended to `refused` (a list) when one is given.  Returns
    (GCN, PPF, LocalFeatue) blocks swapped; a second call finds nothing and returns zeros."""
    kinds = ((("GCN", ("conv1", "conv2", "conv3", "k")), GCN),
             (("PPF", ("k", "radius", "local_feature_fused")), PPF),
             (("LocalFeatue", ("radius", "K", "local_feature_fused")), LocalFeature))
    return _front.swap_children(model, kinds, refused=refused, skip=(GCN, PPF, LocalFeature))
