"""ROPNet's dense part and its forward, end to end on libpcr: a ``Conv1d(k=1)``
weight times channel-major clouds ``(B, C, N)``, the GroupNorm over (cloud,
channel group, all points), the biases, the (Leaky)ReLU, the residual add and
the max over points as ONE call, whose operand is up to five tensors side by
side, each optionally minus another -- no ``torch.cat``, no ``x - x_r``, no
``(B, 6144, N)`` ensemble.

Mirror of pcr_pointwise_forward (contract in include/pcr_api.h, f64 restatement
with the derived bounds in tests/pointwise_ref.py):

* ``pointwise_forward`` -- the checked front end;
* ``PointNet``          -- ``CG.py:15-43``, one call per layer, the max in the last;
* ``CG``                -- ``CGModule.forward`` (``CG.py:63-106``); the overlap
  decoder's first layer is split into a per-cloud bias (``n = 1`` call over the
  weight's columns 1536..) and the product over ``f`` with the first 1536;
* ``OverlapAttention``  -- ``TFMR.py:109-130``: per block one product for q and
  k, one for v, ``attention.offset_attention``, then one call for
  ``x + relu(gn(trans_conv(x - x_r)))``; ``conv_fuse`` one call over five sources;
* ``fuse(model)``       -- swaps a loaded network's ``CGModule`` and
  ``OverlapAttention`` in place, parameters shared;
* ``forward(model, src, tgt, num_iter)`` -- ``ROPNet.forward`` with
  ``train=False`` on the model's own submodules.

f32, CUDA tensors only (no CPU path), forward only, eval mode only: an input or
parameter that requires grad under grad mode raises, a module in training mode
is refused.  Two calls return the same bytes.
"""
from __future__ import annotations

import ctypes

import torch

from . import _front, _lib, attention, grouping, groupmlp, matching, procrustes

__all__ = ["pointwise_forward", "PointNet", "MLPs", "CG", "OverlapAttention", "fuse", "forward", "MAX_POINTS",
           "MAX_IN", "MAX_OUT", "MAX_SOURCES"]

MAX_POINTS = 1 << 22   # pcr_api.h
MAX_IN = 8192          # cin, the sources' channels together
MAX_OUT = 2048         # cout
MAX_SOURCES = 5
MAX_CLOUDS = 65535
_STAGES = ("out", "max", "y", "stats")


def _cloud(t, name, dev=None, b=None, n=None):
    """A (B, C, N) f32 CUDA tensor with unit stride over points (anything else is copied once)."""
    if b is None:
        return _front.tensor(t, name, "(B, C, N)", 3, dev, "f32", _front.unit_last)
    return _front.tensor(t, name, "(B={0}, C, N={2})", (b, None, n), dev, "f32", _front.unit_last)


def pointwise_forward(sources, weight, *, sub=None, bias=None, cloud_bias=None, groups=0, gamma=None, beta=None,
                      eps=1e-5, act=False, slope=0.0, residual=None, want=("out",)):
    """``act(norm_or_bias(weight @ [s_0 - sub_0 | s_1 - sub_1 | ...])) + residual`` as one fused call.

    sources: a ``(B, C, N)`` tensor or up to five of them (channel slices and batch-strided views are
    read where they lie; a stride over points other than 1 is copied).  weight ``(cout, cin)`` or a
    Conv1d's ``(cout, cin, 1)``; a column slice of a wider weight is read where it lies.  sub: None, or
    one entry (a tensor of its source's shape, or None) per source.  bias ``(cout,)``, cloud_bias
    ``(B, cout)``.  groups: GroupNorm's ``num_groups`` over ``cout`` (0: no norm), with gamma / beta
    ``(cout,)`` or None; its statistics are those of the product with its biases.  act:
    ``z > 0 ? z : slope z``.  residual ``(B, cout, N)`` is added AFTER the activation.  want: names
    among "out" ``(B, cout, N)``, "max" ``(B, cout)`` (max over points of out, from -inf), "y" (the
    product before norm and bias) and "stats" ``(B, groups, 2)`` f64 (mean, var).  Returns the one
    tensor asked for, or a tuple in want's order.  ``cin <= 8192``, ``cout <= 2048``."""
    if isinstance(sources, torch.Tensor):
        sources = (sources,)
    sources = tuple(sources)
    if not 1 <= len(sources) <= MAX_SOURCES:
        raise ValueError(f"{len(sources)} sources: 1..{MAX_SOURCES}")
    subs = (None,) * len(sources) if sub is None else ((sub,) if isinstance(sub, torch.Tensor) else tuple(sub))
    if len(subs) != len(sources):
        raise ValueError(f"sub has {len(subs)} entries for {len(sources)} sources")
    _front.forward_only("ropnet.pointwise_forward", *sources, *subs, weight, bias, cloud_bias, gamma, beta, residual)
    srcs = [_cloud(sources[0], "sources[0]")]
    dev = srcs[0].device
    b, _, n = srcs[0].shape
    for i, t in enumerate(sources[1:], 1):
        srcs.append(_cloud(t, f"sources[{i}]", dev, b, n))
    for i, t in enumerate(srcs):
        if t.shape[1] < 1:
            raise ValueError(f"sources[{i}] has no channels")
    subs = [None if u is None else _cloud(u, f"sub[{i}]", dev, b, n) for i, u in enumerate(subs)]
    for i, u in enumerate(subs):
        if u is not None and u.shape[1] != srcs[i].shape[1]:
            raise ValueError(f"sub[{i}] {tuple(u.shape)} must match sources[{i}] {tuple(srcs[i].shape)}")
    cin = sum(t.shape[1] for t in srcs)
    if cin > MAX_IN:
        raise ValueError(f"cin = {cin} above {MAX_IN}")
    if not isinstance(weight, torch.Tensor):
        raise TypeError("weight must be a torch.Tensor")
    w = weight.detach()
    if w.dim() == 3:
        if w.shape[2] != 1:
            raise ValueError(f"weight {tuple(w.shape)}: a kernel size other than 1")
        w = w[:, :, 0]
    if not w.is_cuda or w.dtype != torch.float32 or w.device != dev or w.dim() != 2 or w.shape[1] != cin:
        raise ValueError(f"weight {tuple(weight.shape)} must be (cout, cin = {cin}) torch.float32 on {dev}")
    if w.stride(1) != 1 or not cin <= w.stride(0) <= MAX_IN:   # a column slice of a wider weight goes in by stride
        w = w.contiguous()
    cout = w.shape[0]
    if not 1 <= cout <= MAX_OUT:
        raise ValueError(f"cout={cout} outside 1..{MAX_OUT}")
    if n > MAX_POINTS:
        raise ValueError(f"N={n} above {MAX_POINTS}")
    if b > MAX_CLOUDS:
        raise ValueError(f"B={b} above {MAX_CLOUDS}")
    groups = int(groups)
    if groups < 0 or (groups and cout % groups):
        raise ValueError(f"groups={groups} must divide cout={cout}")
    if not groups and (gamma is not None or beta is not None):
        raise ValueError("gamma / beta without a norm")
    eps, slope, act = float(eps), float(slope), bool(act)
    if not eps >= 0:
        raise ValueError(f"eps={eps} must be >= 0")
    if not abs(slope) <= 1:
        raise ValueError(f"slope={slope} outside -1..1")
    bias = None if bias is None else _front.param(bias, "bias", (cout,), dev)
    cloud_bias = None if cloud_bias is None else _front.param(cloud_bias, "cloud_bias", (b, cout), dev)
    gamma = None if gamma is None else _front.param(gamma, "gamma", (cout,), dev)
    beta = None if beta is None else _front.param(beta, "beta", (cout,), dev)
    if residual is not None:
        residual = _cloud(residual, "residual", dev, b, n)
        if residual.shape[1] != cout:
            raise ValueError(f"residual {tuple(residual.shape)} must be ({b}, {cout}, {n})")
    want, single = _front.wanted(want, _STAGES, single=True)
    if not want:
        raise ValueError("want: nothing asked for")
    if "stats" in want and not groups:
        raise ValueError("want: stats without norm")
    if "max" in want and n == 0:
        raise ValueError("want: max over no points")
    outs = {}
    if "out" in want or groups:
        outs["out"] = torch.empty((b, cout, n), dtype=torch.float32, device=dev)
    if "max" in want:
        outs["max"] = torch.empty((b, cout), dtype=torch.float32, device=dev)
    if "y" in want:
        outs["y"] = torch.empty((b, cout, n), dtype=torch.float32, device=dev)
    if "stats" in want:
        outs["stats"] = torch.empty((b, groups, 2), dtype=torch.float64, device=dev)
    if b and n:
        lib = _lib.load()
        a = _lib.PointwiseArgs()
        a.b, a.n, a.nsrc, a.cout = b, n, len(srcs), cout
        for i, (t, u) in enumerate(zip(srcs, subs)):
            a.c[i], a.src[i], a.src_bs[i], a.src_cs[i] = t.shape[1], t.data_ptr(), t.stride(0), t.stride(1)
            if u is not None:
                a.sub[i], a.sub_bs[i], a.sub_cs[i] = u.data_ptr(), u.stride(0), u.stride(1)
        a.w, a.w_ld = w.data_ptr(), w.stride(0)
        a.bias = bias.data_ptr() if bias is not None else None
        a.cbias = cloud_bias.data_ptr() if cloud_bias is not None else None
        a.gw, a.eps = (cout // groups if groups else 0), eps
        a.gamma = gamma.data_ptr() if gamma is not None else None
        a.beta = beta.data_ptr() if beta is not None else None
        a.act, a.slope = int(act), slope
        if residual is not None:
            a.res, a.res_bs, a.res_cs = residual.data_ptr(), residual.stride(0), residual.stride(1)
        if "out" in outs:
            o = outs["out"]
            a.out, a.out_bs, a.out_cs = o.data_ptr(), o.stride(0), o.stride(1)
        a.cmax = outs["max"].data_ptr() if "max" in outs else None
        a.y = outs["y"].data_ptr() if "y" in outs else None
        a.stats = outs["stats"].data_ptr() if "stats" in outs else None
        with torch.cuda.device(dev):
            ws = _front.scratch(lib.pcr_pointwise_scratch_bytes(b, n, cout), dev)
            _lib.call("pcr_pointwise_forward", ctypes.byref(a), _lib.ptr(ws), _lib.stream_handle(dev))
    got = tuple(outs[k] for k in want)
    return got[0] if single or len(got) == 1 else got


# ---- structure of the reference's modules ------------------------------------------------

def _eval_only(mod, who):
    if mod.training:
        raise RuntimeError(f"{who}: the module is in training mode; this module is forward-only, call .eval()")


def _conv1(conv, who):
    nn = torch.nn
    if not isinstance(conv, nn.Conv1d):
        raise ValueError(f"{who}: a {type(conv).__name__}, not a Conv1d")
    if conv.kernel_size != (1,) or conv.stride != (1,) or conv.padding not in ((0,), "valid") \
            or conv.dilation != (1,) or conv.groups != 1:
        raise ValueError(f"{who}: a kernel size other than 1 (or a stride, padding, dilation or groups)")
    return conv


def _group_norm(norm, cout, who):
    if not isinstance(norm, torch.nn.GroupNorm):
        raise ValueError(f"{who}: an unknown norm, a {type(norm).__name__}")
    if norm.num_channels != cout:
        raise ValueError(f"{who}: the norm has {norm.num_channels} channels, the layer {cout}")
    return norm


def _layers(backbone, who):
    """[(conv, norm or None, slope or None)] of a Sequential of Conv1d(k=1) [GroupNorm] [ReLU | LeakyReLU]."""
    nn = torch.nn
    if not isinstance(backbone, nn.Sequential):
        raise ValueError(f"{who}: expected a Sequential")
    plan = []
    for name, m in backbone.named_children():
        if isinstance(m, nn.Conv1d) or not plan:
            plan.append([_conv1(m, f"{who}.{name}"), None, None])
        elif isinstance(m, nn.LeakyReLU) and plan[-1][2] is None:
            plan[-1][2] = float(m.negative_slope)
        elif isinstance(m, nn.ReLU) and plan[-1][2] is None:
            plan[-1][2] = 0.0
        elif isinstance(m, nn.Dropout):
            pass
        elif plan[-1][1] is None and plan[-1][2] is None:
            plan[-1][1] = _group_norm(m, plan[-1][0].out_channels, f"{who}.{name}")
        else:
            raise ValueError(f"{who}.{name}: a {type(m).__name__} where conv, norm, activation is expected")
    if not plan:
        raise ValueError(f"{who}: no layers")
    return plan


def _run_layer(layer, sources, *, weight=None, sub=None, cloud_bias=None, residual=None, want="out"):
    """One (conv, norm, slope) layer as one call.  weight: used instead of the conv's own, whose bias is then
    left out (the caller has it inside cloud_bias)."""
    conv, norm, slope = layer
    kw = dict(sub=sub, bias=conv.bias if weight is None else None, cloud_bias=cloud_bias, act=slope is not None,
              slope=slope or 0.0, residual=residual, want=want)
    weight = conv.weight if weight is None else weight
    if norm is None:
        return pointwise_forward(sources, weight, **kw)
    return pointwise_forward(sources, weight, groups=norm.num_groups, gamma=norm.weight, beta=norm.bias, eps=norm.eps,
                             **kw)


class PointNet(torch.nn.Module):
    """``CG.py:15-43`` on pointwise_forward with the reference's ``backbone`` names and state-dict keys
    (``backbone.pointnet_conv_i``, ``backbone.pointnet_gn_i``).  One call per layer; the last layer of
    a pooling forward also returns the max over points.  `like` (fuse()): a module whose ``backbone``
    is shared."""

    def __init__(self, in_dim=None, gn=False, out_dims=(), cls=False, like=None):
        super().__init__()
        nn = torch.nn
        if like is not None:
            _layers(like.backbone, "PointNet.backbone")
            self.cls, self.backbone = bool(getattr(like, "cls", False)), like.backbone
            self.train(like.training)
            return
        self.cls = cls
        self.backbone = nn.Sequential()
        for i, out_dim in enumerate(out_dims):
            self.backbone.add_module(f"pointnet_conv_{i}", nn.Conv1d(in_dim, out_dim, 1, 1, 0))
            if gn:
                self.backbone.add_module(f"pointnet_gn_{i}", nn.GroupNorm(8, out_dim))
            if cls and i != len(out_dims) - 1:
                self.backbone.add_module(f"pointnet_relu_{i}", nn.ReLU(inplace=True))
            in_dim = out_dim

    def forward(self, x, pooling=True, *, first=None):
        """x (B, C, N) -> f (B, c_L, N), and with `pooling` also g (B, c_L), its max over points.
        first: (weight, cloud_bias) to run the first layer with instead of its own weight and with a
        per-cloud bias (CG's split decoder layer)."""
        _eval_only(self, "ropnet.PointNet")
        plan = _layers(self.backbone, "PointNet.backbone")
        for i, layer in enumerate(plan):
            last = i == len(plan) - 1
            want = ("out", "max") if last and pooling else "out"
            if i == 0 and first is not None:
                x = _run_layer(layer, x, weight=first[0], cloud_bias=first[1], want=want)
            else:
                x = _run_layer(layer, x, want=want)
        return x


class MLPs(torch.nn.Module):
    """``CG.py:46-60``: Linear layers with ReLU and (in eval, identity) Dropout between them, as
    ``n = 1`` calls.  Shares `like`'s ``mlps``."""

    def __init__(self, like):
        super().__init__()
        self._plan(like.mlps)
        self.mlps = like.mlps
        self.train(like.training)

    @staticmethod
    def _plan(mlps):
        nn = torch.nn
        plan = []
        for name, m in mlps.named_children():
            if isinstance(m, nn.Linear):
                plan.append([m, False])
            elif isinstance(m, nn.ReLU) and plan and not plan[-1][1]:
                plan[-1][1] = True
            elif not isinstance(m, nn.Dropout):
                raise ValueError(f"MLPs.mlps.{name}: a {type(m).__name__} where Linear, ReLU, Dropout is expected")
        if not plan:
            raise ValueError("MLPs.mlps: no layers")
        return plan

    def forward(self, x):
        """x (B, C) or a tuple of (B, c_s) pieces read side by side -> (B, c_L)."""
        _eval_only(self, "ropnet.MLPs")
        x = tuple(t.unsqueeze(-1) for t in (x if isinstance(x, (tuple, list)) else (x,)))
        for lin, relu in self._plan(self.mlps):
            x = pointwise_forward(x, lin.weight, bias=lin.bias, act=relu)
        return x.squeeze(-1)


def batch_quat2mat(q):
    """utils/process.py:122-142 restated: (B, 4) unit quaternions (w, x, y, z) -> (B, 3, 3)."""
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    rows = [1 - 2 * y * y - 2 * z * z, 2 * x * y - 2 * z * w, 2 * x * z + 2 * y * w,
            2 * x * y + 2 * z * w, 1 - 2 * x * x - 2 * z * z, 2 * y * z - 2 * x * w,
            2 * x * z - 2 * y * w, 2 * y * z + 2 * x * w, 1 - 2 * x * x - 2 * y * y]
    return torch.stack(rows, dim=1).reshape(-1, 3, 3)


def batch_transform(pc, R, t=None):
    """utils/process.py:90-101: (B, N, 3) points through R (B, 3, 3) and t (B, 3)."""
    out = torch.matmul(pc, R.permute(0, 2, 1).contiguous())
    return out if t is None else out + t.unsqueeze(1)


class CG(torch.nn.Module):
    """``CGModule`` (CG.py:63-106) around `like`'s own ``encoder``, ``decoder_ol`` and ``decoder_qt``
    (shared, same state-dict keys).  The (B, 6144, N) ensembles are never built: the first decoder
    layer's columns 1536.. times ``[g_x | g_y | g_x - g_y]`` plus its bias is a per-cloud bias (an
    ``n = 1`` call on sources g_x, g_y and g_x with sub g_y, the reference's three blocks kept), and the
    layer then runs over ``f`` with the first 1536 columns read by stride.  N != M is accepted (the
    reference's ``g_x_expand - g_y_expand`` needs N == M)."""

    def __init__(self, like):
        super().__init__()
        enc = _layers(like.encoder.backbone, "CGModule.encoder.backbone")
        dec = _layers(like.decoder_ol.backbone, "CGModule.decoder_ol.backbone")
        MLPs._plan(like.decoder_qt.mlps)
        width = enc[-1][0].out_channels
        if dec[0][0].in_channels != 4 * width:
            raise ValueError(f"CGModule.decoder_ol takes {dec[0][0].in_channels} channels, not 4 x {width}")
        self.encoder = like.encoder if isinstance(like.encoder, PointNet) else PointNet(like=like.encoder)
        self.decoder_ol = like.decoder_ol if isinstance(like.decoder_ol, PointNet) else PointNet(like=like.decoder_ol)
        self.decoder_qt = like.decoder_qt if isinstance(like.decoder_qt, MLPs) else MLPs(like.decoder_qt)
        self.train(like.training)

    def _overlap(self, f, g_own, g_other):
        conv, norm, _ = _layers(self.decoder_ol.backbone, "CG.decoder_ol.backbone")[0]
        c = f.shape[1]
        w = conv.weight.detach()[:, :, 0]
        gx, gy = g_own.unsqueeze(-1), g_other.unsqueeze(-1)
        # both halves of the weight are read where they lie; with a GroupNorm the statistics are those of the
        # full sum, as the per-cloud bias is added in front of them
        cloud_bias = pointwise_forward((gx, gy, gx), w[:, c:], sub=(None, None, gy), bias=conv.bias).squeeze(-1)
        return self.decoder_ol(f, pooling=False, first=(w[:, :c], cloud_bias))

    def forward(self, src, tgt):
        """src (B, N, 3), tgt (B, M, 3) -> T0 (B, 3, 4), x_ol (B, 2, N), y_ol (B, 2, M)."""
        _eval_only(self, "ropnet.CG")
        _front.forward_only("ropnet.CG", src, tgt, *self.parameters())
        f_x, g_x = self.encoder(src.permute(0, 2, 1).contiguous())
        f_y, g_y = self.encoder(tgt.permute(0, 2, 1).contiguous())
        out = self.decoder_qt((g_x, g_y))
        batch_t = out[:, :3]
        batch_quat = out[:, 3:] / (torch.norm(out[:, 3:], dim=1, keepdim=True) + 1e-8)
        batch_T = torch.cat([batch_quat2mat(batch_quat), batch_t[..., None]], dim=-1)
        return batch_T, self._overlap(f_x, g_x, g_y), self._overlap(f_y, g_y, g_x)


_BLOCKS = tuple(f"overlap_attention{i}" for i in range(1, 6))


def _block_plan(blk, who):
    for name in ("q_conv", "k_conv", "v_conv", "trans_conv"):
        _conv1(getattr(blk, name, None), f"{who}.{name}")
    if blk.q_conv.bias is not None or blk.k_conv.bias is not None:
        raise ValueError(f"{who}: q_conv or k_conv with a bias")
    _group_norm(blk.after_norm, blk.trans_conv.out_channels, f"{who}.after_norm")
    if blk.trans_conv.out_channels != blk.trans_conv.in_channels:
        raise ValueError(f"{who}: trans_conv changes the width, the residual add cannot follow")
    if not isinstance(blk.act, torch.nn.ReLU):
        raise ValueError(f"{who}: the activation is a {type(blk.act).__name__}")


class OverlapAttention(torch.nn.Module):
    """``OverlapAttention`` (TFMR.py:109-130) around `like`'s five blocks and ``conv_fuse`` (shared, same
    state-dict keys).  Per block: one product for q and k (two where the weights are not tied), one for
    v, ``attention.offset_attention``, and one call for ``x + relu(gn(trans_conv(x - x_r)))`` with
    ``sub = x_r`` and ``residual = x``.  ``conv_fuse`` reads the five block outputs as five sources."""

    def __init__(self, like):
        super().__init__()
        for name in _BLOCKS:
            _block_plan(getattr(like, name), f"OverlapAttention.{name}")
        fuse_plan = _layers(like.conv_fuse, "OverlapAttention.conv_fuse")
        if len(fuse_plan) != 1:
            raise ValueError("OverlapAttention.conv_fuse: expected one Conv1d, GroupNorm, activation")
        for name in _BLOCKS:
            setattr(self, name, getattr(like, name))
        self.conv_fuse = like.conv_fuse
        self.train(like.training)

    @staticmethod
    def _block(blk, x, ol):
        q = pointwise_forward(x, blk.q_conv.weight)
        k = q if blk.k_conv.weight is blk.q_conv.weight else pointwise_forward(x, blk.k_conv.weight)
        v = pointwise_forward(x, blk.v_conv.weight, bias=blk.v_conv.bias)
        x_r = attention.offset_attention(q, k, v, ol)
        return _run_layer((blk.trans_conv, blk.after_norm, 0.0), x, sub=x_r, residual=x)

    def forward(self, x, ol=None):
        """x (B, C, N), ol (B, N) or None -> (B, 5 C, N)."""
        _eval_only(self, "ropnet.OverlapAttention")
        _front.forward_only("ropnet.OverlapAttention", x, ol, *self.parameters())
        xs = []
        for name in _BLOCKS:
            x = self._block(getattr(self, name), x, ol)
            xs.append(x)
        return _run_layer(_layers(self.conv_fuse, "OverlapAttention.conv_fuse")[0], xs)


def fuse(model, refused=None):
    """Swap a loaded ROPNet's dense modules for the fused ones, in place: every child of class name
    `CGModule` with encoder, decoder_ol and decoder_qt becomes a CG, every `OverlapAttention` with
    overlap_attention1..5 and conv_fuse an OverlapAttention of this module.  The new modules hold the
    SAME submodules, so parameters are shared, not copied; it may run before or after groupmlp.fuse and
    attention.fuse (a swapped container runs its blocks' layers itself, whichever class they have).  A
    module with a kernel size other than 1, an unknown norm or another structure is left in place; its
    name and the reason are appended to `refused` (a list) when one is given.  Returns (CGModule,
    OverlapAttention) swapped; a second call finds nothing and returns zeros."""
    kinds = ((("CGModule", ("encoder", "decoder_ol", "decoder_qt")), CG),
             (("OverlapAttention", _BLOCKS + ("conv_fuse",)), OverlapAttention))
    return _front.swap_children(model, kinds, refused=refused, errors=(ValueError, AttributeError),
                                skip=(CG, OverlapAttention))


# ---- the network's forward ---------------------------------------------------------------

def _gather(points, inds):
    return points[torch.arange(points.shape[0], device=points.device).view(-1, 1), inds]


def _features(tfmr, xyz, normals, ol_score, keep):
    """TFMR.py:186-200 for one side: local features, overlap attention, L2 normalise, sort by overlap
    score, keep the first `keep` -> (features (B, keep, C), points (B, keep, 3), sorted scores, inds)."""
    lf = tfmr.local_features
    use_ppf = bool(tfmr.use_ppf) and normals is not None
    if isinstance(lf, groupmlp.LocalFeature):
        f_p = lf(feature=normals if use_ppf else None, xyz=xyz, use_ppf=use_ppf)
    else:   # the reference's LocalFeatue, unfused: its MLP through the library all the same
        group = grouping.local_ppf_features(xyz, normals if use_ppf else None, lf.radius, lf.K,
                                            channels_first=False)
        f_p = groupmlp.group_mlp(group, **groupmlp._mlp_plan(lf.local_feature_fused, "LocalFeatue"))
    oa = tfmr.overlap_attention
    f = (oa if isinstance(oa, OverlapAttention) else OverlapAttention(oa))(f_p, None).permute(0, 2, 1).contiguous()
    f = f / (torch.norm(f, dim=-1, keepdim=True) + 1e-8)
    score, inds = torch.sort(ol_score, dim=-1, descending=True)
    inds = inds[:, :keep]
    return _gather(f, inds), _gather(xyz, inds), score, inds


def forward(model, src, tgt, num_iter=1):
    """``ROPNet.forward`` (ROPNet.py:26-96) with ``train=False`` on `model`'s own submodules (fused or
    not): the same dict (pred_Ts, pred_src, x_ol, y_ol, src_ol1, src_ol2).  The CG and the overlap
    attention run on pointwise_forward, the local features on grouping / groupmlp, TFMR.py:226-257 on
    matching.tfmr_match, the fit on procrustes.weighted_icp; the two-class softmax, the L2 normalise,
    the sorts and the gathers stay torch's.  The target's features are computed once and kept in a
    local variable, not on the module.  Without normals the trailing ``batch_transform(normal_src, R)``
    is skipped (the reference raises there).  num_iter >= 1."""
    if model.training:
        raise RuntimeError("ropnet.forward: the model is in training mode; this module is forward-only, "
                           "call model.eval()")
    _front.forward_only("ropnet.forward", src, tgt, *model.parameters())
    if num_iter < 1:
        raise ValueError(f"num_iter={num_iter}: the reference's result needs at least one iteration")
    tfmr = model.tfmr
    normal_src = normal_tgt = None
    if model.use_ppf and src.shape[-1] == 6:
        normal_src, normal_tgt = src[..., 3:].contiguous(), tgt[..., 3:].contiguous()
    src, tgt = src[..., :3].contiguous(), tgt[..., :3].contiguous()
    src_raw = src
    N1, M1, top_prob, topk = tfmr.N1s[1], tfmr.M1s[1], tfmr.top_probs[1], tfmr.similarity_topks[1]

    cg = model.cg if isinstance(model.cg, CG) else CG(model.cg)
    T0, x_ol, y_ol = cg(src, tgt)
    R, t = T0[:, :3, :3], T0[:, :3, 3]
    src_t = batch_transform(src_raw, R, t)
    normal_src_t = batch_transform(normal_src, R) if normal_src is not None else None
    pred_Ts, pred_src = [T0], [src_t]
    x_ol_score = torch.softmax(x_ol, dim=1)[:, 1, :]
    y_ol_score = torch.softmax(y_ol, dim=1)[:, 1, :]

    f_y = tgt_kept = sel = None
    for it in range(num_iter):
        f_x, src_kept, x_sorted, _ = _features(tfmr, src_t, normal_src_t, x_ol_score, N1)
        if it == 0:
            f_y, tgt_kept, _, _ = _features(tfmr, tgt, normal_tgt, y_ol_score, M1)
        src_sel, tgt_corr, icp_w, sel = matching.tfmr_match(f_x, f_y, src_kept, tgt_kept, x_sorted, top_prob, topk)
        R_cur, t_cur, _ = procrustes.weighted_icp(src=src_sel, tgt=tgt_corr, weights=icp_w)
        R, t = R_cur @ R, R_cur @ t[:, :, None] + t_cur[:, :, None]
        pred_Ts.append(torch.cat([R, t], dim=-1))
        t = torch.squeeze(t, dim=-1)
        src_t = batch_transform(src_raw, R, t)
        pred_src.append(src_t)
        if normal_src is not None:
            normal_src_t = batch_transform(normal_src, R)

    x_ol_inds = torch.sort(x_ol_score, dim=-1, descending=True)[1][:, :model.N1]
    src_ol1 = _gather(src_raw, x_ol_inds)
    return {"pred_Ts": pred_Ts, "pred_src": pred_src, "x_ol": x_ol, "y_ol": y_ol, "src_ol1": src_ol1,
            "src_ol2": _gather(src_ol1, sel)}
