"""NgeNet's unary family and its forward, end to end on libpcr: rows times an
``nn.Linear`` weight, the InstanceNorm over the whole stacked cloud, the residual
add and the LeakyReLU as ONE call, the operand row ``[x0[gather[i]] | x1[i]]``
gathered and concatenated inside the kernel.

Mirror of pcr_unary_forward (contract in include/pcr_api.h, f64 restatement with
the derived bounds in tests/unary_ref.py):

* ``unary_forward`` -- ``UnaryBlock.forward`` (c2p-net/ngenet/models/KPConv/blocks.py:160-174),
  and with ``gather`` / ``x1`` the decoder's ``NearestUpsampleBlock`` ->
  ``torch.cat([up, skip])`` -> ``UnaryBlock`` (NgeNet.py:185-212) without the
  up-sampled rows or the concatenated operand;
* ``norm_act``      -- ``BatchNormBlock`` (+ LeakyReLU, + residual) on an existing
  tensor, e.g. the KPConv output (blocks.py:135-157);
* ``Unary`` / ``NearestUpsample`` / ``Simple`` / ``ResnetBottleneck`` -- the blocks
  with the reference's attribute names and state-dict keys; ``fuse(model)`` swaps
  a loaded network's blocks in place, parameters shared;
* ``forward(model, inputs)`` -- ``NgeNet.forward`` (NgeNet.py:132-221) on the
  model's own submodules, the overlap scores through
  ``attention.overlap_scores`` and every decoder triple as one call.

The norm takes its statistics over the whole cloud in train and eval mode alike
(``InstanceNorm1d``, no affine, no running statistics), so nothing is folded.

f32, CUDA tensors only (no CPU path), forward only: an input or parameter that
requires grad under grad mode raises.  Two calls return the same bytes.
"""
from __future__ import annotations

import ctypes

import torch

from . import _front, _lib, attention

__all__ = ["unary_forward", "norm_act", "Unary", "NearestUpsample", "Simple", "ResnetBottleneck", "fuse", "forward",
           "MAX_ROWS", "MAX_IN", "MAX_OUT"]

MAX_ROWS = 1 << 22   # pcr_api.h
MAX_IN = 2048        # c0 + c1
MAX_OUT = 1024       # cout
_STAGES = ("y", "stats")


def _rows(t, name, dev=None):
    """A (rows, c) f32 CUDA tensor with unit stride along c, on its own storage where it has one."""
    return _front.tensor(t, name, "(rows, channels)", 2, dev, "f32", _front.rows)


def _call(x0, weight, gather, x1, bias, norm, eps, slope, act, residual, want, who):
    _front.forward_only(who, x0, weight, x1, bias, residual)
    x0 = _rows(x0, "x0")
    dev = x0.device
    m0, c0 = x0.shape
    if c0 < 1:
        raise ValueError("x0 has no channels")
    if gather is not None:
        if not isinstance(gather, torch.Tensor) or gather.dtype.is_floating_point or gather.dtype == torch.bool \
                or gather.dim() != 1:
            raise ValueError("gather must be a 1-d integer tensor")
        if gather.device != dev:
            raise ValueError("all inputs must live on one device")
        if m0 < 1:
            raise ValueError("x0 has no rows to gather from")
        n = gather.shape[0]
        g = gather.to(torch.int32).contiguous()
    else:
        n, g = m0, None
    c1 = 0
    if x1 is not None:
        x1 = _rows(x1, "x1", dev)
        if x1.shape[0] != n:
            raise ValueError(f"x1 has {x1.shape[0]} rows, the operand {n}")
        c1 = x1.shape[1]
        if c1 == 0:
            x1 = None
    cin = c0 + c1
    if cin > MAX_IN:
        raise ValueError(f"c0 + c1 = {cin} above {MAX_IN}")
    if weight is not None:
        w = _rows(weight, "weight", dev).contiguous()
        if w.shape[1] != cin:
            raise ValueError(f"weight {tuple(w.shape)} must be (cout, c0 + c1 = {cin})")
        cout = w.shape[0]
    else:
        w, cout = None, cin
    if not 1 <= cout <= MAX_OUT:
        raise ValueError(f"cout={cout} outside 1..{MAX_OUT}")
    if n > MAX_ROWS:
        raise ValueError(f"n={n} above {MAX_ROWS}")
    norm, act = bool(norm), bool(act)
    if norm and bias is not None:
        raise ValueError("bias together with norm: the norm removes it")
    if norm and n == 1:
        raise ValueError("n=1: the norm needs at least two rows (as torch's InstanceNorm1d)")
    eps, slope = float(eps), float(slope)
    if not eps >= 0:
        raise ValueError(f"eps={eps} must be >= 0")
    if not abs(slope) <= 1:
        raise ValueError(f"slope={slope} outside -1..1")
    if bias is not None:
        bias = _front.param(bias, "bias", (cout,), dev)
    if residual is not None:
        residual = _rows(residual, "residual", dev).contiguous()
        if tuple(residual.shape) != (n, cout):
            raise ValueError(f"residual {tuple(residual.shape)} must be ({n}, {cout})")
    want = _front.wanted(want, _STAGES)
    if "stats" in want and not norm:
        raise ValueError("want: stats without norm")
    out = torch.empty((n, cout), dtype=torch.float32, device=dev)
    outs = {}
    if "y" in want:
        outs["y"] = torch.empty((n, cout), dtype=torch.float32, device=dev)
    if "stats" in want:
        outs["stats"] = torch.empty((cout, 2), dtype=torch.float64, device=dev)
    if n:
        lib = _lib.load()
        a = _lib.UnaryArgs()
        a.n, a.m0, a.c0, a.c1, a.cout = n, m0, c0, c1, cout
        a.x0, a.ld0 = x0.data_ptr(), x0.stride(0)
        a.g0 = g.data_ptr() if g is not None else None
        if x1 is not None:
            a.x1, a.ld1 = x1.data_ptr(), x1.stride(0)
        a.w = w.data_ptr() if w is not None else None
        a.bias = bias.data_ptr() if bias is not None else None
        a.norm, a.eps, a.act, a.slope = int(norm), eps, int(act), slope
        a.res = residual.data_ptr() if residual is not None else None
        a.out = out.data_ptr()
        a.y = outs["y"].data_ptr() if "y" in outs else None
        a.stats = outs["stats"].data_ptr() if "stats" in outs else None
        with torch.cuda.device(dev):
            ws = _front.scratch(lib.pcr_unary_scratch_bytes(n, cout), dev)
            _lib.call("pcr_unary_forward", ctypes.byref(a), _lib.ptr(ws), _lib.stream_handle(dev))
    if want:
        return (out,) + tuple(outs[k] for k in want)
    return out


def unary_forward(x0, weight, *, gather=None, x1=None, bias=None, norm=True, eps=1e-5, slope=0.1, act=True,
                  residual=None, want=()):
    """``act(norm([x0[gather] | x1] @ weight.T) + residual)`` as one fused call.

    x0 ``(m0, c0)``; gather ``(n,)`` integers or None (then row i reads
    ``x0[i]``), an index outside ``[0, m0)`` reading a row of zeros; x1
    ``(n, c1)`` or None; weight ``(cout, c0 + c1)`` (``nn.Linear``'s); bias
    ``(cout,)`` only with ``norm=False``; norm: InstanceNorm over the n rows
    (biased variance, no affine); act: LeakyReLU(slope), applied last; residual
    ``(n, cout)`` added before it.  ``c0 + c1 <= 2048``, ``cout <= 1024``.
    Returns ``(n, cout)``.  want: names among "y" ``(n, cout)`` (the product
    before the norm) and "stats" ``(cout, 2)`` f64 (mean, var), appended."""
    if weight is None:
        raise ValueError("unary_forward needs a weight: norm_act is the call without one")
    return _call(x0, weight, gather, x1, bias, norm, eps, slope, act, residual, want, "ngenet.unary_forward")


def norm_act(x, *, gather=None, x1=None, bias=None, norm=True, eps=1e-5, slope=0.1, act=True, residual=None,
             want=()):
    """``act(norm(x) + residual)`` on an existing ``(n, c)`` tensor -- BatchNormBlock
    and the LeakyReLU behind a KPConv -- with unary_forward's other arguments."""
    return _call(x, None, gather, x1, bias, norm, eps, slope, act, residual, want, "ngenet.norm_act")


# ---- the blocks' structure ---------------------------------------------------------------

def _norm_plan(bn, who):
    """(norm, eps, bias) of a BatchNormBlock-shaped module (use_bn, and batch_norm or bias)."""
    if not hasattr(bn, "use_bn"):
        raise ValueError(f"{who}: expected a BatchNormBlock (use_bn)")
    if bn.use_bn:
        inorm = getattr(bn, "batch_norm", None)
        if not isinstance(inorm, torch.nn.InstanceNorm1d):
            raise ValueError(f"{who}: the norm is a {type(inorm).__name__}, not an InstanceNorm1d")
        if inorm.affine or inorm.track_running_stats:
            raise ValueError(f"{who}: an affine InstanceNorm1d, or one with running statistics, is not built")
        return True, float(inorm.eps), None
    return False, 0.0, bn.bias


def _unary_shaped(mod):
    mlp = getattr(mod, "mlp", None)
    return isinstance(mlp, torch.nn.Linear) and mlp.bias is None and hasattr(getattr(mod, "bn", None), "use_bn") \
        and hasattr(mod, "relu")


def _slope(mod):
    lr = getattr(mod, "leaky_relu", None)
    return float(lr.negative_slope) if isinstance(lr, torch.nn.LeakyReLU) else 0.1


def _run_unary(block, x0, gather=None, x1=None, residual=None, act=None, slope=None):
    """A UnaryBlock-shaped module (the reference's or Unary) as one call, on its own parameters."""
    norm, eps, bias = _norm_plan(block.bn, type(block).__name__ + ".bn")
    return unary_forward(x0, block.mlp.weight, gather=gather, x1=x1, bias=bias, norm=norm, eps=eps,
                         slope=_slope(block) if slope is None else slope, act=bool(block.relu) if act is None else act,
                         residual=residual)


def _run_norm(bn, x, slope, who):
    norm, eps, bias = _norm_plan(bn, who)
    return norm_act(x, bias=bias, norm=norm, eps=eps, slope=slope, act=True)


class BatchNorm(torch.nn.Module):
    """BatchNormBlock (blocks.py:135-157): ``batch_norm`` (InstanceNorm1d) or ``bias``."""

    def __init__(self, in_dim, use_bn, bn_momentum):
        super().__init__()
        self.use_bn = use_bn
        if use_bn:
            self.batch_norm = torch.nn.InstanceNorm1d(in_dim, momentum=bn_momentum)
        else:
            self.bias = torch.nn.Parameter(torch.zeros(in_dim, dtype=torch.float32), requires_grad=True)

    def forward(self, features):
        norm, eps, bias = _norm_plan(self, "BatchNorm")
        return norm_act(features, bias=bias, norm=norm, eps=eps, act=False)


class Unary(torch.nn.Module):
    """UnaryBlock (blocks.py:160-174) on unary_forward, with its attribute names and state-dict
    keys (``mlp.weight``, and ``bn.bias`` when ``use_bn=False``).  `like` (fuse()): an existing
    block whose ``mlp`` and ``bn`` are shared."""

    def __init__(self, in_dim=None, out_dim=None, use_bn=True, bn_momentum=0.1, relu=True, like=None):
        super().__init__()
        if like is not None:
            if not _unary_shaped(like):
                raise ValueError("Unary: `like` is no UnaryBlock (mlp: Linear without bias, bn, relu)")
            _norm_plan(like.bn, "UnaryBlock.bn")
            self.relu, self.mlp, self.bn = like.relu, like.mlp, like.bn
            if self.relu:
                self.leaky_relu = like.leaky_relu
            return
        self.relu = relu
        self.mlp = torch.nn.Linear(in_dim, out_dim, bias=False)
        self.bn = BatchNorm(out_dim, use_bn, bn_momentum)
        if self.relu:
            self.leaky_relu = torch.nn.LeakyReLU(0.1)

    def forward(self, features, batch=None, *, gather=None, x1=None, residual=None):
        return _run_unary(self, features, gather=gather, x1=x1, residual=residual)


class NearestUpsample(torch.nn.Module):
    """NearestUpsampleBlock (blocks.py:191-199); inside forward() the rows are not materialised."""

    def __init__(self, layer_ind):
        super().__init__()
        self.layer_ind = layer_ind

    def forward(self, feats, batch):
        return feats[batch["upsamples"][self.layer_ind][:, 0].long()]


def _conv_inputs(block, batch):
    s_pts = batch["points"][block.layer_ind]
    if "strided" in block.block_name:
        return batch["points"][block.layer_ind + 1], s_pts, batch["pools"][block.layer_ind]
    return s_pts, s_pts, batch["neighbors"][block.layer_ind]


class Simple(torch.nn.Module):
    """SimpleBlock (blocks.py:202-233) around `like`'s own ``KPConv`` (fused or not) and ``bn``:
    the norm and the LeakyReLU behind the convolution are one norm_act."""

    def __init__(self, like):
        super().__init__()
        _norm_plan(like.bn, "SimpleBlock.bn")
        for name in ("block_name", "layer_ind", "in_dim", "out_dim", "radius"):
            setattr(self, name, getattr(like, name, None))
        self.KPConv, self.bn, self.leaky_relu = like.KPConv, like.bn, like.leaky_relu

    def forward(self, s_feats, batch):
        q_pts, s_pts, neigh_inds = _conv_inputs(self, batch)
        q_feats = self.KPConv(q_pts, s_pts, s_feats, neigh_inds)
        return _run_norm(self.bn, q_feats, _slope(self), "Simple.bn")


class ResnetBottleneck(torch.nn.Module):
    """ResnetBottleneckBlock (blocks.py:236-290) around `like`'s own children: ``unary1``, ``unary2``
    and ``unary_shortcut`` run through unary_forward, the norm and LeakyReLU behind ``KPConv`` are one
    norm_act, and the residual add with the last LeakyReLU rides in ``unary2``'s call."""

    def __init__(self, like):
        super().__init__()
        _norm_plan(like.bn, "ResnetBottleneckBlock.bn")
        for name in ("unary1", "unary2", "unary_shortcut"):
            child = getattr(like, name)
            if not isinstance(child, torch.nn.Identity):
                if not _unary_shaped(child):
                    raise ValueError(f"ResnetBottleneckBlock.{name} is no UnaryBlock")
                _norm_plan(child.bn, f"ResnetBottleneckBlock.{name}.bn")
        if isinstance(like.unary2, torch.nn.Identity):
            raise ValueError("ResnetBottleneckBlock.unary2 is an Identity")
        for name in ("block_name", "layer_ind", "in_dim", "out_dim", "radius"):
            setattr(self, name, getattr(like, name, None))
        self.unary1, self.KPConv, self.bn, self.unary2 = like.unary1, like.KPConv, like.bn, like.unary2
        self.max_pool, self.unary_shortcut, self.leaky_relu = like.max_pool, like.unary_shortcut, like.leaky_relu

    def forward(self, s_feats, batch):
        q_pts, s_pts, neigh_inds = _conv_inputs(self, batch)
        s_feats_d = s_feats if isinstance(self.unary1, torch.nn.Identity) else _run_unary(self.unary1, s_feats)
        q_feats = self.KPConv(q_pts, s_pts, s_feats_d, neigh_inds)
        q_feats = _run_norm(self.bn, q_feats, _slope(self), "ResnetBottleneck.bn")
        shortcut = self.max_pool(s_feats, batch) if "strided" in self.block_name else s_feats
        if not isinstance(self.unary_shortcut, torch.nn.Identity):
            shortcut = _run_unary(self.unary_shortcut, shortcut)
        return _run_unary(self.unary2, q_feats, residual=shortcut, act=True, slope=_slope(self))


def fuse(model, refused=None):
    """Swap a loaded network's blocks for the fused ones, in place: every child of class name
    `UnaryBlock` with mlp (a Linear without bias), bn and relu, every `NearestUpsampleBlock` with
    layer_ind, every `SimpleBlock` with KPConv, bn, leaky_relu, block_name and layer_ind, every
    `ResnetBottleneckBlock` with those and unary1, unary2, unary_shortcut and max_pool.  The new
    blocks hold the SAME submodules, so parameters are shared, not copied; a block's KPConv and
    max_pool stay what they are, so kpconv.fuse may run before or after.  A block whose norm is
    not a plain InstanceNorm1d is left in place; its name and the reason are appended to `refused`
    (a list) when one is given.  Returns (UnaryBlock, NearestUpsampleBlock, SimpleBlock,
    ResnetBottleneckBlock) blocks swapped; a second call finds nothing and returns zeros."""
    conv = ("KPConv", "bn", "leaky_relu", "block_name", "layer_ind")
    kinds = ((("UnaryBlock", ("mlp", "bn", "relu")), lambda m: Unary(like=m)),
             (("NearestUpsampleBlock", ("layer_ind",)), lambda m: NearestUpsample(m.layer_ind)),
             (("SimpleBlock", conv), Simple),
             (("ResnetBottleneckBlock", conv + ("unary1", "unary2", "unary_shortcut", "max_pool")), ResnetBottleneck))
    # the leaves first: a swapped block then holds its swapped unaries
    return _front.swap_children(model, kinds, refused=refused, waves=((0, 1), (2, 3)))


# ---- the network's forward ---------------------------------------------------------------

class _Up:
    """A nearest up-sampling that has not been materialised: rows `feats[idx]`."""

    def __init__(self, feats, idx):
        self.feats, self.idx = feats, idx


def _decoder_step(block, state, skip, inputs):
    """One decoder block on `state` (a tensor, or an _Up) with `skip` to concatenate (or None)."""
    kind = type(block).__name__
    if kind in ("NearestUpsampleBlock", "NearestUpsample") and hasattr(block, "layer_ind"):
        if isinstance(state, _Up) or skip is not None:
            raise ValueError("ngenet.forward: an up-sampling directly behind another, or behind a skip")
        return _Up(state, inputs["upsamples"][block.layer_ind][:, 0])
    if not _unary_shaped(block):
        raise ValueError(f"ngenet.forward: decoder block {kind} is neither an up-sampling nor a unary block")
    if isinstance(state, _Up):
        return _run_unary(block, state.feats, gather=state.idx, x1=skip)
    return _run_unary(block, state, x1=skip)


def forward(model, inputs):
    """NgeNet.forward (NgeNet.py:132-221) on `model`'s own submodules (fused or not): the same three
    outputs ``(feats_h | overlap | saliency (n, C + 2), feats_m (n, C), feats_l (n, C))``.  The overlap
    scores go through attention.overlap_scores (no (n1, n2) matrix), and every ``nearest_upsample ->
    cat(skip) -> unary`` triple of the three decoder branches is one unary_forward (no up-sampled rows,
    no concatenated operand).  The bottleneck, pro_gnn and attn_score Conv1ds, the sigmoids and the L2
    normalisation stay torch's.  Call it under torch.no_grad()."""
    stack_points, stacked_normals, stack_lengths = inputs["points"], inputs["normals"], inputs["stacked_lengths"]

    # 1. encoder
    feats = inputs["feats"]
    block_i, skip_feats = 0, []
    for block in model.encoder_blocks:
        if block_i in model.encoder_skips:
            skip_feats.append(feats)
        feats = block(feats, inputs)
        block_i += 1

    # 2.1, 2.2 bottleneck and information interaction
    feats = model.bottleneck(feats.transpose(0, 1).unsqueeze(0))  # (1, C, n)
    len_src = int(stack_lengths[-1][0])
    coords, normals = stack_points[-1], stacked_normals[-1]
    cf = lambda t: t.transpose(0, 1).unsqueeze(0)  # noqa: E731
    feats_src, feats_tgt = model.info_interative(cf(coords[:len_src]), feats[:, :, :len_src], cf(coords[len_src:]),
                                                 feats[:, :, len_src:], cf(normals[:len_src]), cf(normals[len_src:]))
    feats = model.pro_gnn(torch.cat([feats_src, feats_tgt], dim=-1))

    # 2.3 overlap scores, 2.4 feats
    attn_scores = model.attn_score(feats).squeeze(0).transpose(0, 1)  # (n, 1)
    temperature = torch.exp(model.epsilon) + 0.03
    feats_norm = (feats / (torch.norm(feats, dim=1, keepdim=True) + 1e-8)).squeeze(0).transpose(0, 1)  # (n, C)
    ol_scores = attention.overlap_scores(feats_norm.detach(), attn_scores.detach(), len_src, temperature.detach())
    state_h = torch.cat([feats.squeeze(0).transpose(0, 1), attn_scores, ol_scores], dim=1)

    # 3. decoder: three branches; the skip is concatenated inside the unary's call
    state_m = state_l = None
    cnt = 0
    off_l = model.decoder_skips[1] - model.decoder_skips[0] + 1 if len(model.decoder_skips) > 1 else 0
    for ind, block in enumerate(model.decoder_blocks):
        skip = None
        first_m = first_l = False
        if block_i in model.decoder_skips:
            cnt += 1
            skip = skip_feats.pop()
            first_m, first_l = cnt == 1, cnt == 2
        if cnt >= 1:
            block_m = model.decoder_blocks_m[ind - 1]
            state_m = _decoder_step(block_m, skip, None, inputs) if first_m else \
                _decoder_step(block_m, state_m, skip, inputs)
        if cnt >= 2:
            block_l = model.decoder_blocks_l[ind - off_l]
            state_l = _decoder_step(block_l, skip, None, inputs) if first_l else \
                _decoder_step(block_l, state_l, skip, inputs)
        state_h = _decoder_step(block, state_h, skip, inputs)
        block_i += 1
    for s in (state_h, state_m, state_l):
        if not isinstance(s, torch.Tensor):
            raise ValueError("ngenet.forward: a decoder branch is missing or ends in an up-sampling")

    overlap = torch.sigmoid(state_h[:, -2:-1])
    saliency = torch.sigmoid(state_h[:, -1:])
    feats_h = state_h[:, :-2] / torch.norm(state_h[:, :-2], dim=1, keepdim=True)
    feats_m = state_m / torch.norm(state_m, dim=1, keepdim=True)
    feats_l = state_l / torch.norm(state_l, dim=1, keepdim=True)
    return torch.cat([feats_h, overlap, saliency], dim=-1), feats_m, feats_l
