"""Fused softmax attention: no (N, M) tensor in global memory.

Mirrors of the reference's attention stages on libpcr
(pcr_attention_forward / pcr_offset_attention_forward; contract in
include/pcr_api.h, f64 restatement with the derived bound in
tests/attention_ref.py):

* ``multi_head_attention`` -- c2p-net/ngenet/models/information_interactive.py:165-177
* ``overlap_scores``       -- the inline lines c2p-net/ngenet/models/NgeNet.py:173-179
* ``offset_attention``     -- the bmm / softmax / column normalisation / bmm of
  ROPNet/src/models/TFMR.py:97-103
* ``CrossAttention`` / ``OverlapAttentionBlock`` -- the two modules with the
  reference's attribute names and state-dict keys; ``fuse(model)`` swaps a loaded
  network's blocks for them in place.

f32, CUDA tensors only (no CPU path), forward only: an input that requires grad
under grad mode raises.  Tensors are channel-major; a view whose token (last)
stride is 1 -- the (B, dim, nhead, N) reshape of a Conv1d output, a column
slice -- is passed by stride, anything else is copied once.

Two calls on the same inputs return the same bytes.  Batch caveat: where the
grid is small (B * nhead * ceil(N / 128) * ceil(dv / 64) <= 64 workgroups and
M > 224) ``multi_head_attention`` and ``overlap_scores`` split the keys into
runs whose number depends on that product, so a batch element's low bits may
differ between a call on it alone and one on the whole batch.  Without a split,
and always in ``offset_attention``, results do not depend on the batch.

The two modules keep the reference's constructor and forward line for line
apart from the attention itself, as kpconv.KPConv does: drop-in state dicts and
attribute names leave no other way to write them.  Nothing else here follows
the reference's text.
"""
from __future__ import annotations

import math

import torch

from . import _front, _lib

__all__ = ["multi_head_attention", "overlap_scores", "offset_attention", "CrossAttention",
           "OverlapAttentionBlock", "fuse", "MAX_CHANNELS"]

MAX_CHANNELS = 256   # d and dv (pcr_api.h)
MAX_TOKENS = 1 << 24


def _f32(t, name, phrase, ndim, dev=None):
    # unit token stride goes in by stride; anything else is copied once
    return _front.tensor(t, name, phrase, ndim, dev, "f32", _front.unit_last)


def _channels(name, c):
    if not 1 <= c <= MAX_CHANNELS:
        raise ValueError(f"{name}={c} channels outside 1..{MAX_CHANNELS}")


def _attention(q, k, v, out, b, h, n, m, d, dv, scale, strides):
    """One pcr_attention_forward; strides = (q, k, v, out) x (batch, head, channel)."""
    lib = _lib.load()
    dev = q.device
    with torch.cuda.device(dev):
        ws = _front.scratch(lib.pcr_attention_scratch_bytes(b, h, n, m, d, dv), dev)
        args = []
        for t, st in zip((q, k, v, out), strides):
            args += [_lib.ptr(t), *st]
        _lib.call("pcr_attention_forward", *args, b, h, n, m, d, dv, float(scale), _lib.ptr(ws),
                  _lib.stream_handle(dev))


def multi_head_attention(query, key, value):
    """information_interactive.py:165-177 as one fused call: query (B, dim, nhead, N),
    key (B, dim, nhead, M), value (B, dv, nhead, M) -> (B, dv, nhead, N), the scale
    1 / sqrt(dim).  No (B, nhead, N, M) tensor: the output, and where the grid is
    small a scratch of the output's order."""
    _front.forward_only("multi_head_attention", query, key, value)
    q = _f32(query, "query", "(B, dim, nhead, N)", 4)
    k, v = _f32(key, "key", "(B, dim, nhead, M)", 4, q.device), _f32(value, "value", "(B, dv, nhead, M)", 4, q.device)
    b, d, h, n = q.shape
    m, dv = k.shape[3], v.shape[1]
    if k.shape[:3] != (b, d, h):
        raise ValueError(f"key {tuple(k.shape)} must be (B={b}, dim={d}, nhead={h}, M)")
    if v.shape[0] != b or v.shape[2] != h or v.shape[3] != m:
        raise ValueError(f"value {tuple(v.shape)} must be (B={b}, dv, nhead={h}, M={m})")
    _channels("dim", d)
    _channels("dv", dv)
    if h < 1:
        raise ValueError("nhead must be >= 1")
    if m < 1:
        raise ValueError("key is empty (M = 0): a softmax over no keys is undefined")
    if max(n, m) > MAX_TOKENS:
        raise ValueError(f"N={n} or M={m} above {MAX_TOKENS}")
    out = torch.empty((b, dv, h, n), dtype=torch.float32, device=q.device)
    if b == 0 or n == 0:
        return out
    st = [(t.stride(0), t.stride(2), t.stride(1)) for t in (q, k, v, out)]
    _attention(q, k, v, out, b, h, n, m, d, dv, 1.0 / math.sqrt(d), st)
    return out


def overlap_scores(feats_norm, attn_scores, len_src, temperature):
    """NgeNet.py:173-179: feats_norm (n, C) unit rows, attn_scores (n, 1), the
    first len_src rows the source.  Returns ol_scores (n, 1): for a source row
    softmax_j(<f_i, f_j> / temperature) over the target rows times their
    attn_scores, and the same with the clouds swapped.  Two fused calls (one
    head, value width 1, scale 1 / temperature); the (n1, n2) inner product is
    never formed.  feats_norm is taken in place when it is the transposed view
    of a (C, n) tensor (stride 1 along n), as the reference passes it.
    `temperature` may be a one-element tensor (read once, on the host)."""
    _front.forward_only("overlap_scores", feats_norm, attn_scores)
    f = feats_norm
    if isinstance(f, torch.Tensor) and f.dim() == 2:
        f = f.t()                                   # (C, n): channel-major
    f = _f32(f, "feats_norm", "(n, C)", 2)
    c, n = f.shape
    a = attn_scores
    if not isinstance(a, torch.Tensor) or a.dim() != 2 or a.shape != (n, 1):
        raise ValueError(f"attn_scores must be (n={n}, 1)")
    a = _f32(a.t(), "attn_scores", "(n, 1)", 2, f.device)   # (1, n)
    _channels("C", c)
    n1 = int(len_src)
    if not 0 < n1 < n:
        raise ValueError(f"len_src={len_src} must leave both clouds non-empty (n={n})")
    if n > MAX_TOKENS:
        raise ValueError(f"n={n} above {MAX_TOKENS}")
    t = float(temperature)
    if not (t > 0 and math.isfinite(t)):
        raise ValueError(f"temperature={t} must be positive and finite")
    out = torch.empty((1, n), dtype=torch.float32, device=f.device)
    for (qs, ks) in ((slice(0, n1), slice(n1, n)), (slice(n1, n), slice(0, n1))):
        q, k, v, o = f[:, qs], f[:, ks], a[:, ks], out[:, qs]
        st = [(0, 0, x.stride(0)) for x in (q, k, v, o)]
        _attention(q, k, v, o, 1, 1, q.shape[1], k.shape[1], c, 1, 1.0 / t, st)
    return out.t()


def offset_attention(x_q, x_k, x_v, ol_score=None):
    """TFMR.py:97-103 fused: x_q, x_k (B, d, N), x_v (B, C, N), ol_score (B, N) or
    None ->  x_r (B, C, N) with
      a_ij = ol_i <x_q[:, i], x_k[:, j]>,  P = softmax_j a,
      x_r[:, j] = sum_i x_v[:, i] P_ij / (1e-9 + sum_i P_ij).
    Two sweeps over the scores, neither stores them: the scratch is 8 B N bytes."""
    _front.forward_only("offset_attention", x_q, x_k, x_v, ol_score)
    q = _f32(x_q, "x_q", "(B, d, N)", 3)
    k, v = _f32(x_k, "x_k", "(B, d, N)", 3, q.device), _f32(x_v, "x_v", "(B, C, N)", 3, q.device)
    b, d, n = q.shape
    dv = v.shape[1]
    if k.shape != q.shape:
        raise ValueError(f"x_k {tuple(k.shape)} must match x_q {tuple(q.shape)}")
    if v.shape[0] != b or v.shape[2] != n:
        raise ValueError(f"x_v {tuple(v.shape)} must be (B={b}, C, N={n})")
    r = None
    if ol_score is not None:
        r = _f32(ol_score, "ol_score", "(B, N)", 2, q.device)
        if r.shape != (b, n):
            raise ValueError(f"ol_score {tuple(r.shape)} must be (B={b}, N={n})")
    _channels("d", d)
    _channels("C", dv)
    if n > MAX_TOKENS:
        raise ValueError(f"N={n} above {MAX_TOKENS}")
    out = torch.empty((b, dv, n), dtype=torch.float32, device=q.device)
    if b == 0 or n == 0:
        return out
    lib = _lib.load()
    dev = q.device
    with torch.cuda.device(dev):
        ws = _front.scratch(lib.pcr_offset_attention_scratch_bytes(b, n, d, dv), dev)
        _lib.call("pcr_offset_attention_forward", _lib.ptr(q), q.stride(0), q.stride(1), _lib.ptr(k),
                  k.stride(0), k.stride(1), _lib.ptr(v), v.stride(0), v.stride(1), _lib.ptr(r),
                  r.stride(0) if r is not None else 0, _lib.ptr(out), out.stride(0), out.stride(1), b, n, d,
                  dv, _lib.ptr(ws), _lib.stream_handle(dev))
    return out


class CrossAttention(torch.nn.Module):
    """The reference's Cross_Attention (information_interactive.py:180-214) on the
    fused call, with its attribute names and state-dict keys (`conv`, `q_conv`,
    `k_conv`, `v_conv`, `mlp.0`, `mlp.3`).  `like` (fuse()): an existing block
    whose submodules are shared instead of created."""

    def __init__(self, feat_dims, nhead, like=None):
        super().__init__()
        if feat_dims % nhead != 0:
            raise ValueError(f"feat_dims={feat_dims} is no multiple of nhead={nhead}")
        self.feats_dim = int(feat_dims)
        self.nhead = int(nhead)
        nn = torch.nn
        if like is not None:
            self.conv, self.q_conv, self.k_conv, self.v_conv = like.conv, like.q_conv, like.k_conv, like.v_conv
            self.mlp = like.mlp
            return
        self.conv = nn.Conv1d(feat_dims, feat_dims, 1)
        self.q_conv, self.k_conv, self.v_conv = (nn.Conv1d(feat_dims, feat_dims, 1) for _ in range(3))
        for c in (self.q_conv, self.k_conv, self.v_conv):   # the reference starts them as copies of conv
            c.load_state_dict(self.conv.state_dict())
        self.mlp = nn.Sequential(nn.Conv1d(feat_dims * 2, feat_dims * 2, 1), nn.InstanceNorm1d(feat_dims * 2),
                                 nn.ReLU(inplace=True), nn.Conv1d(feat_dims * 2, feat_dims, 1))

    def forward(self, feats1, feats2):
        """feats1 (B, C, N), feats2 (B, C, M) -> (B, C, N)."""
        b = feats1.size(0)
        dims = self.feats_dim // self.nhead
        query = self.q_conv(feats1).reshape(b, dims, self.nhead, -1)
        key = self.k_conv(feats2).reshape(b, dims, self.nhead, -1)
        value = self.v_conv(feats2).reshape(b, dims, self.nhead, -1)
        feats = multi_head_attention(query, key, value).reshape(b, self.feats_dim, -1)
        feats = self.conv(feats)
        return self.mlp(torch.cat([feats1, feats], dim=1))


class OverlapAttentionBlock(torch.nn.Module):
    """The reference's OverlapAttentionBlock (TFMR.py:76-106) on the fused call,
    with its attribute names and state-dict keys; q_conv and k_conv share one
    weight.  `like` (fuse()): an existing block whose submodules are shared."""

    def __init__(self, channels, like=None):
        super().__init__()
        nn = torch.nn
        if like is not None:
            self.q_conv, self.k_conv, self.v_conv = like.q_conv, like.k_conv, like.v_conv
            self.trans_conv, self.after_norm, self.act = like.trans_conv, like.after_norm, like.act
            return
        self.q_conv = nn.Conv1d(channels, channels // 4, 1, bias=False)
        self.k_conv = nn.Conv1d(channels, channels // 4, 1, bias=False)
        self.q_conv.weight = self.k_conv.weight
        self.v_conv = nn.Conv1d(channels, channels, 1)
        self.trans_conv = nn.Conv1d(channels, channels, 1)
        self.after_norm = nn.GroupNorm(channels // 32, channels)
        self.act = nn.ReLU()

    def forward(self, x, ol_score):
        """x (B, C, N), ol_score (B, N) or None -> (B, C, N)."""
        x_r = offset_attention(self.q_conv(x), self.k_conv(x), self.v_conv(x), ol_score)
        x_r = self.act(self.after_norm(self.trans_conv(x - x_r)))
        return x + x_r


def fuse(model):
    """Swap a loaded network's attention blocks for the fused ones, in place: every
    child of class name `Cross_Attention` with q_conv, k_conv, v_conv, conv, mlp,
    nhead and feats_dim becomes a CrossAttention, every `OverlapAttentionBlock`
    with q_conv, k_conv, v_conv, trans_conv, after_norm and act an
    OverlapAttentionBlock of this module.  The new blocks hold the SAME
    submodules, so parameters (and the q/k weight tying) are shared, not
    copied.  Returns (cross-attention blocks swapped, overlap blocks swapped); a
    second call finds nothing and returns (0, 0)."""
    kinds = ((("Cross_Attention", ("q_conv", "k_conv", "v_conv", "conv", "mlp", "nhead", "feats_dim")),
              lambda c: CrossAttention(c.feats_dim, c.nhead, like=c)),
             (("OverlapAttentionBlock", ("q_conv", "k_conv", "v_conv", "trans_conv", "after_norm", "act")),
              lambda c: OverlapAttentionBlock(c.v_conv.in_channels, like=c)))
    return _front.swap_children(model, kinds, errors=(), skip=(CrossAttention, OverlapAttentionBlock))
