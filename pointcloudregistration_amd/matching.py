"""Similarity top-k matching on the GPU: the correspondence stage of ROPNet's
``TFMRModule.forward`` (``ROPNet/src/models/TFMR.py:226-257``) and the
normalise / sort / gather lines in front of it (``TFMR.py:195-200, 214-219``).

The reference forms three ``(B, N1, M1)`` f32 tensors (similarity, mask,
product) over about a dozen launches: ``bmm``, ``max``, ``sort``, ``gather``,
``topk``, ``zeros_like`` + ``index_put``, a normalisation and a second ``bmm``.
Here the whole stage is three launches of libpcr.so (``pcr_similarity_topk``,
``pcr_tfmr_select``; contract in ``include/pcr_api.h``) on torch's current
stream, and no ``(B, N1, M1)`` tensor exists at any point: the similarity is
the f32 ``fmaf`` chain over the channels in ascending order (bit for bit what
the f32 MFMA computes), each row keeps its k largest by (value descending,
index ascending), the rows are ordered by (best value descending, index
ascending), and the kept rows' weights ``v / (sum(v) + 1e-8)`` and
``tgt_corr = sum(w * tgt[idx])`` are evaluated in f32, one rounding per
operation.  The returned tuple feeds ``procrustes.weighted_icp`` unchanged.

Gradients.  The reference differentiates through the similarity values at the
top-k positions.  When an input requires grad and grad mode is on, ``sel`` and
``idx`` still come from the kernels (they are constant with respect to the
inputs), and the values, the weights and ``tgt_corr`` are re-evaluated with
torch ops on the gathered rows only (``B x N2 x k x C`` work, no dense tensor)
so that autograd sees them.  The two modes differ by rounding: the torch
re-evaluation sums the channels in torch's order, not as the fmaf chain.

Like ``grouping``, the module raises on CPU tensors (there is no fallback).
"""
from __future__ import annotations

import torch

from . import _front, _lib

__all__ = ["similarity_topk", "tfmr_match", "tfmr_correspondences"]

MAX_TOPK = 8


def _f32(name, t, last=None):
    _front.tensor(t, name, "(B, N, C)" if last is None else "(B, N, {2})", (None, None, last))
    return t   # not detached: tfmr_match differentiates through the gathered rows


def _features(fx, fy, k):
    fx, fy = _f32("fx", fx), _f32("fy", fy)
    if fx.shape[0] != fy.shape[0] or fx.shape[2] != fy.shape[2] or fx.device != fy.device:
        raise ValueError(f"fx {tuple(fx.shape)} and fy {tuple(fy.shape)} must share batch size, "
                         "feature width and device")
    B, N1, C = fx.shape
    M1 = fy.shape[1]
    k = int(k)
    if N1 < 1 or M1 < 1 or C < 1:
        raise ValueError(f"similarity_topk needs N1, M1, C >= 1, got {N1}, {M1}, {C}")
    if not 1 <= k <= min(MAX_TOPK, M1):
        raise ValueError(f"k={k} must lie in 1 .. min({MAX_TOPK}, M1={M1})")
    return fx, fy, B, N1, M1, C, k


def _scratch(B, N1, M1, C, k, device):
    # never empty: torch's caching allocator hands out 512-byte aligned blocks; the library checks 256
    return _front.scratch(_lib.load().pcr_tfmr_scratch_bytes(B, N1, M1, C, k), device, at_least=1,
                          who="pcr_tfmr_scratch_bytes: ")


def _topk(fx, fy, B, N1, M1, C, k):
    """val, idx (int32) and the scratch that holds the rows' selection keys."""
    fx, fy = fx.detach().contiguous(), fy.detach().contiguous()
    val = torch.empty(B, N1, k, dtype=torch.float32, device=fx.device)
    idx = torch.empty(B, N1, k, dtype=torch.int32, device=fx.device)
    scratch = _scratch(B, N1, M1, C, k, fx.device)
    with torch.cuda.device(fx.device):
        _lib.call("pcr_similarity_topk", _lib.ptr(fx), _lib.ptr(fy), B, N1, M1, C, k, _lib.ptr(val),
                  _lib.ptr(idx), _lib.ptr(scratch), _lib.stream_handle(fx.device))
    return val, idx, scratch


def similarity_topk(fx, fy, k):
    """``val (B, N1, k)`` f32 and ``idx (B, N1, k)`` int64: per row of
    ``fx (B, N1, C)`` the k largest inner products with the rows of
    ``fy (B, M1, C)``, by (value descending, index ascending).  Forward-only:
    an input that requires grad while grad mode is on raises instead of silently
    cutting the graph (``tfmr_match`` has the differentiable form)."""
    fx, fy, B, N1, M1, C, k = _features(fx, fy, k)
    _front.forward_only("similarity_topk", fx, fy, message="similarity_topk is forward-only: call it under "
                        "torch.no_grad() or pass detached tensors; tfmr_match differentiates through the top-k values")
    val, idx, _ = _topk(fx, fy, B, N1, M1, C, k)
    return val, idx.long()


def tfmr_match(fx, fy, src, tgt, x_ol_score, top_prob, topk, return_details=False):
    """``TFMR.py:226-257`` on normalised, gathered inputs: ``fx (B, N1, C)``,
    ``fy (B, M1, C)``, ``src (B, N1, 3)``, ``tgt (B, M1, 3)`` f32 and
    ``x_ol_score (B, N)`` with ``N >= N1`` (the sorted overlap scores).

    Returns the reference's tuple ``(src_sel (B, N2, 3), tgt_corr (B, N2, 3),
    icp_weights (B, N2), similarity_max_inds (B, N2) int64)`` with
    ``N2 = int(top_prob * N1)``; with ``return_details`` also a dict of the
    kept rows' ``idx (B, N2, topk)`` int64 and ``weights (B, N2, topk)``."""
    fx, fy, B, N1, M1, C, k = _features(fx, fy, topk)
    src, tgt = _f32("src", src, 3), _f32("tgt", tgt, 3)
    if tuple(src.shape[:2]) != (B, N1) or tuple(tgt.shape[:2]) != (B, M1):
        raise ValueError(f"src {tuple(src.shape)} / tgt {tuple(tgt.shape)} do not match the features")
    if not isinstance(x_ol_score, torch.Tensor) or x_ol_score.dim() != 2 or x_ol_score.shape[0] != B \
            or x_ol_score.shape[1] < N1:
        raise ValueError(f"x_ol_score must be (B, N >= N1), got {tuple(getattr(x_ol_score, 'shape', ()))}")
    if any(t.device != fx.device for t in (src, tgt, x_ol_score)):
        raise ValueError("all inputs must live on one device")
    n_keep = int(top_prob * N1)
    if not 0 <= n_keep <= N1:
        raise ValueError(f"top_prob={top_prob} keeps {n_keep} of {N1} rows")
    dev = fx.device
    sel = torch.empty(B, n_keep, dtype=torch.int32, device=dev)
    w = torch.empty(B, n_keep, k, dtype=torch.float32, device=dev)
    corr = torch.empty(B, n_keep, 3, dtype=torch.float32, device=dev)
    idx_keep = torch.empty(B, n_keep, k, dtype=torch.int32, device=dev)
    if B > 0 and n_keep > 0:
        val, idx, scratch = _topk(fx, fy, B, N1, M1, C, k)
        tgt_c = tgt.detach().contiguous()
        with torch.cuda.device(dev):
            _lib.call("pcr_tfmr_select", _lib.ptr(val), _lib.ptr(idx), _lib.ptr(tgt_c), B, N1, M1, k, n_keep,
                      _lib.ptr(sel), _lib.ptr(w), _lib.ptr(corr), _lib.ptr(idx_keep), _lib.ptr(scratch),
                      _lib.stream_handle(dev))
    sel, idx_keep = sel.long(), idx_keep.long()
    bi = torch.arange(B, device=dev).view(B, 1)
    if torch.is_grad_enabled() and any(t.requires_grad for t in (fx, fy, tgt)):
        # sel and idx are constants; the values at them, the weights and tgt_corr
        # through torch ops on the gathered rows, in the contract's order
        v = (fx[bi, sel][:, :, None, :] * fy[bi[:, :, None], idx_keep]).sum(-1)   # (B,N2,k)
        s = v[..., 0]
        for t in range(1, k):
            s = s + v[..., t]
        w = v / (s + 1e-8)[..., None]
        tk = tgt[bi[:, :, None], idx_keep]                                      # (B,N2,k,3)
        corr = w[..., 0, None] * tk[..., 0, :]
        for t in range(1, k):
            corr = corr + w[..., t, None] * tk[..., t, :]
    out = (src[bi, sel], corr, x_ol_score[bi, sel], sel)
    if return_details:
        return out + (dict(idx=idx_keep, weights=w),)
    return out


def tfmr_correspondences(f_x_attn, f_y_attn, src, tgt, x_ol_score, y_ol_score, N1, M1, top_prob, topk):
    """``TFMR.py:195-200, 214-219`` and then ``tfmr_match``: normalise the
    attention outputs ``(B, N, C)`` / ``(B, M, C)`` as ``f / (|f| + 1e-8)``, sort
    the overlap scores in descending order, keep the first ``N1`` / ``M1`` points
    and gather features and clouds.  The sorts are stable (the reference's are
    not, so its order among equal scores is unspecified; here the lowest index
    comes first)."""
    fxn = f_x_attn / (torch.norm(f_x_attn, dim=-1, keepdim=True) + 1e-8)
    fyn = f_y_attn / (torch.norm(f_y_attn, dim=-1, keepdim=True) + 1e-8)
    x_ol_sorted, x_inds = torch.sort(x_ol_score, dim=-1, descending=True, stable=True)
    y_inds = torch.sort(y_ol_score, dim=-1, descending=True, stable=True)[1][:, :M1]
    x_inds = x_inds[:, :N1]
    B = src.shape[0]
    bi = torch.arange(B, device=src.device).view(B, 1)
    return tfmr_match(fxn[bi, x_inds], fyn[bi, y_inds], src[bi, x_inds], tgt[bi, y_inds], x_ol_sorted,
                      top_prob, topk)
