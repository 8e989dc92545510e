"""Point-set sampling and grouping on the GPU: drop-ins for the reference's
``fps`` / ``gather_points`` / ``ball_query`` / ``sample_and_group`` and the fused
point-pair-feature group behind ``LocalFeatue`` and ``PPF``, and for the k-NN
graph and edge features (``get_graph_features``) behind NgeNet's ``GCN``.

Reference surface:
  * ``ROPNet/src/models/model_utils.py:6-102``, consumed by
    ``LocalFeatue.forward`` (``TFMR.py:48-71``), once per iteration and cloud;
  * ``c2p-net/ngenet/utils/process.py:57-115``, consumed by ``PPF.forward``
    (``ngenet/models/information_interactive.py:48-84``, ``ppf_k: 64``, radius
    ``0.025 * 32``);
  * ``c2p-net/ngenet/models/information_interactive.py:7-23``
    (``get_graph_features``), consumed twice per cloud by ``GCN.forward``
    (``:107-130``, ``dgcnn_k: 10``, ``gnn_feats_dim: 256``);
  * ``dip/preprocess_lrf.py:97`` samples with ``torch_cluster.fps``.

The reference forms a ``(B, N, N)`` f32 distance matrix and a ``(B, N, N)``
int64 index tensor that it sorts; ``fps`` is a Python loop of ``M`` iterations.
Here every call goes through libpcr.so (``pcr_fps``, ``pcr_ball_query``,
``pcr_group_ppf``, ``pcr_knn_graph``, ``pcr_edge_features``; contract in
``include/pcr_api.h``) on torch's current stream: squared distances in the
direct form ``(dx*dx + dy*dy) + dz*dz``, a point at exactly the radius is
inside, ties go to the lowest index.

``knn_graph`` orders a point's cloud by ``(d2, index)`` and drops rank 0 as the
reference drops column 0 of its ``topk``; the reference breaks exact ties
arbitrarily and ranks by the expanded form, so it is the neighbour *set* (all
that ``GCN``'s max over the k axis sees) that equals the reference's, not
always the order.  ``graph_features`` is the gather ``[f_i, f_j - f_i]``, exact.

What consumes ``local_ppf_features`` and ``knn_graph`` -- the Conv2d / norm /
activation / max chains of ``LocalFeatureFused`` and ``GCN`` -- is fused in
``groupmlp`` (``group_mlp``, ``edge_conv``): with it neither ``graph_features``'
``(B, N, k, 2C)`` tensor nor a ``(B, C, K, N)`` activation is needed.

Like ``nndistance``, the module raises on CPU tensors (there is no fallback).
The ops are forward-only: an input that requires grad while grad mode is on
raises instead of silently cutting the graph.
"""
from __future__ import annotations

import torch

from . import _front, _lib

__all__ = ["fps", "gather_points", "ball_query", "sample_and_group", "local_ppf_features",
           "knn_graph", "graph_features"]


def _cloud(name, t, last=3):
    _front.tensor(t, name, "(B, N, {2})" if last else "(B, N, C)", (None, None, last))
    if t.shape[2] < 1:
        raise ValueError(f"{name} must be (B, N, C), got {tuple(t.shape)} without channels")
    _front.forward_only(name, t, message=f"{name} requires grad: the grouping ops are forward-only; call them "
                        "under torch.no_grad() or pass a detached tensor")
    return t.contiguous()   # the caller's own tensor: sample_and_group hands it back


def _r2(radius):
    # the reference compares f32 distances with the Python scalar radius ** 2
    return float(radius) * float(radius)


def fps(xyz, M, start=None):
    """Farthest-point sampling: ``(B, M)`` int64 indices (model_utils.py:6-24).

    ``start`` (``(B,)`` integers in ``[0, N)``) is the first index of every
    cloud; ``None`` draws it on the host exactly as the reference does, so the
    same torch seed gives the same sample."""
    xyz = _cloud("xyz", xyz)
    B, N, _ = xyz.shape
    M = int(M)
    if N < 1 or M < 1:
        raise ValueError(f"fps needs N >= 1 and M >= 1, got N={N}, M={M}")
    if start is None:
        start = torch.randint(0, N, size=(B,), dtype=torch.long)
    start = torch.as_tensor(start)
    if tuple(start.shape) != (B,) or start.dtype.is_floating_point:
        raise ValueError(f"start must be {B} integers, got {tuple(start.shape)} {start.dtype}")
    if B and (int(start.min()) < 0 or int(start.max()) >= N):
        raise ValueError(f"start must lie in [0, {N})")
    start = start.to(device=xyz.device, dtype=torch.int32).contiguous()
    idx = torch.empty(B, M, dtype=torch.int32, device=xyz.device)
    with torch.cuda.device(xyz.device):
        _lib.call("pcr_fps", _lib.ptr(xyz), _lib.ptr(start), B, N, M, _lib.ptr(idx),
                  _lib.stream_handle(xyz.device))
    return idx.long()


def gather_points(points, inds):
    """``points (B, N, C)`` at ``inds (B, M)`` or ``(B, M, K)`` (model_utils.py:27-41)."""
    B = points.shape[0]
    batch = torch.arange(B, device=points.device).view([B] + [1] * (inds.dim() - 1))
    return points[batch, inds.long(), :]


def _ball_query(xyz, new_xyz, radius, K, want_count):
    xyz = _cloud("xyz", xyz)
    new_xyz = _cloud("new_xyz", new_xyz)
    if xyz.shape[0] != new_xyz.shape[0] or xyz.device != new_xyz.device:
        raise ValueError("xyz and new_xyz must share batch size and device")
    B, N, _ = xyz.shape
    Q = new_xyz.shape[1]
    K = int(K)
    if N < 1 or K < 1:
        raise ValueError(f"ball_query needs N >= 1 and K >= 1, got N={N}, K={K}")
    k = min(K, N)   # the reference's sorted[:, :, :K] has min(K, N) columns
    idx = torch.empty(B, Q, k, dtype=torch.int32, device=xyz.device)
    count = torch.empty(B, Q, dtype=torch.int32, device=xyz.device) if want_count else None
    with torch.cuda.device(xyz.device):
        _lib.call("pcr_ball_query", _lib.ptr(xyz), _lib.ptr(new_xyz), B, N, Q, _r2(radius), k,
                  _lib.ptr(idx), _lib.ptr(count), _lib.stream_handle(xyz.device))
    return idx, count


def ball_query(xyz, new_xyz, radius, K, rt_density=False):
    """``(B, M, min(K, N))`` int64: per query the first K indices, ascending, of the
    points within ``radius`` (inclusive), padded with the row's first neighbour;
    a row without neighbours holds ``N`` (model_utils.py:44-67).  With
    ``rt_density`` also the float density, neighbours before the cap over ``N``."""
    idx, count = _ball_query(xyz, new_xyz, radius, K, rt_density)
    if rt_density:
        # the quotient of two integers, rounded once to f32 (the reference divides
        # on the host); through f64 so that the device's f32 divide has no say
        return idx.long(), (count.double() / xyz.shape[1]).float()
    return idx.long()


def sample_and_group(xyz, points, M, radius, K, use_xyz=True, rt_density=False):
    """The reference's return tuple (model_utils.py:70-102): ``new_xyz (B, M, 3)``,
    ``new_points (B, M, K, C [+ 3])``, ``grouped_inds (B, M, K)``, ``grouped_xyz``
    (centred on ``new_xyz``) and, with ``rt_density``, the density.  ``M < 0``
    makes every point a centre."""
    xyz = _cloud("xyz", xyz)
    _front.forward_only("points", points, message="points requires grad: the grouping ops are forward-only")
    new_xyz = xyz if M < 0 else gather_points(xyz, fps(xyz, M))
    res = ball_query(xyz, new_xyz, radius, K, rt_density=rt_density)
    grouped_inds, density = res if rt_density else (res, None)
    grouped_xyz = gather_points(xyz, grouped_inds) - new_xyz.unsqueeze(2)
    if points is not None:
        grouped_points = gather_points(points, grouped_inds)
        new_points = (torch.cat((grouped_xyz.float(), grouped_points.float()), dim=-1)
                      if use_xyz else grouped_points)
    else:
        new_points = grouped_xyz
    if rt_density:
        return new_xyz, new_points, grouped_inds, grouped_xyz, density
    return new_xyz, new_points, grouped_inds, grouped_xyz


def local_ppf_features(xyz, normals, radius, K, channels_first=True, return_inds=False):
    """The group that ``LocalFeatue.forward(normals, xyz, use_ppf=True)`` hands to
    its Conv2d (TFMR.py:56-71), in one call: every point a centre, K ball-query
    neighbours, channels ``x_i`` (3), ``g = x_j - x_i`` (3) and, with normals,
    ``angle(n_i, g)``, ``angle(n_j, g)``, ``angle(n_i, n_j)``, ``|g|``.

    Returns ``(B, C, K, N)`` (``channels_first``, the layout Conv2d consumes) or
    ``(B, N, K, C)``, C = 10 with normals and 6 with ``normals=None``; with
    ``return_inds`` also the ``(B, N, K)`` int64 neighbour indices.  ``K <= N``."""
    xyz = _cloud("xyz", xyz)
    B, N, _ = xyz.shape
    K = int(K)
    if N < 1 or K < 1 or K > N:
        raise ValueError(f"local_ppf_features needs 1 <= K <= N, got N={N}, K={K}")
    if normals is not None:
        normals = _cloud("normals", normals)
        if normals.shape != xyz.shape or normals.device != xyz.device:
            raise ValueError("normals must match xyz in shape and device")
    C = 10 if normals is not None else 6
    shape = (B, C, K, N) if channels_first else (B, N, K, C)
    feat = torch.empty(shape, dtype=torch.float32, device=xyz.device)
    idx = torch.empty(B, N, K, dtype=torch.int32, device=xyz.device) if return_inds else None
    with torch.cuda.device(xyz.device):
        _lib.call("pcr_group_ppf", _lib.ptr(xyz), _lib.ptr(normals), B, N, _r2(radius), K,
                  1 if channels_first else 0, _lib.ptr(feat), _lib.ptr(idx),
                  _lib.stream_handle(xyz.device))
    if return_inds:
        return feat, idx.long()
    return feat


_KNN_MAX_K = 63   # pcr_knn_graph: k + 1 keys fit one wave


def _knn(coords, k, want_dists):
    coords = _cloud("coords", coords)
    B, N, _ = coords.shape
    k = int(k)
    if not 1 <= k <= _KNN_MAX_K:
        raise ValueError(f"k={k} outside 1..{_KNN_MAX_K}")
    if N < 1:
        raise ValueError(f"knn_graph needs N >= 1, got N={N}")
    kk = min(k, N - 1)
    idx = torch.empty(B, N, kk, dtype=torch.int32, device=coords.device)
    d2 = torch.empty(B, N, kk, dtype=torch.float32, device=coords.device) if want_dists else None
    if B and kk:
        with torch.cuda.device(coords.device):
            _lib.call("pcr_knn_graph", _lib.ptr(coords), B, N, k, _lib.ptr(idx), _lib.ptr(d2),
                      _lib.stream_handle(coords.device))
    return idx, d2


def knn_graph(coords, k, return_dists=False):
    """``(B, N, min(k, N - 1))`` int64: per point the indices of its k nearest
    other points, nearest first (``get_graph_features``' ``inds``,
    information_interactive.py:16-19).  All N points, the point itself included,
    are ranked by ``(d2, index)`` and rank 0 is dropped, as the reference drops
    column 0: that is the point itself unless a lower-index point coincides with
    it.  ``1 <= k <= 63``.  With ``return_dists`` also the f32 squared distances,
    ascending."""
    idx, d2 = _knn(coords, k, return_dists)
    if return_dists:
        return idx.long(), d2
    return idx.long()


def graph_features(feats, coords=None, k=10, inds=None, channels_first=False, return_inds=False):
    """``get_graph_features(feats, coords, k)`` (information_interactive.py:7-23):
    ``(B, N, kk, 2C)`` with ``[..., :C] = f_i`` and ``[..., C:] = f_j - f_i`` over
    the ``kk = min(k, N - 1)`` nearest neighbours j of i; ``channels_first`` gives
    the same values as ``(B, 2C, N, kk)``, the layout ``GCN`` hands its Conv2d.

    Exactly one of ``coords (B, N, 3)`` and ``inds (B, N, kk)`` (integers in
    ``[0, N)``, e.g. from ``knn_graph``) is given: ``inds`` lets ``GCN.forward``
    build the graph once for its two calls.  With ``return_inds`` also the
    ``(B, N, kk)`` int64 indices."""
    feats = _cloud("feats", feats, last=None)
    B, N, C = feats.shape
    if (coords is None) == (inds is None):
        raise ValueError("graph_features needs exactly one of coords and inds")
    if coords is not None:
        if not isinstance(coords, torch.Tensor) or coords.dim() != 3 or \
                tuple(coords.shape[:2]) != (B, N) or coords.device != feats.device:
            raise ValueError("coords must match feats in batch size, point count and device")
        idx, _ = _knn(coords, k, False)
    else:
        if not isinstance(inds, torch.Tensor) or inds.dtype.is_floating_point or \
                inds.dtype == torch.bool:
            raise ValueError("inds must be an integer tensor")
        if inds.dim() != 3 or tuple(inds.shape[:2]) != (B, N) or inds.device != feats.device:
            raise ValueError(f"inds must be ({B}, {N}, kk) on feats' device, got {tuple(inds.shape)}")
        if inds.shape[2] > _KNN_MAX_K:
            raise ValueError(f"inds has {inds.shape[2]} columns, outside 0..{_KNN_MAX_K}")
        idx = inds.to(torch.int32).contiguous()
    kk = idx.shape[2]
    shape = (B, 2 * C, N, kk) if channels_first else (B, N, kk, 2 * C)
    out = torch.empty(shape, dtype=torch.float32, device=feats.device)
    if B and kk:
        with torch.cuda.device(feats.device):
            _lib.call("pcr_edge_features", _lib.ptr(feats), _lib.ptr(idx), B, N, C, kk,
                      1 if channels_first else 0, _lib.ptr(out), _lib.stream_handle(feats.device))
    if return_inds:
        return out, idx.long()
    return out
