"""f2: KPConv input pyramid helpers on the GPU (drop-in for ngenet's cpp_wrappers).

Mirrors of the reference's Python-facing functions:

* ``subsample_batch``  -- cpp_subsampling.subsample_batch
  (c2p-net/ngenet/cpp_wrappers/cpp_subsampling/wrapper.cpp:59-330)
* ``batch_query``      -- cpp_neighbors.batch_query
  (cpp_neighbors/wrapper.cpp:63-230)
* ``batch_grid_subsampling`` / ``batch_neighbors`` -- the dataloader wrappers
  (c2p-net/ngenet/data/dataloader.py:12-66), returning torch tensors.

Same argument names, defaults and results (subsampled points and features
bit-identical and in the same order; neighbour rows identical, including the
reference's order among exactly equal distances, which the library replays on
the host for the rows that hold them, see DESIGN.md "f2"), RuntimeError("Error") on an
empty result like the wrappers.  The work runs in libpcr (pcr_grid_subsample,
pcr_radius_count / pcr_radius_neighbors); there is no CPU path.  numpy / CPU
inputs give numpy outputs (as the reference); CUDA tensors stay on the device.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _front, _lib


def _device(*xs):
    for x in xs:
        if isinstance(x, torch.Tensor) and x.is_cuda:
            return x.device, True
    return torch.device("cuda", torch.cuda.current_device()), False


def _points(x, dev, name, ncol=3):
    t = torch.as_tensor(np.asarray(x) if not isinstance(x, torch.Tensor) else x)
    t = t.to(device=dev, dtype=torch.float32).contiguous()
    if ncol is not None and (t.dim() != 2 or t.shape[1] != ncol):
        raise RuntimeError(f"Wrong dimensions : {name}.shape is not (N, {ncol})")
    return t


def _lengths(x, name):
    a = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    a = np.ascontiguousarray(a, dtype=np.int32)
    if a.ndim != 1:
        raise RuntimeError(f"Wrong dimensions : {name}.shape is not (B,) ")
    return a


def _out(t, on_device):
    return t if on_device else t.cpu().numpy()


def subsample_batch(points, batches, features=None, classes=None, sampleDl=0.1,
                    method="barycenters", max_p=0, verbose=0):
    """Barycentric voxel-grid subsampling of a stack of clouds.

    Returns (s_points (M,3) f32, s_len (B,) int32[, s_features (M,d) f32])."""
    if method not in ("barycenters", "voxelcenters"):
        raise RuntimeError('Error parsing method. Valid method names are "barycenters" and '
                           '"voxelcenters" ')
    if classes is not None:
        # the label vote (grid_subsampling.cpp:97-102) is unused by ngenet's callers
        raise NotImplementedError("subsample_batch: classes are not supported")
    dev, on_dev = _device(points, features)
    pts = _points(points, dev, "points")
    bl = _lengths(batches, "batches")
    n = pts.shape[0]
    feat, fdim = None, 0
    if features is not None:
        feat = _points(features, dev, "features", None)
        if feat.dim() == 1:
            feat = feat.reshape(-1, 1)
        if feat.dim() != 2 or feat.shape[0] != n:
            raise RuntimeError("Wrong dimensions : features.shape is not (N, d)")
        fdim = feat.shape[1]
    out_p = torch.empty((max(n, 1), 3), dtype=torch.float32, device=dev)
    out_f = torch.empty((max(n, 1), max(fdim, 1)), dtype=torch.float32, device=dev) if feat is not None else None
    out_len = np.zeros(bl.shape[0], np.int32)
    total = ctypes.c_int32(0)
    with torch.cuda.device(dev):
        _lib.call("pcr_grid_subsample", _lib.ptr(pts), n, bl.ctypes.data, bl.shape[0],
                  _lib.ptr(feat), fdim, float(sampleDl), int(max_p), _lib.ptr(out_p),
                  _lib.ptr(out_f), out_len.ctypes.data, ctypes.byref(total),
                  _lib.stream_handle(dev))
    m = total.value
    if m < 1:
        raise RuntimeError("Error")
    s_len = torch.from_numpy(out_len).to(dev) if on_dev else out_len
    res = (_out(out_p[:m], on_dev), s_len)
    if feat is not None:
        res = res + (_out(out_f[:m, :fdim], on_dev),)
    return res


def _neighbors(queries, supports, q_batches, s_batches, radius, max_nn):
    dev, on_dev = _device(queries, supports)
    q = _points(queries, dev, "query")
    s = _points(supports, dev, "support")
    qb = _lengths(q_batches, "queries_batches")
    sb = _lengths(s_batches, "supports_batches")
    if qb.shape[0] != sb.shape[0]:
        raise RuntimeError("Wrong number of batch elements: different for queries and supports ")
    nq, ns = q.shape[0], s.shape[0]
    mc = ctypes.c_int32(0)
    stream = _lib.stream_handle(dev)
    with torch.cuda.device(dev):
        _lib.call("pcr_radius_count", _lib.ptr(q), nq, _lib.ptr(s), ns, qb.ctypes.data,
                  sb.ctypes.data, qb.shape[0], float(radius), None, ctypes.byref(mc), stream)
        width = mc.value if max_nn <= 0 else min(mc.value, int(max_nn))
        out = torch.empty((nq, width), dtype=torch.int32, device=dev)
        if nq * width > 0:
            _lib.call("pcr_radius_neighbors", _lib.ptr(q), nq, _lib.ptr(s), ns, qb.ctypes.data,
                      sb.ctypes.data, qb.shape[0], float(radius), width, _lib.ptr(out), None,
                      stream)
    return out, mc.value, on_dev


def batch_query(queries, supports, q_batches, s_batches, radius=0.1):
    """Radius neighbours of every query among the supports of its batch:
    (Nq, max_count) int32 rows by ascending distance, padded with len(supports)."""
    out, mc, on_dev = _neighbors(queries, supports, q_batches, s_batches, radius, 0)
    if out.numel() < 1:
        raise RuntimeError("Error")
    return _out(out, on_dev)


def batch_neighbors(batch_queries, batch_supports, q_batches, s_batches, radius, max_nn):
    """dataloader.py:12-25: batch_query truncated to max_nn columns (if > 0), as a
    torch tensor (on the GPU when the inputs are CUDA tensors)."""
    out, mc, on_dev = _neighbors(batch_queries, batch_supports, q_batches, s_batches, radius,
                                 max_nn)
    if mc * out.shape[0] < 1:
        raise RuntimeError("Error")
    return out if on_dev else out.cpu()


def batch_grid_subsampling(points, batches_len, features=None, labels=None, sampleDl=0.1,
                           max_p=0, verbose=0, random_grid_orient=True):
    """dataloader.py:28-66 (points / features) returning torch tensors."""
    if labels is not None:
        raise NotImplementedError("batch_grid_subsampling: labels are not supported")
    res = subsample_batch(points, batches_len, features=features, sampleDl=sampleDl,
                          max_p=max_p, verbose=verbose)
    return tuple(r if isinstance(r, torch.Tensor) else torch.from_numpy(r) for r in res)


def collate_fn(list_data, config, neighborhood_limits, device=None):
    """dataloader.py:69-182 (collate_fn): stacks the items' clouds (src, tgt per
    item) and builds the KPConv input pyramid -- conv neighbours, strided grid
    subsampling with normals, pooling and upsampling neighbours per layer --
    with every neighbour search and subsampling in libpcr.  Arrays stay on the
    GPU between layers; the returned dict has the reference's keys and, as the
    reference, CPU tensors unless `device` names a CUDA device."""
    pts_l, raw_l, feats_l, norm_l, lens, transf_l, coors_l = [], [], [], [], [], [], []
    for item in list_data:
        pts_l += [item["src_points"], item["tgt_points"]]
        raw_l += [item["src_points_raw"], item["tgt_points_raw"]]
        feats_l += [item["src_feats"], item["tgt_feats"]]
        norm_l += [item["src_normals"], item["tgt_normals"]]
        lens += [len(item["src_points"]), len(item["tgt_feats"])]  # (:98-99, as the reference)
        transf_l.append(item["transf"])
        coors_l.append(torch.from_numpy(np.asarray(item["coors"])).long())
    dev = torch.device("cuda", torch.cuda.current_device())
    cat = lambda xs: torch.from_numpy(np.concatenate(xs, axis=0).astype(np.float32))  # noqa: E731
    points = cat(pts_l).to(dev)
    normals = cat(norm_l).to(dev)
    lengths = np.asarray(lens, np.int32)
    stack = pyramid(points, lengths, normals, config.architecture, config.first_subsampling_dl,
                    config.conv_radius, neighborhood_limits)
    out_dev = torch.device(device) if device is not None else torch.device("cpu")
    mv = lambda t: t.to(out_dev)  # noqa: E731
    return {
        "points": [mv(t) for t in stack["points"]],
        "neighbors": [mv(t) for t in stack["neighbors"]],
        "pools": [mv(t) for t in stack["pools"]],
        "upsamples": [mv(t) for t in stack["upsamples"]],
        "stacked_lengths": [mv(t) for t in stack["stacked_lengths"]],
        "feats": mv(cat(feats_l)),
        "normals": [mv(t) for t in stack["normals"]],
        "coors": coors_l,
        "transf": mv(torch.from_numpy(np.array(transf_l).astype(np.float32))),
        "batched_points_raw": mv(cat(raw_l)),
    }


def pyramid(points, lengths, normals, architecture, first_subsampling_dl, conv_radius,
            neighborhood_limits):
    """The layer loop of collate_fn (dataloader.py:116-167) on device tensors:
    points (N,3) f32 CUDA, lengths (B,) host int32, normals (N,3) f32 CUDA.
    Returns lists of CUDA tensors (neighbour indices int64, as .long() there)."""
    lengths = torch.as_tensor(np.asarray(lengths, np.int32))
    r_normal = first_subsampling_dl * conv_radius
    out = {"points": [], "neighbors": [], "pools": [], "upsamples": [], "stacked_lengths": [],
           "normals": []}
    layer = 0
    for block_i, block in enumerate(architecture):
        if "upsample" in block:
            break
        conv_i = pool_i = up_i = None
        if "strided" in block or "upsample" in architecture[block_i + 1]:
            conv_i = batch_neighbors(points, points, lengths, lengths, r_normal,
                                     neighborhood_limits[layer])
        if "strided" in block:
            voxel_size = 2 * r_normal / conv_radius
            new_points, new_len, new_normals = subsample_batch(points, lengths, features=normals,
                                                               sampleDl=voxel_size)
            new_len = new_len.cpu()
            pool_i = batch_neighbors(new_points, points, new_len, lengths, r_normal,
                                     neighborhood_limits[layer])
            up_i = batch_neighbors(points, new_points, lengths, new_len, 2 * r_normal,
                                   neighborhood_limits[layer])
        if conv_i is not None:
            out["points"].append(points)
            out["stacked_lengths"].append(lengths)
            out["normals"].append(normals)
            out["neighbors"].append(conv_i.long())
        if pool_i is not None:
            out["pools"].append(pool_i.long())
            out["upsamples"].append(up_i.long())
            points, lengths, normals = new_points, new_len, new_normals
            r_normal *= 2
            layer += 1
    return out


# ---------------------------------------------------------------------------
# The consumers of the pyramid: KPConv.forward and MaxPoolBlock.forward
# (c2p-net/ngenet/models/KPConv/blocks.py:73-128, 182-188) as one libpcr call
# each (pcr_kpconv_forward, pcr_neighbor_max; contract in include/pcr_api.h).
# Inference only: there is no backward.
# ---------------------------------------------------------------------------
MAX_KERNEL_POINTS = 16
MAX_NEIGHBORS = 256
MAX_CHANNELS = 2048
MAX_POOL_CHANNELS = 4096
_INFLUENCE = {"linear": 0, "constant": 1}


def _f32(t, name, ncol=None, dev=None):
    return _front.tensor(t, name, "(N, C)" if ncol is None else "(N, {1})", (None, ncol), dev, "floating",
                         torch.Tensor.contiguous)


def _indices(t, name, rows, dev):
    t = _front.tensor(t, name, "({0}, k)", (rows, None), dev, "index")
    if not 1 <= t.shape[1] <= MAX_NEIGHBORS:
        raise ValueError(f"{name} has k={t.shape[1]} columns, outside 1..{MAX_NEIGHBORS}")
    return t.contiguous()


def kpconv_forward(q_pts, s_pts, s_feats, neigh_inds, kernel_points, weights, KP_extent,
                   KP_influence="linear"):
    """KPConv.forward (blocks.py:73-128, aggregation 'sum') as one fused call:
    q_pts (n,3), s_pts (m,3), s_feats (m,C_in), neigh_inds (n,k) int32/int64 with
    every index outside [0, m) a pad, kernel_points (K,3), weights
    (K,C_in,C_out) -> (n,C_out) f32.  Nothing of size n k C_in, n k K or
    n K C_in is allocated: the output and m bytes of row flags."""
    if KP_influence not in _INFLUENCE:
        raise ValueError(f"KP_influence={KP_influence!r}: 'linear' or 'constant'")
    _front.forward_only("kpconv_forward", q_pts, s_pts, s_feats, kernel_points, weights)
    q = _f32(q_pts, "q_pts", 3)
    dev = q.device
    s, f = _f32(s_pts, "s_pts", 3, dev), _f32(s_feats, "s_feats", None, dev)
    kp = _f32(kernel_points, "kernel_points", 3, dev)
    if not isinstance(weights, torch.Tensor) or not weights.is_cuda or weights.dim() != 3 or weights.device != dev:
        raise ValueError(f"weights must be a CUDA tensor of shape (K, C_in, C_out) on {dev}")
    w = weights.detach().to(torch.float32).contiguous()
    n, m = q.shape[0], s.shape[0]
    K, c_in, c_out = w.shape
    if m < 1:
        raise ValueError("s_pts is empty")
    if f.shape != (m, c_in):
        raise ValueError(f"s_feats {tuple(f.shape)} must be (m={m}, C_in={c_in})")
    if kp.shape[0] != K or not 1 <= K <= MAX_KERNEL_POINTS:
        raise ValueError(f"kernel_points {tuple(kp.shape)} / weights {tuple(w.shape)}: K must agree and lie "
                         f"in 1..{MAX_KERNEL_POINTS}")
    if not (1 <= c_in <= MAX_CHANNELS and 1 <= c_out <= MAX_CHANNELS):
        raise ValueError(f"C_in={c_in}, C_out={c_out} must lie in 1..{MAX_CHANNELS}")
    idx = _indices(neigh_inds, "neigh_inds", n, dev)
    ext = float(KP_extent)
    if KP_influence == "linear" and not ext > 0:
        raise ValueError(f"KP_extent={KP_extent} must be > 0")
    out = torch.empty((n, c_out), dtype=torch.float32, device=dev)
    if n == 0:
        return out
    flags = torch.empty(m, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _lib.call("pcr_kpconv_forward", _lib.ptr(q), _lib.ptr(s), _lib.ptr(f), _lib.ptr(idx),
                  idx.element_size(), n, m, idx.shape[1], _lib.ptr(kp), _lib.ptr(w), K, c_in, c_out, ext,
                  _INFLUENCE[KP_influence], _lib.ptr(flags), _lib.ptr(out), _lib.stream_handle(dev))
    return out


def neighbor_max(feats, inds):
    """MaxPoolBlock.forward (blocks.py:182-188): out[i] = max over the columns of
    feats[inds[i]], a pad (index outside [0, m)) reading 0.  feats (m,C) f32,
    inds (n,k) int32/int64 -> (n,C) f32, exact."""
    _front.forward_only("neighbor_max", feats)
    f = _f32(feats, "feats")
    m, c = f.shape
    if m < 1 or not 1 <= c <= MAX_POOL_CHANNELS:
        raise ValueError(f"feats {tuple(f.shape)}: needs m >= 1 and C in 1..{MAX_POOL_CHANNELS}")
    if not isinstance(inds, torch.Tensor) or inds.dim() != 2:
        raise ValueError("inds must be a (n, k) index tensor")
    idx = _indices(inds, "inds", inds.shape[0], f.device)
    n = idx.shape[0]
    out = torch.empty((n, c), dtype=torch.float32, device=f.device)
    if n == 0:
        return out
    with torch.cuda.device(f.device):
        _lib.call("pcr_neighbor_max", _lib.ptr(f), _lib.ptr(idx), idx.element_size(), n, m, idx.shape[1], c,
                  _lib.ptr(out), _lib.stream_handle(f.device))
    return out


class KPConv(torch.nn.Module):
    """The reference's KPConv (blocks.py:44-132) on the fused op, with its
    attribute names and state-dict keys (`weights`, `kernel_points`).  Built from
    given kernel points (K,3); it reads no kernel-point files.  `weights` may be
    an existing Parameter to share (fuse()), else it is initialised as there."""

    def __init__(self, in_channels, out_channels, radius, kernel_points, KP_extent, KP_influence="linear",
                 aggregation_mode="sum", weights=None):
        super().__init__()
        if aggregation_mode != "sum":
            raise NotImplementedError(f"aggregation_mode={aggregation_mode!r}: only 'sum' is built")
        if KP_influence not in _INFLUENCE:
            raise NotImplementedError(f"KP_influence={KP_influence!r}: 'linear' or 'constant'")
        if isinstance(kernel_points, torch.nn.Parameter):
            kp = kernel_points
        else:
            kp = torch.nn.Parameter(torch.as_tensor(kernel_points, dtype=torch.float32).clone(),
                                    requires_grad=False)
        if kp.dim() != 2 or kp.shape[1] != 3:
            raise ValueError(f"kernel_points must be (K, 3), got {tuple(kp.shape)}")
        self.in_channels, self.out_channels = int(in_channels), int(out_channels)
        self.radius = radius
        self.K = kp.shape[0]
        self.KP_extent = KP_extent
        self.KP_influence = KP_influence
        self.aggregation_mode = aggregation_mode
        if weights is None:
            weights = torch.nn.Parameter(torch.zeros((self.K, self.in_channels, self.out_channels),
                                                     dtype=torch.float32))
            torch.nn.init.kaiming_uniform_(weights, a=5 ** 0.5)
        if tuple(weights.shape) != (self.K, self.in_channels, self.out_channels):
            raise ValueError(f"weights {tuple(weights.shape)} must be (K, in_channels, out_channels) = "
                             f"{(self.K, self.in_channels, self.out_channels)}")
        self.weights = weights
        self.kernel_points = kp

    def forward(self, q_pts, s_pts, s_feats, neigh_inds):
        return kpconv_forward(q_pts, s_pts, s_feats, neigh_inds, self.kernel_points, self.weights,
                              self.KP_extent, self.KP_influence)

    def __repr__(self):
        return "KPConv(radius: {:.2f}, nkernels: {:d}, in_feat: {:d}, out_feat: {:d})".format(
            self.radius, self.K, self.in_channels, self.out_channels)


class MaxPool(torch.nn.Module):
    """MaxPoolBlock (blocks.py:177-188) on neighbor_max."""

    def __init__(self, layer_ind):
        super().__init__()
        self.layer_ind = layer_ind

    def forward(self, feats, batch):
        return neighbor_max(feats, batch["pools"][self.layer_ind])


def _conv_shaped(mod):
    w, kp = getattr(mod, "weights", None), getattr(mod, "kernel_points", None)
    return (isinstance(w, torch.Tensor) and w.dim() == 3 and isinstance(kp, torch.Tensor) and kp.dim() == 2
            and kp.shape[1] == 3 and kp.shape[0] == w.shape[0] and hasattr(mod, "KP_extent")
            and getattr(mod, "aggregation_mode", None) == "sum" and not isinstance(mod, KPConv))


def fuse(model):
    """Swap the torch composites of a loaded network for the fused ops, in place:
    every submodule with `weights` (K,C_in,C_out), `kernel_points` (K,3),
    `KP_extent` and aggregation_mode 'sum' becomes a KPConv sharing the same
    parameters, every MaxPoolBlock (by class name, with `layer_ind`) a MaxPool.
    Returns (convolutions swapped, pools swapped)."""
    kinds = ((_conv_shaped, lambda c: KPConv(c.weights.shape[1], c.weights.shape[2], getattr(c, "radius", 0.0),
                                             c.kernel_points, c.KP_extent, getattr(c, "KP_influence", "linear"), "sum",
                                             weights=c.weights)),
             (("MaxPoolBlock", ("layer_ind",)), lambda c: MaxPool(c.layer_ind)))
    return _front.swap_children(model, kinds, errors=())
