"""numpy restatement of the k-NN graph contract (include/pcr_api.h:
pcr_knn_graph, pcr_edge_features): direct-form distances, every point of the
cloud ranked by the pair (d2, index), rank 0 dropped.  The CPU tests pin it to
what the reference's get_graph_features returned (tests/golden/knn_golden.npz);
the GPU tests then stand on it."""
import numpy as np

from grouping_ref import F, sqdist

ROWS = 512   # rows of the (n,n) key matrix formed at a time


def ranked(xyz, k):
    """Ranks 0 .. kk of every row, kk = min(k, n - 1): idx (b,n,kk+1) int64 and
    d2 (b,n,kk+1) f32.  The key (d2 bits << 32) | j is what orders them:
    distances are >= +0, so their bits order like the values."""
    xyz = np.asarray(xyz, F)
    b, n, _ = xyz.shape
    kk = min(int(k), n - 1)
    idx = np.empty((b, n, kk + 1), np.int64)
    d2 = np.empty((b, n, kk + 1), F)
    j = np.arange(n, dtype=np.uint64)
    for c in range(b):
        for r0 in range(0, n, ROWS):
            d = sqdist(xyz[c, r0:r0 + ROWS, None, :], xyz[c][None, :, :])
            key = (d.view(np.uint32).astype(np.uint64) << np.uint64(32)) | j
            if kk + 1 < n:
                key = np.partition(key, kk, axis=1)[:, :kk + 1]
            key = np.sort(key, axis=1)
            idx[c, r0:r0 + ROWS] = (key & np.uint64(0xFFFFFFFF)).astype(np.int64)
            d2[c, r0:r0 + ROWS] = (key >> np.uint64(32)).astype(np.uint32).view(F)
    return idx, d2


def knn_graph(xyz, k):
    """-> idx (b,n,kk) int64, d2 (b,n,kk) f32: ranks 1 .. kk."""
    idx, d2 = ranked(xyz, k)
    return np.ascontiguousarray(idx[..., 1:]), np.ascontiguousarray(d2[..., 1:])


def edge_features(feats, idx, channels_first=False):
    """(b,n,kk,2c): [f_i, f_j - f_i]; channels_first: the same as (b,2c,n,kk)."""
    feats = np.asarray(feats, F)
    b, n, c = feats.shape
    kk = idx.shape[2]
    fi = np.broadcast_to(feats[:, :, None, :], (b, n, kk, c))
    fj = feats[np.arange(b)[:, None, None], idx]
    out = np.concatenate([fi, fj - fi], axis=-1).astype(F)
    if channels_first:
        out = np.transpose(out, (0, 3, 1, 2))
    return np.ascontiguousarray(out)
