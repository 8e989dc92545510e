"""numpy restatement of the grouping contract (include/pcr_api.h: pcr_fps,
pcr_ball_query, pcr_group_ppf), direct-form distances, every f32 operation
rounded on its own.  The CPU tests pin it to the reference's outputs in
tests/golden/grouping_golden.npz; the GPU tests then stand on it where the
fixture has no case (8192 / 8193 points)."""
import numpy as np

F = np.float32


def sqdist(a, b):
    """(dx*dx + dy*dy) + dz*dz in f32 for broadcastable (..., 3) arrays."""
    a = np.asarray(a, F)
    b = np.asarray(b, F)
    dx = a[..., 0] - b[..., 0]
    dy = a[..., 1] - b[..., 1]
    dz = a[..., 2] - b[..., 2]
    return (dx * dx + dy * dy) + dz * dz


def radius2(radius):
    """The f32 threshold: the product in double, then rounded once."""
    return F(float(radius) * float(radius))


def fps(xyz, start, m):
    """xyz (b,n,3) f32, start (b) -> (b,m) int64."""
    xyz = np.asarray(xyz, F)
    b, n, _ = xyz.shape
    out = np.zeros((b, m), np.int64)
    for c in range(b):
        dist = np.full(n, F(1e10), F)
        cur = int(start[c])
        for i in range(m):
            out[c, i] = cur
            d = sqdist(xyz[c, cur], xyz[c])
            closer = d < dist
            dist[closer] = d[closer]
            cur = int(np.argmax(dist))   # first index of the maximum
    return out


def ball_query(xyz, query, radius, k):
    """-> idx (b,q,k) int64, count (b,q) int64.  Neighbour iff not d2 > r2;
    ascending indices cut to k, later columns repeat the first neighbour, a row
    without neighbours holds n."""
    xyz = np.asarray(xyz, F)
    query = np.asarray(query, F)
    b, n, _ = xyz.shape
    q = query.shape[1]
    r2 = radius2(radius)
    idx = np.empty((b, q, k), np.int64)
    count = np.empty((b, q), np.int64)
    for c in range(b):
        inside = ~(sqdist(query[c][:, None, :], xyz[c][None, :, :]) > r2)   # (q,n)
        count[c] = inside.sum(1)
        rank = np.cumsum(inside, axis=1) - 1          # position of a neighbour in its row
        first = np.where(count[c] > 0, np.argmax(inside, axis=1), n)
        rows = np.repeat(first[:, None], k, axis=1)
        qi, j = np.nonzero(inside & (rank < k))
        rows[qi, rank[qi, j]] = j
        idx[c] = rows
    return idx, count


def _angle(a, c, dt):
    """atan2(|a x c|, a . c) evaluated in dtype dt; the dot's sum starts from +0."""
    a = a.astype(dt)
    c = c.astype(dt)
    c0 = a[..., 1] * c[..., 2] - a[..., 2] * c[..., 1]
    c1 = a[..., 2] * c[..., 0] - a[..., 0] * c[..., 2]
    c2 = a[..., 0] * c[..., 1] - a[..., 1] * c[..., 0]
    cn = np.sqrt((c0 * c0 + c1 * c1) + c2 * c2)
    dot = ((dt(0) + a[..., 0] * c[..., 0]) + a[..., 1] * c[..., 1]) + a[..., 2] * c[..., 2]
    return np.arctan2(cn, dot)


def group_ppf(xyz, normals, idx, dt=F):
    """Features (b,n,k,C) of the group idx (b,n,k): C = 10 with normals, else 6.
    Channels 0-5 (x_i and g = x_j - x_i) are always f32; channels 6-9 are
    evaluated in `dt` on the f32 normals and the f32 g (dt = float64 gives the
    value the f32 results are measured against).  Returned as float64 when dt is
    float64 so that nothing is rounded again."""
    xyz = np.asarray(xyz, F)
    b, n, _ = xyz.shape
    k = idx.shape[2]
    bi = np.arange(b)[:, None, None]
    xi = np.broadcast_to(xyz[:, :, None, :], (b, n, k, 3))
    g = xyz[bi, idx] - xi                              # f32
    parts = [xi, g]
    if normals is not None:
        normals = np.asarray(normals, F)
        ni = np.broadcast_to(normals[:, :, None, :], (b, n, k, 3))
        nj = normals[bi, idx]
        gd = g.astype(dt)
        norm = np.sqrt((gd[..., 0] * gd[..., 0] + gd[..., 1] * gd[..., 1]) + gd[..., 2] * gd[..., 2])
        ppf = np.stack([_angle(ni, g, dt), _angle(nj, g, dt), _angle(ni, nj, dt), norm], axis=-1)
        parts.append(ppf)
    out_dt = np.float64 if dt is np.float64 else F
    return np.concatenate([p.astype(out_dt) for p in parts], axis=-1)
