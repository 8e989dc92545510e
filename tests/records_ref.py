"""numpy restatements for the transform and record kernels of csrc/procrustes.hip.

`chamfer_mean` is pipeline_records_kernel's real summation order:
  * 1024 partial sums in f64, partial t over the indices t, t + 1024, ... in
    increasing order (the kernel's 8-wide runs add in index order; an index
    past the end adds +0.0, which changes nothing);
  * per wave of 64 partials the xor butterfly, which in lane 0 is the halving
    tree p[l] += p[l + h], h = 32 ... 1 (a + b == b + a bit for bit);
  * the 16 wave totals added in order, starting from 0.0;
  * sum1 / N + sum2 / M.
`sum256` is the 256-lane order of the Procrustes / ICP sums (oracle det_sum),
kept to show that an input tells the two orders apart.

`distances(N, M)` builds the (P, N), (P, M) f32 test distances: non-negative,
full mantissas, magnitudes over 2^-40 ... 2^20, from seeds searched once so that
the 1024-lane order is told apart from the other two (SEEDS, below).
"""
import math

import numpy as np

P = 3
SHAPES = ((1, 1), (63, 65), (1023, 1025), (1024, 1024), (8191, 9000), (8193, 64))


def transform_f32(x, T):
    """transform_kernel restated: x (B,N,3) f32, T (B,4,4) or (B,3,4) f64 ->
    ((T_a0 x + T_a1 y) + T_a2 z) + T_a3 with every step rounded in f64, then
    rounded to f32; rows of T past the third are not read."""
    x = np.asarray(x, np.float32)
    T = np.asarray(T, np.float64)
    X = x.astype(np.float64)
    R, t = T[:, :3, :3], T[:, :3, 3]
    out = np.empty_like(x)
    for a in range(3):
        out[..., a] = ((((R[:, a, 0, None] * X[..., 0]) + R[:, a, 1, None] * X[..., 1])
                        + R[:, a, 2, None] * X[..., 2]) + t[:, a, None]).astype(np.float32)
    return out


def _rows(d):
    d = np.asarray(d, np.float32)
    return d.reshape(1, -1) if d.ndim == 1 else d


def sum1024(d):
    """(P, n) or (n,) f32 -> (P,) f64 sums in the record kernel's order."""
    d = _rows(d)
    pad = np.zeros((d.shape[0], -d.shape[1] % 1024), np.float32)
    rows = np.concatenate([d, pad], axis=1).astype(np.float64).reshape(d.shape[0], -1, 1024)
    acc = np.zeros((d.shape[0], 1024))
    for k in range(rows.shape[1]):
        acc = acc + rows[:, k]
    acc = acc.reshape(d.shape[0], 16, 64)
    h = 32
    while h:
        acc[:, :, :h] = acc[:, :, :h] + acc[:, :, h:2 * h]
        h //= 2
    tot = np.zeros(d.shape[0])
    for w in range(16):
        tot = tot + acc[:, w, 0]
    return tot


def sum256(d):
    """The 256-lane order: lane l over i = l, l + 256, ..., then a halving tree."""
    d = _rows(d)
    pad = np.zeros((d.shape[0], -d.shape[1] % 256), np.float32)
    rows = np.concatenate([d, pad], axis=1).astype(np.float64).reshape(d.shape[0], -1, 256)
    acc = np.zeros((d.shape[0], 256))
    for k in range(rows.shape[1]):
        acc = acc + rows[:, k]
    h = 128
    while h:
        acc[:, :h] = acc[:, :h] + acc[:, h:2 * h]
        h //= 2
    return acc[:, 0].copy()


def sum_np(d):
    d = _rows(d)
    return np.array([np.sum(r.astype(np.float64)) for r in d])


def _mean(sum_fn, d1, d2):
    d1, d2 = _rows(d1), _rows(d2)
    return sum_fn(d1) / float(d1.shape[1]) + sum_fn(d2) / float(d2.shape[1])


def chamfer_mean(d1, d2):
    """Slot 36 of the records: (P,N), (P,M) f32 -> (P,) f64, bit for bit."""
    return _mean(sum1024, d1, d2)


def chamfer_mean_256(d1, d2):
    return _mean(sum256, d1, d2)


def chamfer_mean_np(d1, d2):
    return _mean(sum_np, d1, d2)


def chamfer_mean_fsum(d1, d2):
    """Correctly rounded sums (math.fsum), then / N + / M in f64."""
    d1, d2 = _rows(d1), _rows(d2)
    return np.array([math.fsum(a.astype(np.float64).tolist()) / a.shape[0]
                     + math.fsum(b.astype(np.float64).tolist()) / b.shape[0] for a, b in zip(d1, d2)])


def wide(rng, shape):
    """Non-negative f32 with full random mantissas, exponents uniform over
    2^-40 ... 2^20."""
    m = (1.0 + rng.random(shape)).astype(np.float32)
    e = rng.integers(-40, 20, shape)
    return np.ldexp(m, e).astype(np.float32)


# seed per shape: the first seed (counting from 0) at which `discriminates`
# holds for the shape, found by search_seeds() (`python tests/records_ref.py`)
SEEDS = {(1, 1): 0, (63, 65): 0, (1023, 1025): 0, (1024, 1024): 1, (8191, 9000): 0, (8193, 64): 0}


def distances(N, M, seed=None):
    rng = np.random.default_rng([N, M, SEEDS[(N, M)] if seed is None else seed])
    return wide(rng, (P, N)), wide(rng, (P, M))


def _bits_differ(a, b):
    return np.asarray(a, np.float64).view(np.uint64) != np.asarray(b, np.float64).view(np.uint64)


def discriminates(d1, d2):
    """The inputs tell the 1024-lane order apart: for every side with >= 1024
    entries some item's 1024-order SUM differs in bits from both its 256-lane
    sum and np.sum; and some item's slot-36 VALUE in the 1024-lane order
    differs from the value either other order gives (so the difference
    survives / N + / M).  Sides below 1024 entries cannot discriminate (one
    term per partial) and ask nothing."""
    ok = True
    for d in (d1, d2):
        if _rows(d).shape[1] >= 1024:
            s = sum1024(d)
            ok = ok and bool(np.any(_bits_differ(s, sum256(d)) & _bits_differ(s, sum_np(d))))
    if max(_rows(d1).shape[1], _rows(d2).shape[1]) >= 1024:
        c = chamfer_mean(d1, d2)
        ok = ok and bool(np.any(_bits_differ(c, chamfer_mean_256(d1, d2))
                                & _bits_differ(c, chamfer_mean_np(d1, d2))))
    return ok


def search_seeds(limit=200):
    out = {}
    for (N, M) in SHAPES:
        for seed in range(limit):
            if discriminates(*distances(N, M, seed)):
                out[(N, M)] = seed
                break
    return out


if __name__ == "__main__":
    print(search_seeds())
