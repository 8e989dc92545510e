"""Seeded inputs of the KPConv forward / neighbour max-pool tests.  Only the
reference's outputs are stored (kpconv_conv_golden.npz); the inputs are rebuilt
from these generators by make_golden_kpconv_conv.py and by the tests.

A case is (n, m, k, K, C_in, C_out) and a search radius.  Supports and queries
are uniform in the unit cube; a query's columns are its k nearest supports by
ascending distance, those within the radius as indices and the rest as pads
(m, the reference's pad value).  The last query sits far outside the cube, so
every case has an all-pad query.  Features are abs(normal) in the even cases
and signed in the odd ones (rows with negative sums exist there); one row in
eight is exactly zero.  Every row sum is either exactly 0 or at least
1e-3 sum|f| away from it, so the counted-neighbour rule cannot flip between
an f32 and an f64 sum: if a seed breaks that, change the seed.
"""
import numpy as np

SEED = 20240917

# name -> ((n, m, k, K, C_in, C_out), radius)
CASES = {
    "first": ((129, 65, 37, 15, 1, 64), 0.55),      # first layer; k % 4 != 0; one query past a tile
    "c32": ((300, 257, 20, 15, 32, 32), 0.25),      # the common 32 -> 32 layer
    "deep": ((33, 33, 5, 15, 256, 256), 0.40),      # the deepest layer; the channel-chunk loop
    "pads": ((70, 40, 40, 15, 128, 128), 0.29),     # about 90 % pads
    "ragged": ((64, 300, 38, 7, 24, 40), 0.35),     # ragged channels; K = 7; n < m, as in a pool
    "m1": ((33, 1, 3, 16, 8, 8), 0.80),             # m = 1; K = 16
}
CONSTANT_CASE = "ragged"          # the case also stored with KP_influence = 'constant'
POOL_CASES = ("c32", "ragged")    # the cases whose MaxPoolBlock output is stored


def make(name):
    """-> dict(q, s, f, idx (int64), kp, W, extent)."""
    (n, m, k, K, c_in, c_out), radius = CASES[name]
    order = sorted(CASES).index(name)
    rng = np.random.default_rng((SEED, order))
    s = rng.random((m, 3)).astype(np.float32)
    q = rng.random((n, 3)).astype(np.float32)
    q[-1] = 50.0
    d2 = ((q[:, None, :].astype(np.float64) - s[None].astype(np.float64)) ** 2).sum(-1)
    near = np.argsort(d2, axis=1, kind="stable")
    dn = np.take_along_axis(d2, near, 1)
    if k > m:   # more columns than supports: the rest can only be pads
        near = np.concatenate([near, np.zeros((n, k - m), np.int64)], 1)
        dn = np.concatenate([dn, np.full((n, k - m), np.inf)], 1)
    idx = np.where(dn[:, :k] <= radius * radius, near[:, :k], m).astype(np.int64)
    assert (idx[-1] == m).all() and (idx != m).any()
    signed = order % 2 == 1
    f = rng.standard_normal((m, c_in)).astype(np.float32)
    if not signed:
        f = np.abs(f)
    f[rng.random(m) < 0.125] = 0.0
    if m >= 8:
        f[m // 2] = 0.0
    rs = f.astype(np.float64).sum(1)
    ab = np.abs(f).astype(np.float64).sum(1)
    assert ((ab == 0) | (np.abs(rs) >= 1e-3 * ab)).all(), f"{name}: a row sum is too close to 0, change SEED"
    kp = rng.standard_normal((K, 3))
    kp = (kp / np.linalg.norm(kp, axis=1, keepdims=True) * rng.random((K, 1)) ** (1 / 3) * 0.66 * radius)
    kp[0] = 0.0
    W = (rng.standard_normal((K, c_in, c_out)) / np.sqrt(K * c_in)).astype(np.float32)
    return dict(q=q, s=s, f=f, idx=idx, kp=kp.astype(np.float32), W=W, extent=float(np.float32(0.5 * radius)))
