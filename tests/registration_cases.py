"""Inputs that drive the RANSAC and ICP loops (csrc/ransac.hip, csrc/icp.hip) through
the branches well-behaved synthetic pairs never reach: equal-fitness updates, full
ties, no inliers, no validated hypothesis, a bound that collapses to 0 or to -inf,
max_iteration on the round and chunk edges, tiny and ragged shapes, and ICP with
nothing (or next to nothing) to estimate from.  Shared by
test_registration_cases_cpu.py (which proves on the oracle alone that each case still
reaches the branch it is named for) and test_ransac_edges_gpu.py /
test_icp_edges_gpu.py (which hold the kernels to the oracle bit for bit).

Every case is a deterministic function of fixed seeds.  Oracle results are cached
here, so both files and every test in them share one oracle run per input."""
import functools
from typing import NamedTuple

import numpy as np

# --------------------------------------------------------------------------
# RANSAC
# --------------------------------------------------------------------------


class RCase(NamedTuple):
    src: np.ndarray      # (n, 3) f32
    tgt: np.ndarray      # (m, 3) f32
    corr: np.ndarray     # (K, 2) i32
    prm: dict            # d, ransac_n, edge, dcheck, max_iteration, confidence, seed, pair_id


OFF = -1.0   # a checker switched off


def _prm(d=0.05, ransac_n=3, edge=0.9, dcheck=None, max_iteration=200, confidence=0.999, seed=0,
         pair_id=0):
    return dict(d=d, ransac_n=ransac_n, edge=edge, dcheck=d if dcheck is None else dcheck,
                max_iteration=max_iteration, confidence=confidence, seed=seed, pair_id=pair_id)


def _f32(a):
    return np.ascontiguousarray(a, np.float32)


def lattice():
    """The 8 x 8 x 8 lattice arange(8) / 8 (exact in f32), 512 points."""
    g = np.arange(8) / 8.0
    return _f32(np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3))


RZ90 = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
SHIFT = np.array([0.5, -0.25, 1.0])


def _outlier_corr(rng, n, m, frac):
    """The identity correspondences of min(n, m) points with `frac` of them sent to
    random targets."""
    k = min(n, m)
    co = np.stack([np.arange(k), np.arange(k)], 1).astype(np.int32)
    bad = rng.random(k) < frac
    co[bad, 1] = rng.integers(0, m, int(bad.sum()))
    return co


TIE_SEED = 5


def _tie(noise):
    rng = np.random.default_rng(TIE_SEED)
    src = lattice()
    co = _outlier_corr(rng, 512, 512, 0.4)
    tgt = src.astype(np.float64) @ RZ90.T + SHIFT
    if noise:
        tgt = tgt + rng.normal(0.0, noise, tgt.shape)
    return RCase(src, _f32(tgt), co, _prm(confidence=1.0, max_iteration=200, seed=TIE_SEED))


def tie_rmse():
    """Lattice -> lattice turned 90 degrees about z and shifted, N(0, 1e-3) noise, 40 %
    wrong correspondences, d = 0.05 < half the lattice step, confidence 1: every good
    hypothesis has fitness exactly 1.0, so the best moves on rmse alone."""
    return _tie(1e-3)


def tie_full():
    """tie_rmse without noise: every good hypothesis has fitness 1.0 AND rmse 0.0 (its
    error sum is below one fixed-point unit), so the first must stay the best."""
    return _tie(0.0)


def perfect():
    """The noisy lattice pair with every correspondence true: w = 1, est_k = 0."""
    c = _tie(1e-3)
    co = np.stack([np.arange(512), np.arange(512)], 1).astype(np.int32)
    return RCase(c.src, c.tgt, co, _prm(confidence=0.999, max_iteration=1000, seed=1))


def no_inliers():
    """300 points of [0,1]^3 against unrelated targets 100 away, a random permutation
    as correspondences, both checkers off, d = 1e-3: every hypothesis is validated and
    none has an inlier."""
    rng = np.random.default_rng(0)
    src = rng.random((300, 3))
    tgt = rng.random((300, 3)) * 10.0 + 100.0
    co = np.stack([np.arange(300), rng.permutation(300)], 1).astype(np.int32)
    return RCase(_f32(src), _f32(tgt), co,
                 _prm(d=1e-3, edge=OFF, dcheck=OFF, max_iteration=300, seed=2))


def none_pass():
    """The lattice against 512 copies of one target point, checkers on: a triangle
    cannot keep its edge lengths, so no hypothesis passes."""
    src = lattice()
    tgt = np.tile(np.array([[0.5, 0.5, 0.5]]), (512, 1))
    co = np.stack([np.arange(512), np.arange(512)], 1).astype(np.int32)
    return RCase(src, _f32(tgt), co, _prm(max_iteration=300, seed=3))


MINUS_INF_SEED = 0


def minus_inf_bound(ransac_n=8):
    """ransac_n = 8, K = 1000 correspondences of which 10 are true, checkers off: an
    accepted hypothesis has w = cin / K of about 0.01 or less, 1 - w^8 rounds to 1.0,
    det_log gives 0 and the bound is log(1 - conf) / 0 = -inf."""
    rng = np.random.default_rng(MINUS_INF_SEED)
    src = rng.random((512, 3))
    tgt = src @ RZ90.T + SHIFT
    co = np.stack([rng.integers(0, 512, 1000), rng.integers(0, 512, 1000)], 1).astype(np.int32)
    true = rng.choice(1000, 10, replace=False)
    co[true, 1] = co[true, 0]
    return RCase(_f32(src), _f32(tgt), co,
                 _prm(ransac_n=ransac_n, edge=OFF, dcheck=OFF, max_iteration=3000, seed=4))


def _small_pair(rng, n, m=None, noise=1e-3):
    m = n if m is None else m
    src = rng.random((n, 3))
    tgt = src[np.arange(m) % n] @ RZ90.T + SHIFT + rng.normal(0.0, noise, (m, 3))
    return _f32(src), _f32(tgt)


def shape_case(name):
    """The tiny and ragged shapes: n = m = K = 3; K == ransac_n == 8; n = 1; m = 1;
    n in {31, 33, 63, 65, 257} (mask words, 64-query chunks, split sweeps with fewer
    chunks than parts)."""
    rng = np.random.default_rng(hash_name(name))
    if name == "n3_m3_k3":
        s, t = _small_pair(rng, 3)
        co = np.stack([np.arange(3), np.arange(3)], 1).astype(np.int32)
        return RCase(s, t, co, _prm(max_iteration=64, seed=6))
    if name == "k8_rn8":
        s, t = _small_pair(rng, 65)
        i = rng.choice(65, 8, replace=False)
        co = np.stack([i, i], 1).astype(np.int32)
        return RCase(s, t, co, _prm(ransac_n=8, max_iteration=64, seed=7))
    if name == "n1":
        s, t = _small_pair(rng, 1, 5)
        co = np.zeros((3, 2), np.int32)
        return RCase(s, t, co, _prm(edge=OFF, dcheck=OFF, max_iteration=64, seed=8))
    if name == "m1":
        s, t = _small_pair(rng, 33, 1)
        co = np.stack([np.arange(33), np.zeros(33)], 1).astype(np.int32)
        return RCase(s, t, co, _prm(edge=OFF, dcheck=OFF, max_iteration=64, seed=9))
    n = int(name[1:])
    s, t = _small_pair(rng, n)
    return RCase(s, t, _outlier_corr(rng, n, n, 0.3), _prm(max_iteration=200, seed=10 + n))


def hash_name(name):
    """A seed from a name, stable across runs (hash() of a str is salted)."""
    return sum((i + 1) * ord(ch) for i, ch in enumerate(name))


SHAPES = ("n3_m3_k3", "k8_rn8", "n1", "m1", "n31", "n33", "n63", "n65", "n257")

RANSAC_CASES = {"tie_rmse": tie_rmse, "tie_full": tie_full, "perfect": perfect,
                "no_inliers": no_inliers, "none_pass": none_pass,
                "minus_inf_bound": minus_inf_bound}
RANSAC_CASES.update({s: functools.partial(shape_case, s) for s in SHAPES})

# max_iteration on and next to the edges: one hypothesis, a ballot word (64), a
# hypothesis block (256), the first round (1024), the first block and word of the
# second round, and the end of the host loop's first 4096-hypothesis round
ROUND_EDGES = (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 1024 + 256, 1024 + 257,
               5119, 5120, 5121)


@functools.lru_cache(maxsize=None)
def rcase(name):
    c = RANSAC_CASES[name]()
    for a in (c.src, c.tgt, c.corr):
        a.setflags(write=False)
    return c


_memo = {}


def _freeze(r):
    for v in r.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return r


def run_ransac(oracle, c, **over):
    """oracle.ransac of a case with some parameters replaced (not cached)."""
    p = dict(c.prm, **over)
    return oracle.ransac(c.src, c.tgt, c.corr, p["d"], ransac_n=p["ransac_n"], edge_ratio=p["edge"],
                         dist_check=p["dcheck"], max_iteration=p["max_iteration"],
                         confidence=p["confidence"], seed=p["seed"], pair_id=p["pair_id"])


def oracle_ransac(oracle, name, **over):
    """The oracle's result of a named case, once per (name, overrides), read-only."""
    key = ("ransac", name, tuple(sorted(over.items())))
    if key not in _memo:
        _memo[key] = _freeze(run_ransac(oracle, rcase(name), **over))
    return _memo[key]


def tie_trajectory(oracle, name, upto=200):
    """(best_itr, fitness, rmse, validated) after max_iteration = 1..upto: the loop
    under confidence 1 never stops early, so this is the history of one run."""
    return [(r["best_itr"], r["fitness"], r["inlier_rmse"], r["validated"])
            for r in (oracle_ransac(oracle, name, max_iteration=k) for k in range(1, upto + 1))]


def tie_updates(oracle, name, upto=200):
    """Iterations at which the best changed, with (fitness, rmse) before and after."""
    out, prev = [], (-1, 0.0, 0.0, 0)
    for t in tie_trajectory(oracle, name, upto):
        if t[0] != prev[0]:
            out.append((t[0], prev[1:3], t[1:3]))
        prev = t
    return out


def round_edge_iterations(oracle):
    """ROUND_EDGES plus {u, u + 1} for every update u of tie_rmse: the winner is the
    last hypothesis of a run, or the first one outside it."""
    ks = set(ROUND_EDGES)
    for u, _, _ in tie_updates(oracle, "tie_rmse"):
        ks.update((u, u + 1))
    return tuple(sorted(k for k in ks if k >= 1))


def corr_inliers(c, T):
    """cin of a transform: correspondences with |T s - t|^2 < d * d, in the kernels'
    order of operations."""
    S = c.src.astype(np.float64)[c.corr[:, 0]]
    G = c.tgt.astype(np.float64)[c.corr[:, 1]]
    q = [((T[r, 0] * S[:, 0] + T[r, 1] * S[:, 1]) + T[r, 2] * S[:, 2]) + T[r, 3] for r in range(3)]
    dx, dy, dz = G[:, 0] - q[0], G[:, 1] - q[1], G[:, 2] - q[2]
    return int((((dx * dx + dy * dy) + dz * dz) < c.prm["d"] * c.prm["d"]).sum())


def dense_grid_fits(tgt, d):
    """Whether the r-cell tables of csrc/grid_dense.h can hold this target cloud: at
    most 72 * 1024 cells of width 1.005 d in its bounding box (the table bytes of
    clouds this small fit whenever the cells do).  Where they cannot,
    PCR_RANSAC_GRID=dense is an error by design and the tests run auto instead."""
    if len(tgt) == 0:
        return True
    c = np.floor(np.asarray(tgt, np.float64) / (1.005 * d))
    return float(np.prod(c.max(0) - c.min(0) + 1.0)) <= 72 * 1024


# ---- the mixed batch: every kind under one parameter set --------------------

BATCH_P = 257
BATCH_PRM = _prm(d=0.05, ransac_n=3, edge=0.9, dcheck=10.0, max_iteration=300, confidence=1.0,
                 seed=21)
BATCH_KINDS = ("tie_rmse", "tie_full", "perfect", "no_inliers", "none_pass", "n1", "m1", "n3",
               "n31", "n33", "n63", "n65", "n257", "k2_invalid", "n0_invalid")


def _scaled_pair(rng):
    """64 points of [0, 100]^3 against themselves shrunk by 0.92: a sampled triangle
    keeps its edge ratios above 0.9 and passes the (loose) distance check, but the
    rigid fit leaves each corner 0.08 of its distance to the triangle's centroid --
    many d -- from its target, and no other point near one except by chance.  (Three
    draws of one correspondence do align it: a pair of this kind can find a result.)"""
    src = rng.random((64, 3)) * 100.0
    tgt = 0.92 * src @ RZ90.T + SHIFT
    return _f32(src), _f32(tgt)


def batch_pair(p):
    """Pair p of the mixed batch: (kind, src, tgt, corr)."""
    kind = BATCH_KINDS[p % len(BATCH_KINDS)]
    rng = np.random.default_rng(1000 + p)
    ident = lambda k: np.stack([np.arange(k), np.arange(k)], 1).astype(np.int32)  # noqa: E731
    if kind in ("tie_rmse", "tie_full"):
        src = lattice()
        tgt = src.astype(np.float64) @ RZ90.T + SHIFT
        if kind == "tie_rmse":
            tgt = tgt + rng.normal(0.0, 1e-3, tgt.shape)
        return kind, src, _f32(tgt), _outlier_corr(rng, 512, 512, 0.4)
    if kind == "perfect":
        s, t = _small_pair(rng, 65)
        return kind, s, t, ident(65)
    if kind == "no_inliers":
        s, t = _scaled_pair(rng)
        return kind, s, t, ident(64)
    if kind == "none_pass":
        s, _ = _small_pair(rng, 40)
        return kind, s, _f32(np.tile([[0.5, 0.5, 0.5]], (40, 1))), ident(40)
    if kind == "n1":
        s, t = _small_pair(rng, 1, 5)
        return kind, s, t, np.zeros((3, 2), np.int32)
    if kind == "m1":
        s, t = _small_pair(rng, 33, 1)
        return kind, s, t, np.stack([np.arange(33), np.zeros(33)], 1).astype(np.int32)
    if kind == "k2_invalid":
        s, t = _small_pair(rng, 31)
        return kind, s, t, ident(2)
    if kind == "n0_invalid":
        s, t = _small_pair(rng, 31)
        return kind, s[:0], t, ident(31)
    n = int(kind[1:])
    s, t = _small_pair(rng, n)
    return kind, s, t, (ident(3) if n == 3 else _outlier_corr(rng, n, n, 0.3))


@functools.lru_cache(maxsize=None)
def batch():
    """The padded mixed batch: dict(kinds, src (P,Nmax,3), tgt, corr (P,Kmax,2), n_src,
    n_tgt, n_corres, pair_ids).  Padding rows hold points that would change a pair's
    result if a kernel looked at them (sources inside the target cloud, targets on
    source points) and correspondences between them."""
    pairs = [batch_pair(p) for p in range(BATCH_P)]
    N = max(len(s) for _, s, _, _ in pairs)
    M = max(len(t) for _, _, t, _ in pairs)
    K = max(len(c) for _, _, _, c in pairs)
    src = np.zeros((BATCH_P, N, 3), np.float32)
    tgt = np.zeros((BATCH_P, M, 3), np.float32)
    corr = np.zeros((BATCH_P, K, 2), np.int32)
    for p, (_, s, t, c) in enumerate(pairs):
        src[p] = t[0]
        src[p, :len(s)] = s
        tgt[p] = s[0] if len(s) else 0.0
        tgt[p, :len(t)] = t
        corr[p, :, 0] = N - 1
        corr[p, :, 1] = M - 1
        corr[p, :len(c)] = c
    out = dict(kinds=[k for k, _, _, _ in pairs], pairs=pairs, src=src, tgt=tgt, corr=corr,
               n_src=np.array([len(s) for _, s, _, _ in pairs], np.int32),
               n_tgt=np.array([len(t) for _, _, t, _ in pairs], np.int32),
               n_corres=np.array([len(c) for _, _, _, c in pairs], np.int32),
               pair_ids=(np.arange(BATCH_P, dtype=np.int32) * 3 + 11))
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def oracle_batch(oracle):
    """oracle.ransac of every pair of the mixed batch (one run per session)."""
    if "batch" not in _memo:
        b, q = batch(), BATCH_PRM
        _memo["batch"] = [_freeze(run_ransac(oracle, RCase(s, t, c, q), pair_id=int(b["pair_ids"][p])))
                          for p, (_, s, t, c) in enumerate(b["pairs"])]
    return _memo["batch"]


# --------------------------------------------------------------------------
# ICP
# --------------------------------------------------------------------------

ICP_D = 0.25           # float(d * d) == d * d == 0.0625 exactly
ICP_ITERS = (0, 1, 30)


class ICase(NamedTuple):
    src: np.ndarray    # (n, 3) f32
    tgt: np.ndarray    # (m, 3) f32
    init: np.ndarray   # (4, 4) f64
    d: float


def _rigid(rx, ry, rz, t):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    T = np.eye(4)
    T[:3, :3] = Rz @ Ry @ Rx
    T[:3, 3] = t
    return T


NON_IDENTITY = _rigid(0.3, -0.2, 0.5, [0.125, -0.5, 0.25])


def float_radius():
    """(r, x): a radius whose float(r * r) differs from r * r and an f32 coordinate x
    whose square lies between the two, so a target at distance x is a correspondence
    under one threshold and none under the other (Open3D hands FLANN the float)."""
    for r in (0.05, 0.07, 0.03, 0.11, 0.013, 0.3, 0.7, 0.09, 0.023):
        lo, hi = sorted((float(np.float32(r * r)), r * r))
        if lo == hi:
            continue
        x = np.float32(np.sqrt(lo))
        for _ in range(8):
            if lo <= float(x) * float(x) < hi:
                return r, float(x)
            x = np.nextafter(x, np.float32(1.0))
    raise AssertionError("no radius with an f32 coordinate between float(r*r) and r*r")


def _spots(rng, n, size):
    """n <= 64 points, one per cell of a 4 x 4 x 4 lattice of step 1, each within
    `size` of its cell's corner: no two within 1 - size of each other."""
    g = np.arange(4.0)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)[:n] + rng.random((n, 3)) * size


def icp_case(name):
    rng = np.random.default_rng(hash_name(name))
    I = np.eye(4)
    cloud = lambda n: rng.random((n, 3))  # noqa: E731
    if name == "none_identity":       # every target 5 away: count == 0 at the start
        s = cloud(40)
        return ICase(_f32(s), _f32(s + 5.0), I, ICP_D)
    if name == "none_init":           # the same with an init that is not the identity
        s = cloud(40)
        return ICase(_f32(s), _f32(s + 5.0), NON_IDENTITY, ICP_D)
    if name in ("one_corr", "two_corr"):   # k sources near a target, the rest far: rank-deficient Horn
        k = 1 if name == "one_corr" else 2
        s = _spots(rng, 20, 0.25)
        t = s + 7.0
        t[:k] = s[:k] + 0.0625
        return ICase(_f32(s), _f32(t), I, ICP_D)
    if name == "n1":
        s = cloud(1)
        return ICase(_f32(s), _f32(np.concatenate([s + 0.03125, cloud(6) + 3.0])), I, ICP_D)
    if name == "m1":
        s = cloud(33) * 0.125
        return ICase(_f32(s), _f32(s[:1] + 0.015625), I, ICP_D)
    if name == "at_d":                # dyadic coordinates: the first source is exactly d from its target
        s = np.round(_spots(rng, 30, 0.25) * 64.0) / 64.0
        t = s + np.array([0.125, 0.0, 0.0])
        t[0] = s[0] + np.array([0.0, ICP_D, 0.0])
        return ICase(_f32(s), _f32(t), I, ICP_D)
    if name == "float_thr":
        r, x = float_radius()
        s = _spots(rng, 30, 0.25)
        t = s + np.array([0.0, 0.0, r * 0.25])
        s[0] = 0.0
        t[0] = [x, 0.0, 0.0]
        return ICase(_f32(s), _f32(t), I, r)
    if name == "dup_targets":         # every target twice: the lower index wins
        s = cloud(50)
        t = np.repeat(s @ _rigid(0.02, 0.01, -0.02, [0, 0, 0])[:3, :3].T + 0.03125, 2, axis=0)
        return ICase(_f32(s), _f32(t), I, ICP_D)
    if name == "collinear":           # both clouds on one line
        u = np.sort(rng.random(65))
        s = u[:, None] * np.array([1.0, 0.5, 0.25])
        return ICase(_f32(s), _f32(s + np.array([0.03125, 0.0625, 0.0])), I, ICP_D)
    if name == "identical":           # all sources one point, all targets one point
        return ICase(np.full((70, 3), 0.5, np.float32), np.full((9, 3), 0.5625, np.float32), I, ICP_D)
    if name == "ordinary":            # a plain small pair, for max_iteration 0 and 1
        s = cloud(257)
        T = _rigid(0.03, -0.02, 0.04, [0.02, -0.03, 0.01])
        return ICase(_f32(s), _f32(s @ T[:3, :3].T + T[:3, 3]), I, ICP_D / 2)
    raise KeyError(name)


ICP_CASES = ("none_identity", "none_init", "one_corr", "two_corr", "n1", "m1", "at_d", "float_thr",
             "dup_targets", "collinear", "identical", "ordinary")


@functools.lru_cache(maxsize=None)
def icase(name):
    c = icp_case(name)
    for a in (c.src, c.tgt, c.init):
        a.setflags(write=False)
    return c


def jitter_init(init, k):
    """init of copy k: copy 0 keeps the case's own (the exact identity stays one)."""
    if k == 0:
        return init
    rng = np.random.default_rng(7000 + k)
    return _rigid(*rng.normal(0.0, 0.01, 3), rng.normal(0.0, 0.01, 3)) @ init


def oracle_icp(oracle, name, max_iteration, k=0):
    """oracle.icp of copy k of a case at max_iteration, once per session."""
    key = ("icp", name, max_iteration, k)
    if key not in _memo:
        c = icase(name)
        _memo[key] = _freeze(oracle.icp(c.src, c.tgt, c.d, init=jitter_init(c.init, k),
                                        max_iteration=max_iteration))
    return _memo[key]
