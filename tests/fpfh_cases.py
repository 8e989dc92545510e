"""Inputs that drive the f1 kernels (csrc/fpfh.hip) through the branches ordinary
clouds never reach: neighbour lists longer than max_nn, longer than the 512-entry LDS
list, longer than one wave, and the degenerate ones.  Shared by
test_fpfh_cases_cpu.py (which proves from brute-force counts that each case still
meets the condition it is named for) and test_fpfh_edges_gpu.py.

Every case is a deterministic function of a fixed seed and returns
(points (N,3) f32, r, notes); notes is a dict of what the construction knows.
Results computed from a case are cached here so that both test files, and every
test in them, share one brute force / oracle run per (case, K)."""
import functools

import numpy as np

import fpfh_ref

K_LIMIT = 448          # features.MAX_NN_LIMIT
LDS_CAP = 512          # kCap of csrc/fpfh.hip: entries of the LDS list
WAVE = 64


def blob():
    """1400 points of N(0, 0.01) -- nearly all within r of each other, in the cells
    around the origin -- and 300 of U(-0.3, 0.3): the list overflows the LDS cap more
    than once mid-stream, and every max_nn cuts."""
    rng = np.random.default_rng(0)
    p = np.concatenate([rng.normal(0.0, 0.01, (1400, 3)), rng.uniform(-0.3, 0.3, (300, 3))])
    return p.astype(np.float32), 0.05, {"dense": 1400}


def blob400():
    """blob at a size the pure-Python numpy_fpfh can afford."""
    rng = np.random.default_rng(0)
    p = np.concatenate([rng.normal(0.0, 0.01, (300, 3)), rng.uniform(-0.3, 0.3, (100, 3))])
    return p.astype(np.float32), 0.05, {"dense": 300}


CLUSTER_SIZES = (447, 448, 449, 511, 512, 513, 575, 576, 577)


def clusters():
    """Nine clusters 1.0 apart along x, each U(-0.004, 0.004)^3 (diameter < r), of
    exactly K-1, K, K+1, cap-1, cap, cap+1 and cap+63, cap+64, cap+65 points: every
    point of a cluster has the cluster as its in-radius set.  Rows shuffled."""
    rng = np.random.default_rng(1)
    parts, label = [], []
    for c, m in enumerate(CLUSTER_SIZES):
        q = rng.uniform(-0.004, 0.004, (m, 3))
        q[:, 0] += float(c)
        parts.append(q)
        label.append(np.full(m, c))
    p, label = np.concatenate(parts), np.concatenate(label)
    o = rng.permutation(len(p))
    return p[o].astype(np.float32), 0.05, {"label": label[o], "sizes": CLUSTER_SIZES}


def lattice():
    """13^3 lattice of spacing 1/16 about the origin, rows shuffled, r = 0.25: r*r is
    exactly 0.0625 in f32 and the pairs 4 steps apart along an axis sit exactly on it
    (strict <: excluded); distances repeat in large groups that index order breaks."""
    g = np.arange(-6, 7) / 16.0
    p = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    o = np.random.default_rng(2).permutation(len(p))
    return p[o].astype(np.float32), 0.25, {"on_thr_pairs": 6 * 9 * 13 * 13}


def identical():
    """600 copies of one point: every d2 is 0, the order is the index alone."""
    return np.full((600, 3), 0.25, np.float32), 0.05, {}


def sparse():
    """Groups of 1, 2, 3 and 4 points, a 200-point exact line and a 200-point exact
    tilted plane (dyadic coordinates, exact in f32), each more than 10 r from the rest.
    notes gives each part's row range."""
    rng = np.random.default_rng(3)
    r = 0.05
    s = rng.choice(40 * 20, 200, replace=False)
    u, v = (s % 40) / 128.0, (s // 40) / 128.0
    plane = np.stack([u, v, 0.5 * u + 0.25 * v + 0.125], 1)
    t = np.sort(rng.choice(400, 200, replace=False)) / 256.0
    line = t[:, None] * np.array([1.0, 0.5, 0.25]) + np.array([2.0, 0.0, 0.0])
    g1 = np.array([[4.0, 0.0, 0.0]])
    g2 = np.array([[5.0, 0.0, 0.0], [5.0078125, 0.0, 0.0]])
    g3 = np.array([[6.0, 0.0, 0.0], [6.015625, 0.0, 0.0], [6.0, 0.0078125, 0.00390625]])
    g4 = np.array([[7.0, 0.0, 0.0], [7.015625, 0.0, 0.0], [7.0, 0.015625, 0.0], [7.0, 0.0, 0.0078125]])
    parts = {"plane": plane, "line": line, "g1": g1, "g2": g2, "g3": g3, "g4": g4}
    rows, at = {}, 0
    for k, q in parts.items():
        rows[k] = (at, at + len(q))
        at += len(q)
    p = np.concatenate(list(parts.values()))
    assert np.array_equal(p.astype(np.float32).astype(np.float64), p)   # exact in f32
    return p.astype(np.float32), r, {"rows": rows,
                                     "plane_normal": np.array([-0.5, -0.25, 1.0]) / np.sqrt(1.3125)}


CASES = {"blob": blob, "blob400": blob400, "clusters": clusters, "lattice": lattice,
         "identical": identical, "sparse": sparse}

# max_nn values the GPU tests run each case's search with (the CPU file proves the
# oracle against brute force at the same ones)
SEARCH_K = {"blob": (1, 2, 3, 30, 64, 100, 448), "clusters": (448,), "lattice": (100, 448),
            "identical": (448,), "sparse": (30, 100), "blob400": (30, 100)}
NORMALS_K = {"blob": 30, "blob400": 30, "sparse": 30, "identical": 30, "clusters": 448}
FPFH_K = {"blob": (1, 2, 100, 448), "clusters": (448,), "identical": (448,), "sparse": (100,),
          "blob400": (100,)}


@functools.lru_cache(maxsize=None)
def get(name):
    p, r, notes = CASES[name]()
    p.setflags(write=False)
    return p, r, notes


@functools.lru_cache(maxsize=None)
def brute(name, K):
    """brute_hybrid of a case at max_nn K: (idx, d2, cnt, full_cnt), read-only."""
    p, r, _ = get(name)
    if K != K_LIMIT:   # one distance pass per case: cut the longest list
        idx, d2, cnt, full = brute(name, K_LIMIT)
        out = (np.ascontiguousarray(idx[:, :K]), np.ascontiguousarray(d2[:, :K]),
               np.minimum(cnt, K).astype(np.int32), full)
    else:
        out = fpfh_ref.brute_hybrid(p, r, K)
    for a in out:
        a.setflags(write=False)
    return out


_memo = {}


def memo(key, fn):
    """fn() once per key: oracle results shared among the tests of a session."""
    if key not in _memo:
        v = fn()
        for a in (v if isinstance(v, tuple) else (v,)):
            a.setflags(write=False)
        _memo[key] = v
    return _memo[key]


def oracle_search(oracle, name, K):
    p, r, _ = get(name)
    return memo(("search", name, K), lambda: oracle.hybrid_search(p, r, K))


def prior(name):
    """The random prior normals of a case."""
    p, _, _ = get(name)
    return memo(("prior", name), lambda: np.random.default_rng(7).standard_normal(p.shape))


def oracle_normals(oracle, name, with_prior=False):
    p, r, _ = get(name)
    pr = prior(name) if with_prior else None
    return memo(("normals", name, with_prior),
                lambda: oracle.estimate_normals(p, r, NORMALS_K[name], prior=pr))


def fpfh_normals(oracle, name):
    """The normals the FPFH runs take: the oracle's at (r, 30), no prior."""
    p, r, _ = get(name)
    return memo(("fnormals", name), lambda: oracle.estimate_normals(p, r, 30))


def oracle_fpfh(oracle, name, K):
    p, r, _ = get(name)
    return memo(("fpfh", name, K), lambda: oracle.fpfh(p, fpfh_normals(oracle, name), r, K))


def blob400_numpy(oracle):
    """numpy_fpfh of blob400 at K = 100 on brute-force lists: (spfh, fpfh)."""
    p, _, _ = get("blob400")
    idx, d2, cnt, _ = brute("blob400", 100)
    return memo(("np_fpfh",), lambda: fpfh_ref.numpy_fpfh(p, fpfh_normals(oracle, "blob400"), idx, d2, cnt))


def live(name, K):
    """Points whose FPFH groups must sum to 200: a list of more than one entry (the own
    SPFH groups then sum to 100) holding a neighbour at d2 != 0 (the weighted sum is
    then non-empty and normalised to 100; every neighbour has the point itself in
    radius, so its own list has more than one entry whenever K >= 2)."""
    _, d2, cnt, _ = brute(name, K)
    return (cnt > 1) & (d2[:, 1:] != 0.0).any(1)
