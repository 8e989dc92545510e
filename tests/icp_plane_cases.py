"""Inputs of the point-to-plane ICP tests (CPU and GPU) and their memoised reference
results (tests/icp_plane_ref.py).  Every case is small: the sizes are the ones at which
the kernel's paths change -- fewer points than a wave, one more than a wave, several
chunks per workgroup; fewer than 6 correspondences; one target."""
import functools
from typing import NamedTuple

import numpy as np

import icp_plane_ref as ref
import registration_cases as rc

D = 0.25               # float(d * d) == d * d exactly
ITERS = (0, 1, 2, 30)
AXES = (1.0, 0.7, 0.5)
MOTION = rc._rigid(0.02, -0.015, 0.025, [0.01, -0.02, 0.015])   # well inside D


class PCase(NamedTuple):
    src: np.ndarray    # (n, 3) f32
    tgt: np.ndarray    # (m, 3) f32
    nrm: np.ndarray    # (m, 3) f32
    init: np.ndarray   # (4, 4) f64
    d: float
    kernel: str
    k: float


def ellipsoid(rng, m, axes=AXES):
    """m points on the ellipsoid with semi-axes `axes` and their unit outward normals."""
    u = rng.normal(size=(m, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    a = np.asarray(axes)
    g = u / a
    return u * a, g / np.linalg.norm(g, axis=1, keepdims=True)


def _move_back(p, T):
    """The points that T takes to p."""
    return (p - T[:3, 3]) @ T[:3, :3]


def _near(rng, tgt, n, noise=0.03):
    """n sources, each within `noise` (per axis) of a target drawn at random."""
    j = rng.integers(0, len(tgt), n)
    return tgt[j] + rng.uniform(-noise, noise, (n, 3)), j


KERNELS = ("l2", "huber", "cauchy", "gm", "tukey")
# k below and above the residuals' scale (~0.02; GM's k is on the scale of r^2)
K_LOW_HIGH = {"huber": (0.005, 0.1), "cauchy": (0.005, 0.1), "gm": (1e-4, 0.01), "tukey": (0.01, 0.1)}

SIZE_N = (1, 5, 6, 63, 65, 1000)
SIZE_M = (1, 64, 777)
SIZE_CASES = tuple(f"n{n}_m{m}" for n in SIZE_N for m in SIZE_M)
KERNEL_CASES = ("l2",) + tuple(f"{kn}_{lh}" for kn in KERNELS[1:] for lh in ("low", "high"))
EDGE_CASES = ("none_identity", "none_init", "other_init", "at_d", "float_thr", "nonunit", "nan_normal",
              "planar", "far")
CASES = SIZE_CASES + KERNEL_CASES + EDGE_CASES


def _ordinary(rng, n, m, kernel, k, noise=0.03):
    t, nr = ellipsoid(rng, m)
    s, j = _near(rng, t, n, noise)
    return _move_back(s, MOTION), t, nr, j


def make_case(name):
    rng = np.random.default_rng(rc.hash_name("plane_" + name))
    I = np.eye(4)
    f = rc._f32
    if name in SIZE_CASES:
        n, m = (int(v[1:]) for v in name.split("_"))
        kn = KERNELS[SIZE_CASES.index(name) % len(KERNELS)]
        k = 1.0 if kn == "l2" else K_LOW_HIGH[kn][1]
        s, t, nr, _ = _ordinary(rng, n, m, kn, k)
        return PCase(f(s), f(t), f(nr), I, D, kn, k)
    if name in KERNEL_CASES:
        kn, _, lh = name.partition("_")
        k = 1.0 if kn == "l2" else K_LOW_HIGH[kn][lh == "high"]
        s, t, nr, _ = _ordinary(rng, 65, 777, kn, k)
        return PCase(f(s), f(t), f(nr), I, D, kn, k)
    if name in ("none_identity", "none_init"):   # every target 5 away: count == 0 at the start
        s, t, nr, _ = _ordinary(rng, 40, 64, "l2", 1.0)
        return PCase(f(s), f(t + 5.0), f(nr), I if name == "none_identity" else rc.NON_IDENTITY, D, "tukey", 0.1)
    if name == "other_init":           # the init carries most of the motion
        s, t, nr, _ = _ordinary(rng, 65, 64, "l2", 1.0)
        return PCase(f(_move_back(s, rc.NON_IDENTITY)), f(t), f(nr), rc.NON_IDENTITY, D, "huber", 0.02)
    if name == "at_d":                 # dyadic coordinates: the first source is exactly d from its target
        s = np.round(rc._spots(rng, 30, 0.25) * 64.0) / 64.0
        t = s + np.array([0.125, 0.0, 0.0])
        t[0] = s[0] + np.array([0.0, D, 0.0])
        nr = rng.normal(size=(30, 3))
        return PCase(f(s), f(t), f(nr / np.linalg.norm(nr, axis=1, keepdims=True)), I, D, "l2", 1.0)
    if name == "float_thr":            # a radius whose float square differs from its f64 square
        r, x = rc.float_radius()
        s = rc._spots(rng, 30, 0.25)
        t = s + np.array([0.0, 0.0, r * 0.25])
        s[0] = 0.0
        t[0] = [x, 0.0, 0.0]
        nr = rng.normal(size=(30, 3))
        return PCase(f(s), f(t), f(nr / np.linalg.norm(nr, axis=1, keepdims=True)), I, r, "cauchy", 0.05)
    if name == "nonunit":              # normals of lengths 0.5 .. 3
        s, t, nr, _ = _ordinary(rng, 65, 64, "l2", 1.0)
        return PCase(f(s), f(t), f(nr * rng.uniform(0.5, 3.0, (64, 1))), I, D, "tukey", 0.2)
    if name == "nan_normal":           # the normal of a target that has correspondences is NaN
        s, t, nr, j = _ordinary(rng, 65, 64, "l2", 1.0)
        nr[j[0]] = np.nan
        nr[j[1], 1] = np.inf
        return PCase(f(s), f(t), f(nr), I, D, "l2", 1.0)
    if name == "planar":               # a plane with equal normals: A has rank 3, the third pivot is exactly 0
        g = np.arange(8.0) * 0.125
        t = np.stack(np.meshgrid(g, g, [0.0], indexing="ij"), -1).reshape(-1, 3)
        s = np.concatenate([t, t[:1]]) + np.concatenate([rng.uniform(-0.03, 0.03, (65, 2)),
                                                         np.full((65, 1), 0.03125)], axis=1)
        return PCase(f(s), f(t), f(np.tile([0.0, 0.0, 1.0], (64, 1))), I, D, "l2", 1.0)
    if name == "far":                  # coordinates around 1e3: a coarse quantum
        s, t, nr, _ = _ordinary(rng, 65, 64, "l2", 1.0)
        return PCase(f(s + 1000.0), f(t + 1000.0), f(nr), I, D, "huber", 0.05)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def case(name):
    c = make_case(name)
    for a in (c.src, c.tgt, c.nrm, c.init):
        a.setflags(write=False)
    return c


_memo = {}


def reference(name, max_iteration, k=0):
    """icp_plane_ref.icp_plane of copy k (rc.jitter_init) of a case, once per session."""
    key = (name, max_iteration, k)
    if key not in _memo:
        c = case(name)
        _memo[key] = ref.icp_plane(c.src, c.tgt, c.nrm, c.d, init=rc.jitter_init(c.init, k), kernel=c.kernel,
                                   k=c.k, max_iteration=max_iteration)
    return _memo[key]


def big_target_case():
    """A target too large for the grid's LDS copy (csrc/lds_fit.h: 16 B per point and 2 B
    per slot within 160 KiB less the kernel's header; 8193 points take 16384 slots and
    do not fit), few sources."""
    rng = np.random.default_rng(rc.hash_name("plane_big_target"))
    t, nr = ellipsoid(rng, 8200)
    s, _ = _near(rng, t, 40, 0.02)
    return PCase(rc._f32(_move_back(s, MOTION)), rc._f32(t), rc._f32(nr), np.eye(4), 0.1, "tukey", 0.05)
