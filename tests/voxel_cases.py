"""Inputs that drive f2 (csrc/voxel.hip, csrc/voxel_runs.hip, geometry.py) through
the paths random clouds never reach: points on and one ulp either side of a cell
face, sort keys that fill all 64 bits or have unequal fields, a batch large enough
for the threaded host replay, batches with empty / one-point / one-voxel clouds and
normals with NaNs, and one voxel that holds most of a cloud.  Shared by
test_voxel_cases_cpu.py (which proves, from the oracle and numpy alone, that each
case still meets the condition it is named for) and test_voxel_edges_gpu.py.

No GPU and no torch here.  Every builder is a deterministic function of fixed seeds;
a case is a Case(clouds, normals, colors, voxel) of f64 arrays (normals / colors are
lists like clouds, or None).  Oracle results are cached so that both test files, and
every test in them, share one oracle run per (cloud, voxel)."""
import collections
import functools

import numpy as np

Case = collections.namedtuple("Case", "clouds normals colors voxel")


# ---- the independent grouping --------------------------------------------------

def _numpy_groups(pts, voxel, normals=None, colors=None):
    """Voxel means of one cloud by numpy alone, in np.unique's key order (compare
    order-free).  Sums are sequential f64 additions from zero in input order
    (AccumulatedPoint::AddPoint): round j adds every voxel's j-th point at once, so
    each voxel still sees its own points one after the other.  With normals and / or
    colors, returns (points, normals or None, colors or None); a normal with a NaN
    component adds nothing but still counts in the divisor."""
    pts = np.asarray(pts, np.float64).reshape(-1, 3)
    vmin = pts.min(0) - voxel * 0.5
    keys = np.floor((pts - vmin) / voxel).astype(np.int64)
    uk, inv, cnt = np.unique(keys, axis=0, return_inverse=True, return_counts=True)
    inv = inv.reshape(-1)
    order = np.argsort(inv, kind="stable")           # by voxel, input order inside
    start = np.concatenate([[0], np.cumsum(cnt)[:-1]])
    by_len = np.argsort(-cnt, kind="stable")         # voxels with > j points: a prefix
    n_longer = len(cnt) - np.searchsorted(cnt[by_len][::-1], np.arange(cnt.max()), side="right")

    def means(vals):
        s = np.zeros((len(uk), 3))
        for j in range(int(cnt.max())):
            g = by_len[:n_longer[j]]
            s[g] = s[g] + vals[order[start[g] + j]]
        return s / cnt.astype(np.float64)[:, None]

    out_p = means(pts)
    if normals is None and colors is None:
        return out_p
    out_n = out_c = None
    if normals is not None:
        nr = np.asarray(normals, np.float64).reshape(-1, 3)
        out_n = means(np.where(np.isnan(nr).any(1, keepdims=True), 0.0, nr))
    if colors is not None:
        out_c = means(np.asarray(colors, np.float64).reshape(-1, 3))
    return out_p, out_n, out_c


def sorted_rows(a):
    return a[np.lexsort(a.T[::-1])]


def quotients(pts, voxel):
    """(p - voxel_min_bound) / voxel, the f64 value the voxel index is the floor of."""
    pts = np.asarray(pts, np.float64)
    return (pts - (pts.min(0) - voxel * 0.5)) / voxel


def key_bits(pts, voxel):
    """Per axis, the bit count of the widest voxel index floor((max - vmb) / voxel)."""
    return tuple(int(v).bit_length() for v in np.floor(quotients(pts, voxel).max(0)).astype(np.int64))


# ---- builders ------------------------------------------------------------------

LATTICE_VOXELS = (0.1, 0.05, 1.0 / 3.0, 0.3, 0.025, 1.0)
LATTICE_BASES = (0.0, -7.3, 1234.5)


def lattice(voxel, base):
    """An anchor at (base, base, base) -- the cloud's minimum, so voxel_min_bound is
    base - voxel / 2 -- and base + (g + 0.5) * voxel for g on a 40 x 5 x 3 integer
    grid: 601 points whose quotients are nominally the integers g + 1, i.e. on a cell
    face of all three axes.  In f64 they land on the integer or an ulp either side."""
    g = np.stack(np.meshgrid(np.arange(40.0), np.arange(5.0), np.arange(3.0), indexing="ij"), -1).reshape(-1, 3)
    pts = np.concatenate([np.full((1, 3), float(base)), base + (g + 0.5) * voxel])
    return Case([pts], None, None, float(voxel))


WIDE_VOXEL = 0.25
WIDE_SINGLE = ((22, 21, 21), (30, 3, 12), (3, 30, 12))   # 64 bits in one cloud; unequal fields
WIDE_BATCH = (21, 21, 21)                                # 63 bits + 1 cloud bit
WIDE_TOO_FINE = (22, 22, 21)                             # 65 bits: the library rejects it


def wide_cloud(bits, seed=0):
    """3000 uniform points in a box of 0.9 * 2**bits[i] * voxel per axis, rows 0 and 1
    on its two corners (the widest index then has exactly bits[i] bits), and the
    first 500 rows again shifted by +1e-3: runs of two, a few split by a face."""
    rng = np.random.default_rng(100 + seed)
    ext = 0.9 * np.exp2(np.asarray(bits, np.float64)) * WIDE_VOXEL
    p = rng.random((3000, 3)) * ext
    p[0], p[1] = 0.0, ext
    return np.concatenate([p, p[:500] + 1e-3])


def wide_keys(bits):
    """One cloud per requested field widths; WIDE_BATCH gives two clouds."""
    n = 2 if tuple(bits) == WIDE_BATCH else 1
    return Case([wide_cloud(bits, s) for s in range(n)], None, None, WIDE_VOXEL)


def threaded_replay():
    """60000, 0 and 60000 points uniform in [0,100] x [0,100] x [0,4] at voxel 0.5:
    about 55k voxels per cloud, so V >= 65536 over two non-empty clouds -- the branch
    of voxel.hip that replays the clouds' map orders on host threads."""
    rng = np.random.default_rng(11)
    clouds = [rng.random((k, 3)) * np.array([100.0, 100.0, 4.0]) for k in (60000, 0, 60000)]
    return Case(clouds, None, None, 0.5)


LAYOUTS = ((0, 700), (700, 0), (300, 0, 0, 300), (1, 500), (500, 1, 1), (40,) * 5, (40,) * 9)
LAYOUT_VOXEL = 0.4
ONE_VOXEL = ((40,) * 5, 2)     # (layout, cloud) that lies inside a single voxel


def layout(lens):
    """Clouds of the given lengths, uniform in [0, 3]^3 about differing origins (about
    500 cells at voxel 0.4), with normals whose rows have a NaN in component i % 3 for
    every 7th row (phase differing per cloud) and colors.  The ONE_VOXEL cloud spans
    less than voxel / 2 per axis, so all of it has voxel index (0, 0, 0)."""
    rng = np.random.default_rng(1000 + 31 * len(lens) + sum(lens))
    clouds, normals, colors = [], [], []
    for b, k in enumerate(lens):
        span = 0.45 * LAYOUT_VOXEL if (tuple(lens), b) == ONE_VOXEL else 3.0
        clouds.append(rng.random((k, 3)) * span + rng.uniform(-5.0, 5.0, 3))
        nr = rng.standard_normal((k, 3))
        rows = np.arange(b % 7, k, 7)
        nr[rows, rows % 3] = np.nan
        normals.append(nr)
        colors.append(rng.random((k, 3)))
    return Case(clouds, normals, colors, LAYOUT_VOXEL)


LONG_RUN = 20000


def long_run():
    """20000 points inside one voxel among 2000 ordinary ones, rows shuffled, all near
    1e6: the big voxel's sequential f64 sum (about 2e10, ulp 4e-6) rounds at nearly
    every step, so its bits depend on the order of the additions.  One ordinary row is
    (1e6, 1e6, 1e6), the minimum: cell faces at 1e6 - 0.5 + k, the big voxel is
    (11, 11, 11)."""
    rng = np.random.default_rng(12)
    big = 1e6 + 10.6 + 0.8 * rng.random((LONG_RUN, 3))
    rest = 1e6 + 20.0 * rng.random((2000, 3))
    rest[0] = 1e6
    p = np.concatenate([big, rest])[rng.permutation(LONG_RUN + 2000)]
    return Case([p], None, None, 1.0)


def _name(x):
    return "-".join(str(round(v, 4) if isinstance(v, float) else v) for v in x)


CASES = {}
for _v in LATTICE_VOXELS:
    for _b in LATTICE_BASES:
        CASES[f"lattice-{_name((_v, _b))}"] = functools.partial(lattice, _v, _b)
for _bits in WIDE_SINGLE + (WIDE_BATCH, WIDE_TOO_FINE):
    CASES[f"wide-{_name(_bits)}"] = functools.partial(wide_keys, _bits)
CASES["threaded"] = threaded_replay
for _l in LAYOUTS:
    CASES[f"layout-{_name(_l)}"] = functools.partial(layout, _l)
CASES["long_run"] = long_run

LATTICE_NAMES = [n for n in CASES if n.startswith("lattice-")]
LAYOUT_NAMES = [n for n in CASES if n.startswith("layout-")]


def lattice_name(voxel, base):
    return f"lattice-{_name((voxel, base))}"


def wide_name(bits):
    return f"wide-{_name(bits)}"


def layout_name(lens):
    return f"layout-{_name(lens)}"


@functools.lru_cache(maxsize=None)
def get(name):
    case = CASES[name]()
    for group in (case.clouds, case.normals, case.colors):
        for a in group or ():
            a.setflags(write=False)
    return case


# ---- shared oracle results -------------------------------------------------------

_memo = {}


def oracle_cloud(oracle, key, pts, voxel, normals=None, colors=None):
    """oracle.voxel_down_sample of one cloud, once per key, read-only.  An empty
    cloud gives (0, 3) arrays for points and for each extra that was passed."""
    if key not in _memo:
        if len(pts):
            out = oracle.voxel_down_sample(pts, voxel, normals, colors)
        else:
            e = np.zeros((0, 3))
            out = (e, None if normals is None else e.copy(), None if colors is None else e.copy())
        for a in out:
            if a is not None:
                a.setflags(write=False)
        _memo[key] = out
    return _memo[key]


def oracle_case(oracle, name, voxel=None):
    """Per cloud of a case, the oracle's (points, normals or None, colors or None) at
    the case's voxel size (or the given one)."""
    case = get(name)
    v = case.voxel if voxel is None else float(voxel)
    return [oracle_cloud(oracle, (name, b, v), p, v, case.normals[b] if case.normals else None,
                         case.colors[b] if case.colors else None)
            for b, p in enumerate(case.clouds)]
