"""featnn_thresh9 with its hits in LDS and its column stream staged in LDS
groups (csrc/featnn_thresh.hip): a block keeps a counter
and kThreshK slots per listed row in LDS, adds each row's local count to the
row's global count once per column slice and copies the local slots that land
below kThreshK (thresh_flush_count, csrc/featnn_thresh.h).

Bar, as tests/test_featthresh_gpu.py: bit-exact -- nn12, n_corres and the
correspondence list equal the oracle's, through the same entry (`_check`: the
threshold route and the 3-term route).  The shapes are the smallest at which
the LDS lists can go wrong:
  * the slot boundary: kThreshK exact copies fit (the candidates decide, the
    lowest index), kThreshK + 1 overflow to the exact rescan -- inside one
    column tile (one lane takes every hit in one step), spread 3 + 3 + 2 (+ 1)
    over column slices (P = 1 has 32 slices: the global count is a sum of
    block-local counts), and across an LDS group boundary and in the ragged
    last step;
  * more listed rows than a block round holds (512): counters and slots are
    cleared and reused;
  * a pair whose bias is 2^60 (an infinite element) beside finite pairs;
  * ragged counts: padding columns never become candidates; a pair with an
    empty list, a pair without columns.
`twin_src`: the structure (copies, twins) sits in the target cloud (pass 1,
kIdx = true, meets it) or in the source cloud (pass 2, kIdx = false).

The CPU test runs the host check of the flush arithmetic
(tests/cpp/thresh_flush_check.cpp) under -fsanitize=address,undefined."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from test_featthresh_gpu import CSRC, K_SLOTS, ROOT, _MEMO, _check, _run

G_TILES = 16   # kThreshG: column tiles per LDS group (csrc/featnn_thresh.hip)
ROUND_ROWS = 512  # rows of a block round

# (D, twin_src): D = 32 and 16 in both directions, D = 17 once
DIRS = [(32, False), (32, True), (16, False), (16, True)]
DIRS17 = DIRS + [(17, False)]


def test_flush_arithmetic_under_sanitizers(tmp_path):
    """CPU: thresh_flush_count against a plain model of the slices' flushes --
    positions within the K slots, no slot written twice, overflow exactly when
    the total exceeds K, nothing written past a row's slots; a plain executable
    under ASan + UBSan."""
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "thresh_flush_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "thresh_flush_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok:"), r.stdout


def _clouds(rng, n, m, d):
    """A small cloud A (2 n rows) and a large one B (m rows): n rows of B have a
    twin 1e-2 away in B, A holds a noisy copy of each of those rows and that
    copy's own twin -- both directions have rows the 1-term screen cannot
    certify, two or three candidates each."""
    B = rng.standard_normal((m, d)).astype(np.float32)
    idx = rng.permutation(m)[:2 * n]
    B[idx[n:]] = B[idx[:n]] + (1e-2 * rng.standard_normal((n, d))).astype(np.float32)
    A = (B[idx[:n]] + 0.5 * rng.standard_normal((n, d))).astype(np.float32)
    A = np.concatenate([A, (A + 1e-2 * rng.standard_normal((n, d))).astype(np.float32)])
    return A, B


def _plant(rng, A, B, row, cols):
    """Row `row` of A next to a fresh vector whose exact copies are B's `cols`."""
    z = rng.standard_normal(A.shape[1]).astype(np.float32)
    A[row] = z + (0.3 * rng.standard_normal(A.shape[1])).astype(np.float32)
    B[list(cols)] = z


def _slot_boundary(oracle, monkeypatch, key, D, twin_src, n, m, plants):
    """plants: per planted row of the small cloud, the K + 1 columns of the
    large cloud its copies take; the first K of them, then all.  The copies in
    the target cloud: pass 1's rescan counter is exact -- with K copies no row
    reaches the exact rescan, with K + 1 the planted rows do.  The copies in the
    source cloud: the column rescan also takes columns the resolve could not
    decide, so its counter is compared between the two runs."""
    x = []
    for extra in (0, 1):
        rng = np.random.default_rng(1000 + D + 7 * twin_src + m)
        A, B = _clouds(rng, n, m, D)
        taken = set()
        for i, cols in enumerate(plants):
            assert len(set(cols)) == K_SLOTS + 1 and not taken & set(cols) and max(cols) < m
            taken |= set(cols)
            _plant(rng, A, B, 3 + 5 * i, cols[:K_SLOTS + extra])
        F, G = (B, A) if twin_src else (A, B)
        (r12, c21), (x12, x21) = _check(oracle, monkeypatch, key + (D, twin_src, extra), F[None], G[None])
        print(key, D, twin_src, extra, "listed", r12, c21, "rescanned", x12, x21)
        assert r12 > 0 and c21 > 0, (r12, c21)  # both passes ran the threshold sweep
        x.append(x21 if twin_src else x12)
    if twin_src:
        assert x[1] > x[0], x
    else:
        assert x[0] == 0 and x[1] >= len(plants), x


@pytest.mark.gpu
@pytest.mark.parametrize("D,twin_src", DIRS17)
def test_slot_boundary_in_one_tile(oracle, monkeypatch, D, twin_src):
    """K and K + 1 copies in one 32-column tile, all in columns one lane half
    holds (8 (r / 4) + (r % 4)): one lane takes every hit in one step -- and a
    second row whose copies alternate between the tile's lane halves."""
    one_lane = [64 + c for c in (0, 1, 2, 3, 8, 9, 10, 11, 16)]
    both = [160 + c for c in (0, 4, 1, 5, 9, 13, 26, 30, 31)]
    _slot_boundary(oracle, monkeypatch, ("lds_tile",), D, twin_src, 40, 257, [one_lane, both])


@pytest.mark.gpu
@pytest.mark.parametrize("D,twin_src", DIRS)
def test_slot_boundary_across_slices(oracle, monkeypatch, D, twin_src):
    """One pair has 32 column slices; 2048 + 33 columns are 33 steps, so slice
    i is step i (the last one two steps).  The copies sit 3 + 3 + 2 (+ 1) in
    three slices: the row's count is a sum of three blocks' local counts, the
    last of them in the ragged last step."""
    m = 2048 + 33
    cols = [64 * 5 + 1, 64 * 5 + 33, 64 * 5 + 63, 64 * 17, 64 * 17 + 31, 64 * 17 + 32,
            64 * 32 + 2, m - 1, 64 * 32 + 17]
    _slot_boundary(oracle, monkeypatch, ("lds_slices",), D, twin_src, 40, m, [cols])


@pytest.mark.gpu
@pytest.mark.parametrize("D,twin_src", DIRS)
def test_slot_boundary_across_lds_groups(oracle, monkeypatch, D, twin_src):
    """293 column steps in 32 slices: slice 0 is steps 0..8 and slice 31 steps
    283..292, more than one LDS group of 8 steps each.  One row's copies
    straddle slice 0's group boundary (columns 511 | 512); another's sit on
    both sides of slice 31's (steps 290 | 291) and in the ragged last step,
    the last column among them."""
    gs = G_TILES // 2
    m = 293 * 64 - 23
    b0 = 64 * gs                      # slice 0: its second group's first column
    first = [b0 - 4, b0 - 3, b0 - 2, b0 - 1, b0, b0 + 1, b0 + 31, b0 + 32, b0 - 64]
    s31 = (293 * 31) // 32            # slice 31's first step
    b1 = 64 * (s31 + gs)              # its second group's first column
    last = [b1 - 1, b1 - 33, b1 - 64, b1, b1 + 63, m - 1, m - 2, 64 * 292, b1 + 70]
    assert s31 == 283 and b1 == 64 * 291 and 64 * 292 < m - 2
    _slot_boundary(oracle, monkeypatch, ("lds_groups",), D, twin_src, 24, m, [first, last])


@pytest.mark.gpu
@pytest.mark.parametrize("D,twin_src", DIRS)
def test_more_listed_rows_than_a_block_round(oracle, monkeypatch, D, twin_src):
    """1100 x 1100: every target has a twin 1e-2 away and every source sits
    1e-4 from a target of its own, so nearly every row and column is listed,
    with two to four candidates: more than 512 listed rows (17+ row tiles) in
    both passes -- a block's LDS counters and slots are cleared and reused."""
    rng = np.random.default_rng(2000 + D)
    b = rng.standard_normal((550, D)).astype(np.float32)
    G = np.concatenate([b, (b + 1e-2 * rng.standard_normal((550, D))).astype(np.float32)])[rng.permutation(1100)]
    F = (G + 1e-4 * rng.standard_normal((1100, D)).astype(np.float32))[rng.permutation(1100)]
    if twin_src:
        F, G = G, F
    (r12, c21), (x12, x21) = _check(oracle, monkeypatch, ("lds_rounds", D, twin_src), F[None], G[None])
    print("rounds", D, twin_src, "listed", r12, c21, "rescanned", x12, x21)
    assert r12 > ROUND_ROWS and c21 > ROUND_ROWS, (r12, c21)
    assert x12 == 0, x12


@pytest.mark.gpu
@pytest.mark.parametrize("D,twin_src", DIRS)
def test_pair_with_infinite_element_beside_finite_pairs(oracle, monkeypatch, D, twin_src):
    """Three pairs of 300 x 300 twins, the middle one with an infinite element
    in one row of the cloud the sweep streams as columns: its bias is 2^60, and
    every column is within every row's threshold (each lane stops counting at
    K + 1 hits).  The run completes and all three pairs equal the oracle."""
    rng = np.random.default_rng(3000 + D + twin_src)
    prs = [_clouds(rng, 75, 300, D) for _ in range(3)]
    A = np.stack([np.concatenate([a, a])[:300] for a, _ in prs])
    B = np.stack([b for _, b in prs])
    B[1, 200, D - 1] = np.inf
    F, G = (B, A) if twin_src else (A, B)
    fb, rs = _check(oracle, monkeypatch, ("lds_inf", D, twin_src), F, G)
    print("inf", D, twin_src, "listed", fb, "rescanned", rs)
    assert fb[0] > 0 and fb[1] > 0, fb


@pytest.mark.gpu
@pytest.mark.parametrize("D,twin_src", DIRS17)
def test_ragged_counts_padding_is_no_candidate(oracle, monkeypatch, D, twin_src):
    """Five pairs with ragged counts.  Past each pair's count the streamed cloud
    holds exact copies of rows of the other cloud (distance 0: as candidates
    they would win) and kThreshK + 1 copies of one of them (they would
    overflow its row).  Pair 3's points are far apart (an empty list) and pair
    4 has no columns at all: its rows come out as index 0."""
    rng = np.random.default_rng(4000 + D + twin_src)
    n, m = 97, 203
    ca = [97, 33, 64, 97, 50]
    cb = [150, 203, 65, 130, 0]
    A = np.zeros((5, n, D), np.float32)
    B = np.zeros((5, m, D), np.float32)
    for p in range(5):
        a, b = _clouds(rng, 48, m, D)
        A[p], B[p] = np.concatenate([a, a[:1]]), b
    A[3] = (30.0 * rng.standard_normal((n, D))).astype(np.float32)
    B[3, :n] = A[3][rng.permutation(n)]
    B[3, n:] = (30.0 * rng.standard_normal((m - n, D))).astype(np.float32) + 500.0
    for p in range(5):
        pad = m - cb[p]
        if pad:
            B[p, cb[p]:] = A[p, rng.integers(0, ca[p], pad)]
            B[p, cb[p]:cb[p] + min(pad, K_SLOTS + 1)] = A[p, 2]
    ns, nt = (np.array(ca, np.int32), np.array(cb, np.int32))
    F, G = (B, A) if twin_src else (A, B)
    if twin_src:
        ns, nt = nt, ns
    # the pair without points in one cloud: no oracle call on an empty cloud
    e = 4
    key = ("lds_ragged", D, twin_src)
    fb, rs = _check(oracle, monkeypatch, key, F[:e], G[:e], ns[:e], nt[:e])
    print("ragged", D, twin_src, "listed", fb, "rescanned", rs)
    nn, nc, co = _run(F, G, ns, nt)
    exp = _MEMO[key]
    for p in range(e):
        e12, ec = exp[p]
        assert np.array_equal(nn[p, :ns[p]], e12), p
        assert int(nc[p]) == len(ec) and np.array_equal(co[p, :len(ec)], ec), p
    # (its rows' index is row_tail's 0; what the mutual stage makes of a pair
    # without columns is not this kernel's)
    assert not nn[e, :ns[e]].any()
