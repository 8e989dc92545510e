"""The two forms of the 1-term sweep featnn_row9 (csrc/featnn_row.hip): rows
stationary (a wave keeps two row tiles, the block streams the columns through
LDS) and columns stationary (a wave keeps a step's column tiles and runs over
the block's 16 row tiles in LDS; the waves split the steps and merge their
(B1, B2, I) triples at the end, csrc/row9_merge.h).  PCR_ROW9_SWEEP=rows|cols|
cols8 selects the form (cols: four waves per block; cols8: eight).

Bar, under every form: nn12, n_corres and the correspondence list equal the
oracle's bit for bit on both routes of the leftover rows (_check of
test_featthresh_gpu), and the fallback and rescan counters are equal between
the forms -- the routing is a function of (B1, B2, I), so equal counters pin
the merge on the device.

Shapes, the smallest at which the columns-stationary form can go wrong:
column counts 1, 33, 64, 65, 511, 512, 513, 545 (fewer real steps than waves,
waves that see padding only, an odd number of column tiles, the 16-tile padding
boundary); row counts 1, 31, 33, 511, 513 (a partial row tile, a partial block,
a second block with one row); a pass-2 list far shorter than a block; a pair
with an empty list and a pair without columns beside full pairs (9 ragged
pairs); exact duplicate columns in the two lane halves of a tile, the two tiles
of a step, neighbouring steps (different waves), steps W apart (the same wave)
and either side of column 512; near twins whose second value comes from
another wave; a pair whose bias is 2^60.  `twin_src`: the structure sits in the
target cloud (pass 1 meets it) or in the source cloud (pass 2).

The counters are a function of the triples only while no bucket of the regroup
overflows: which rows of a full bucket go to the list instead depends on the
order of the appends, in either form.  So every pair here keeps its rows per
winning step under the bucket capacity max(64, 4 rows / steps): many rows only
against many columns with the winners spread over them.

The CPU test runs the host check of the merge (tests/cpp/row9_merge_check.cpp)
under -fsanitize=address,undefined."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from test_featthresh_gpu import COUNTS, CSRC, ROOT, _MEMO, _check, _run

FORMS = ("cols", "rows", "cols8")
DIRS = [(32, False), (32, True), (16, False), (16, True)]
DIRS17 = DIRS + [(17, False)]


def test_merge_under_sanitizers(tmp_path):
    """CPU: the steps split over W = 4 and 8 waves (interleaved as the kernel
    does) and merged give the sequential loop's (B1, B2, I) exactly -- random
    sequences, all equal, the equal smallest in different waves and in the same
    wave, one real step among padding, +inf everywhere; a plain executable
    under ASan + UBSan."""
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "row9_merge_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "row9_merge_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok:"), r.stdout


def _forms(oracle, monkeypatch, key, F, G, ns=None, nt=None):
    """_check under every form; the counters must agree.  Returns them."""
    got = {}
    for form in FORMS:
        monkeypatch.setenv("PCR_ROW9_SWEEP", form)
        got[form] = _check(oracle, monkeypatch, key, F, G, ns, nt)
    monkeypatch.delenv("PCR_ROW9_SWEEP")
    print(key, got)
    for form in FORMS[1:]:
        assert got[form] == got[FORMS[0]], (form, got)
    return got[FORMS[0]]


def _pair(rng, n, m, d):
    """n rows near rows of an m-row cloud; a quarter of the m rows have a twin
    1e-2 away (rows and J columns the 1-term certificate fails)."""
    B = rng.standard_normal((m, d)).astype(np.float32)
    k = m // 4
    idx = rng.permutation(m)[:2 * k]
    B[idx[k:]] = B[idx[:k]] + (1e-2 * rng.standard_normal((k, d))).astype(np.float32)
    A = (B[rng.integers(0, m, n)] + 0.5 * rng.standard_normal((n, d))).astype(np.float32)
    return A, B


# (rows, columns) of the nine pairs: every row count and every column count
SHAPES = [(513, 545), (511, 511), (513, 513), (511, 512), (33, 65), (31, 64), (33, 33), (31, 1), (1, 33)]


@pytest.mark.gpu
@pytest.mark.parametrize("D,twin_src", DIRS17)
def test_row_and_column_counts(oracle, monkeypatch, D, twin_src):
    """Nine ragged pairs over the row counts {1, 31, 33, 511, 513} and the
    column counts {1, 33, 64, 65, 511, 512, 513, 545}.  Past a pair's count
    each cloud holds exact copies of the other's rows: read, they would win."""
    rng = np.random.default_rng(5000 + D + twin_src)
    P, n, m = len(SHAPES), 513, 545
    A = np.zeros((P, n, D), np.float32)
    B = np.zeros((P, m, D), np.float32)
    for p, (r, c) in enumerate(SHAPES):
        a, b = _pair(rng, r, c, D)
        A[p, :r], B[p, :c] = a, b
        A[p, r:] = b[rng.integers(0, c, n - r)]
        B[p, c:] = a[rng.integers(0, r, m - c)]
    ca = np.array([r for r, _ in SHAPES], np.int32)
    cb = np.array([c for _, c in SHAPES], np.int32)
    F, G, ns, nt = (B, A, cb, ca) if twin_src else (A, B, ca, cb)
    (r12, c21), _ = _forms(oracle, monkeypatch, ("cs_counts", D, twin_src), F, G, ns, nt)
    assert r12 > 0 and c21 > 0, (r12, c21)


@pytest.mark.gpu
@pytest.mark.parametrize("D", [32, 16])
def test_pass2_list_far_shorter_than_a_block(oracle, monkeypatch, D):
    """600 sources around five of 300 targets: J, the rows of pass 2, is a
    handful of columns -- one block per pair with a single partial row tile --
    while pass 1 has a full block and a partial one."""
    rng = np.random.default_rng(5100 + D)
    G = rng.standard_normal((2, 300, D)).astype(np.float32)
    F = np.stack([(G[p, rng.integers(0, 5, 600) * 59] + 0.2 * rng.standard_normal((600, D))).astype(np.float32)
                  for p in range(2)])
    _forms(oracle, monkeypatch, ("cs_shortlist", D), F, G)
    nj = [len(np.unique(e12)) for e12, _ in _MEMO[("cs_shortlist", D)]]
    assert max(nj) <= 5, nj


# nine ragged pairs over the counts of test_featthresh_gpu's COUNTS ({1, 31, 33,
# 257}; 257 sources only against 257 targets: see the module docstring)
NINE = ([257, 1, 31, 33, 33, 31, 1, 257, 33], [257, 33, 1, 31, 257, 257, 31, 257, 0])


@pytest.mark.gpu
@pytest.mark.parametrize("D", [32, 16])
def test_nine_ragged_pairs_empty_list_and_no_columns(oracle, monkeypatch, D):
    """Nine ragged pairs (P is no multiple of 8), twins in both clouds; pair
    3's points are far apart (every row certifies: an empty list) and the last
    pair has no columns at all (its rows come out as index 0)."""
    assert sorted(set(NINE[0] + NINE[1])) == [0] + sorted(set(COUNTS["a"][0]))
    rng = np.random.default_rng(5200 + D)
    ca, cb = NINE
    P, n, m = 9, 257, 257
    A = np.zeros((P, n, D), np.float32)
    B = np.zeros((P, m, D), np.float32)
    for p in range(P):
        a, b = _pair(rng, ca[p], max(cb[p], 1), D)
        A[p, :ca[p]], B[p, :max(cb[p], 1)] = a, b
        k = ca[p] // 4  # a quarter of the sources twinned too
        A[p, k:2 * k] = A[p, :k] + (1e-2 * rng.standard_normal((k, D))).astype(np.float32)
        A[p, ca[p]:] = b[rng.integers(0, len(b), n - ca[p])]
        B[p, cb[p]:] = a[rng.integers(0, ca[p], m - cb[p])]
    A[3, :ca[3]] = (30.0 * rng.standard_normal((ca[3], D))).astype(np.float32)
    B[3, :cb[3]] = A[3, :ca[3]][rng.permutation(ca[3])[:cb[3]]]
    ns, nt = np.array(ca, np.int32), np.array(cb, np.int32)
    key = ("cs_nine", D)
    e = 8  # the pair without points in one cloud: no oracle call on an empty cloud
    _forms(oracle, monkeypatch, key, A[:e], B[:e], ns[:e], nt[:e])
    exp = _MEMO[key]
    for form in FORMS:
        monkeypatch.setenv("PCR_ROW9_SWEEP", form)
        nn, nc, co = _run(A, B, ns, nt)
        for p in range(e):
            e12, ec = exp[p]
            assert np.array_equal(nn[p, :ns[p]], e12), (form, p)
            assert int(nc[p]) == len(ec) and np.array_equal(co[p, :len(ec)], ec), (form, p)
        assert not nn[e, :ns[e]].any(), form


# exact duplicates (lower, higher column): the lane halves of one tile; the two
# tiles of one step; steps s and s + 1 (different waves); steps 8 and 4 apart
# (the same wave with 8 and with 4 waves); either side of column 512
DUPS = [(70, 74), (130, 162), (200, 264), (300, 812), (330, 586), (511, 512)]


@pytest.mark.gpu
@pytest.mark.parametrize("D,twin_src", DIRS)
def test_exact_duplicate_columns_lowest_index(oracle, monkeypatch, D, twin_src):
    """1100 x 1100; each duplicated column has three rows next to it: the oracle's argmin is
    the lower copy, the two values are equal bit for bit, and no form may
    certify the higher one.  (B1 ties between lane halves, between the tiles of
    a step, between waves and within a wave.)"""
    rng = np.random.default_rng(5300 + D + twin_src)
    n, m = 1100, 1100
    A, B = _pair(rng, n, m, D)
    for i, (lo, hi) in enumerate(DUPS):
        z = rng.standard_normal(D).astype(np.float32)
        B[lo] = z
        B[hi] = z
        A[3 * i:3 * i + 3] = z + (0.3 * rng.standard_normal((3, D))).astype(np.float32)
    F, G = (B, A) if twin_src else (A, B)
    key = ("cs_dups", D, twin_src)
    (r12, c21), _ = _forms(oracle, monkeypatch, key, F[None], G[None])
    if not twin_src:
        e12 = _MEMO[key][0][0]
        for i, (lo, hi) in enumerate(DUPS):
            assert (e12[3 * i:3 * i + 3] == lo).all(), (i, e12[3 * i:3 * i + 3])
        assert r12 >= 3 * len(DUPS), r12


@pytest.mark.gpu
@pytest.mark.parametrize("D,twin_src", DIRS)
def test_near_twin_in_another_waves_step(oracle, monkeypatch, D, twin_src):
    """Twelve columns (three rows next to each) with a twin 1e-2 away exactly one step (64 columns) on:
    B1 and B2 of the rows next to them come from different waves.  The rows
    fail the 1-term certificate and are settled downstream, in every form
    alike (the counters)."""
    rng = np.random.default_rng(5400 + D + twin_src)
    n, m = 1100, 1100
    B = (3.0 * rng.standard_normal((m, D))).astype(np.float32)
    A = (B[rng.integers(0, m, n)] + 0.5 * rng.standard_normal((n, D))).astype(np.float32)
    cols = [5 + 83 * i for i in range(12)]
    for i, c in enumerate(cols):
        B[c + 64] = B[c] + (1e-2 * rng.standard_normal(D)).astype(np.float32)
        A[3 * i:3 * i + 3] = B[c] + (0.3 * rng.standard_normal((3, D))).astype(np.float32)
    F, G = (B, A) if twin_src else (A, B)
    (r12, c21), _ = _forms(oracle, monkeypatch, ("cs_twins", D, twin_src), F[None], G[None])
    if twin_src:
        assert c21 > 0, c21
    else:
        assert r12 >= 3 * len(cols), r12


@pytest.mark.gpu
@pytest.mark.parametrize("D,twin_src", DIRS)
def test_pair_with_bias_2_60_beside_finite_pairs(oracle, monkeypatch, D, twin_src):
    """Three pairs of 300 x 300, the middle one with an infinite element in the
    cloud the sweep streams as columns: its bias is 2^60, its values collapse,
    and its rows are listed -- in every form alike."""
    rng = np.random.default_rng(5500 + D + twin_src)
    prs = [_pair(rng, 300, 300, D) for _ in range(3)]
    A = np.stack([a for a, _ in prs])
    B = np.stack([b for _, b in prs])
    B[1, 200, D - 1] = np.inf
    F, G = (B, A) if twin_src else (A, B)
    fb, _ = _forms(oracle, monkeypatch, ("cs_inf", D, twin_src), F, G)
    assert fb[0] > 0 and fb[1] > 0, fb
