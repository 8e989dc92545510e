"""The threshold route of the mutual feature matching (csrc/featnn_thresh.hip):
the rows and J columns the 1-term screen (featnn_row9) cannot certify are
settled from the columns within B1 + bnd of the row's smallest screened value
(featnn_thresh9, kThreshK = 8 slots per row) by their exact f64 distances
(featnn_exact_cand); a row with more candidates goes to the exact rescan.

Bar: bit-exact -- nn12, n_corres and the correspondence list equal the
oracle's corres(featnn(F, G), featnn(G, F)), and the 3-term route
(PCR_FEAT_THRESH=0) gives identical outputs.  Shapes: counts in {1, 31, 33,
257} (one column tile and a lane short of it, one over, several row tiles and
column steps), ragged, D in {16, 17, 32}, 1 and 9 pairs (9: the p mod 8 XCD
map, and more than one column slice per row tile at a 64-wave pair); and on
every route of the driver (each PCR_FEAT_* hook, S = 3) clouds of 513 x 257 and
257 x 513 rows, which pad to different tile counts.

The CPU tests need no GPU: a numpy model of the screen's candidate sets (how
many columns fall within a row's threshold, so the twin inputs are known to
fit the slots), and the host check of the threshold's rounding helper
(tests/cpp/thresh_bits_check.cpp under -fsanitize=address,undefined)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from pointcloudregistration_amd import registration as reg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pointcloudregistration_amd", "csrc")
K_SLOTS = 8  # kThreshK (csrc/featnn_v5.h)
U = 2.0 ** -24
_MEMO = {}


def _np(t):
    return t.detach().cpu().numpy()


def _twins(rng, n, d, sep, twin_src):
    """Every target has a twin `sep` away (as test_featcorres_gpu._twins); with
    twin_src every source too."""
    a = rng.standard_normal((n, d)).astype(np.float32)
    b = (a + 0.5 * rng.standard_normal((n, d))).astype(np.float32)
    tw = (b + sep * rng.standard_normal((n, d))).astype(np.float32)
    ft = np.concatenate([b, tw])[rng.permutation(2 * n)]
    if twin_src:
        a = np.concatenate([a, (a + sep * rng.standard_normal((n, d))).astype(np.float32)])
    return a, ft


def _twin_batch(P, sep, twin_src):
    """P pairs of twins: 128 sources (256 when twinned) x 256 targets, D = 32."""
    key = ("twins", P, sep, twin_src)
    if key not in _MEMO:
        rng = np.random.default_rng(900 + P + (7 if twin_src else 0) + int(-np.log10(sep)))
        prs = [_twins(rng, 128, 32, sep, twin_src) for _ in range(P)]
        _MEMO[key] = (np.stack([a for a, _ in prs]), np.stack([b for _, b in prs]))
    return _MEMO[key]


def _candidate_counts(X, Y, headroom):
    """Per row of X: (fails, count) -- whether its 1-term top-2 gap is within
    the certificate bound, and how many columns of Y have a 1-term value within
    B1 + bnd.  The model: values |y|^2 - 2 f16(x).f16(y) in f64 on a power-of-two
    scale (max |x| in [2^(11 - headroom), 2^(12 - headroom))), bnd as bound_ct
    (csrc/featnn_v5.h) with the pair's bias B as feat_colterms chooses it."""
    X, Y = X.astype(np.float64), Y.astype(np.float64)
    D = X.shape[1]
    mx = max(np.abs(X).max(), np.abs(Y).max())
    s = 2.0 ** (11 - headroom - np.floor(np.log2(mx)))
    xs, ys = (X * s).astype(np.float32), (Y * s).astype(np.float32)
    xh, yh = xs.astype(np.float16).astype(np.float64), ys.astype(np.float16).astype(np.float64)
    sub = 2.0 ** -14 * np.sqrt(D)
    exr, eyr = np.linalg.norm(xs - xh, axis=1), np.linalg.norm(ys - yh, axis=1)
    ex, E = exr + sub, eyr.max() + sub
    q = np.linalg.norm(xs.astype(np.float64), axis=1)
    G = np.linalg.norm(ys.astype(np.float64), axis=1).max()
    M, Em = max(q.max(), G), max(exr.max(), eyr.max())
    m2 = (M * M + 4.0 * M * Em + 2.0 * Em * Em) * (1.0 + 2.0 ** -15) + 1.0
    B = 2.0 ** (np.floor(np.log2(m2)) + 1)
    Kt = 16 * ((D + 15) // 16)
    err = 2.0 * (Kt + 2) * U * ((B + G * G) + 2.0 * (q + ex) * (G + E)) + 2.0 * (ex * G + (q + ex) * E) + \
        U * (2.0 * B + G * G) + 4.0
    bnd = 2.0 * err
    v = (ys.astype(np.float64) ** 2).sum(1)[None, :] - 2.0 * xh @ yh.T
    vs = np.sort(v, axis=1)
    b1 = vs[:, 0]
    fails = (vs[:, 1] - b1 <= bnd) if v.shape[1] > 1 else np.ones(len(b1), bool)
    return fails, (v <= (b1 + bnd)[:, None]).sum(1)


TWIN_CASES = [(sep, ts) for sep in (1e-2, 1e-6) for ts in (False, True)]


@pytest.mark.parametrize("sep,twin_src", TWIN_CASES)
def test_twin_inputs_fit_the_candidate_slots(sep, twin_src):
    """CPU: on the twin inputs most rows fail the 1-term certificate and every
    row's candidate set (both directions, at the packs' scale with zero to two
    binades of headroom) fits kThreshK slots -- so on the GPU the candidates,
    not the exact rescan, decide direction 0."""
    F, G = _twin_batch(9, sep, twin_src)
    for p in range(F.shape[0]):
        for hr in (0, 1, 2):
            f12, c12 = _candidate_counts(F[p], G[p], hr)
            f21, c21 = _candidate_counts(G[p], F[p], hr)
            assert f12.mean() > 0.6, (p, hr, f12.mean())
            assert c12.max() <= K_SLOTS and c21.max() <= K_SLOTS, (p, hr, c12.max(), c21.max())
            assert c12.min() >= 1 and c21.min() >= 1


def test_thresh_bits_helper_under_sanitizers(tmp_path):
    """CPU: thresh_bits_up (csrc/featnn_thresh.h) is never below the f64
    threshold, monotone in the pattern order, and handles +inf and the largest
    finite value; a plain executable under ASan + UBSan."""
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "thresh_bits_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "thresh_bits_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok:"), r.stdout


def _expected(oracle, key, F, G, ns, nt):
    """the oracle's (nn12, correspondences) of every pair, computed once per input"""
    if key not in _MEMO:
        out = []
        for p in range(F.shape[0]):
            f, g = F[p, :ns[p]], G[p, :nt[p]]
            e12 = oracle.featnn(f, g)
            out.append((e12, oracle.corres(e12, oracle.featnn(g, f), True, 3)))
        _MEMO[key] = out
    return _MEMO[key]


def _run(F, G, ns=None, nt=None):
    co, nc, nn12 = reg.feature_correspondences(F, G, ns, nt)
    return _np(nn12), _np(nc), _np(co)


def _check(oracle, monkeypatch, key, F, G, ns=None, nt=None):
    """Both routes against the oracle, bit for bit, and against each other.
    Returns the threshold route's (fallback, rescan) counters."""
    from pointcloudregistration_amd import _lib
    P = F.shape[0]
    cs = np.full(P, F.shape[1], np.int32) if ns is None else ns
    ct = np.full(P, G.shape[1], np.int32) if nt is None else nt
    exp = _expected(oracle, key, F, G, cs, ct)
    _lib.featnn_fallback_rows(reset=True)
    _lib.featnn_rescan_rows(reset=True)
    nn, nc, co = _run(F, G, ns, nt)
    fb = _lib.featnn_fallback_rows(reset=True)
    rs = _lib.featnn_rescan_rows(reset=True)
    monkeypatch.setenv("PCR_FEAT_THRESH", "0")
    nn3, nc3, co3 = _run(F, G, ns, nt)
    monkeypatch.delenv("PCR_FEAT_THRESH")
    for p in range(P):
        e12, ec = exp[p]
        for a, b, c in ((nn, nc, co), (nn3, nc3, co3)):
            assert np.array_equal(a[p, :cs[p]], e12), p
            assert int(b[p]) == len(ec), p
            assert np.array_equal(c[p, :len(ec)], ec), p
    return fb, rs


COUNTS = {
    "a": ([257, 1, 31, 33, 257, 33, 31, 1, 257], [257, 33, 1, 31, 33, 257, 257, 31, 1]),
    "b": ([31, 33, 1, 257, 1, 257, 33, 31, 33], [31, 33, 1, 31, 257, 1, 1, 33, 257]),
}


@pytest.mark.gpu
@pytest.mark.parametrize("D,counts", [(32, "a"), (32, "b"), (16, "a"), (17, "b"), (32, None), (17, None)])
def test_random_descriptors_ragged(oracle, monkeypatch, D, counts):
    """Noisy copies of a shared code book (a few near neighbours per row: some
    rows fail the 1-term certificate), every (n_src, n_tgt) of {1, 31, 33,
    257}^2 over the two 9-pair count sets; counts None: one full pair."""
    P = 9 if counts else 1
    rng = np.random.default_rng(40 + D + P)
    code = rng.standard_normal((P, 300, D)).astype(np.float32)
    F = (np.stack([code[p, rng.permutation(300)[:257]] for p in range(P)]) +
         rng.normal(0, 0.6, (P, 257, D))).astype(np.float32)
    G = (np.stack([code[p, rng.permutation(300)[:257]] for p in range(P)]) +
         rng.normal(0, 0.6, (P, 257, D))).astype(np.float32)
    ns = nt = None
    if counts:
        ns, nt = (np.array(c, np.int32) for c in COUNTS[counts])
    _check(oracle, monkeypatch, ("random", D, counts), F, G, ns, nt)


ROUTES = {  # (D, the hook, stored chunks per image tile): every route of feature_corres_v5
    "default": (32, None, 2),
    "image_full": (32, ("PCR_FEAT_IMAGE", "full"), 5),
    "three_term_leftovers": (32, ("PCR_FEAT_THRESH", "0"), 5),
    "row8_one_term": (32, ("PCR_FEAT_ROW9", "0"), 5),
    "three_term_only": (32, ("PCR_FEAT_ONE", "0"), 5),
    "row7_s3": (48, None, 7),
}


def _unequal_sides(D, wide_src):
    """Four pairs whose clouds pad to different tile counts: per-pair counts from
    {1, 33, 513} on one side (Nmax 513: 17 row tiles, padded to 32) and {31, 65,
    257} on the other (Mmax 257: 9 tiles, padded to 16), the last pair empty on
    the wide side; wide_src: the wide side is the sources.  Noisy copies of a
    code book with a quarter of each cloud twinned 1e-2 away (rows and J
    columns the 1-term certificate fails).  Past a pair's count each cloud holds
    exact copies of the other's rows: as an argmin they would win."""
    key = ("unequal", D, wide_src)
    if key not in _MEMO:
        rng = np.random.default_rng(1700 + D + wide_src)
        P, nw, nn = 4, 513, 257
        code = rng.standard_normal((P, 560, D)).astype(np.float32)
        W = (np.stack([code[p, rng.permutation(560)[:nw]] for p in range(P)]) +
             rng.normal(0, 0.6, (P, nw, D))).astype(np.float32)
        N = (np.stack([code[p, rng.permutation(560)[:nn]] for p in range(P)]) +
             rng.normal(0, 0.6, (P, nn, D))).astype(np.float32)
        cw, cn = np.array([513, 1, 33, 0], np.int32), np.array([31, 257, 65, 100], np.int32)
        for X, c in ((W, cw), (N, cn)):
            for p in range(P):
                k = int(c[p]) // 4
                idx = rng.permutation(int(c[p]))[:2 * k]
                X[p, idx[k:]] = X[p, idx[:k]] + (1e-2 * rng.standard_normal((k, D))).astype(np.float32)
        for p in range(P):
            if cw[p] and cn[p] < nn:
                N[p, cn[p]:] = W[p, rng.integers(0, cw[p], nn - cn[p])]
            if cn[p] and cw[p] < nw:
                W[p, cw[p]:] = N[p, rng.integers(0, cn[p], nw - cw[p])]
        _MEMO[key] = (W, N, cw, cn) if wide_src else (N, W, cn, cw)
    return _MEMO[key]


@pytest.mark.gpu
@pytest.mark.parametrize("wide_src", [True, False])
@pytest.mark.parametrize("route", list(ROUTES))
def test_unequal_sides_on_every_route(oracle, monkeypatch, route, wide_src):
    """Nmax != Mmax with the two counts on different sides of a tile-padding
    boundary (513 x 257 and 257 x 513), on each route: a pass that took a
    count, a stride or a per-cloud array from the wrong side shows only here.
    nn12, n_corres and the correspondences equal the oracle's bit for bit; the
    empty pair (no sources, or no targets: index 0) is left to the other checks."""
    from pointcloudregistration_amd import _lib
    D, hook, chunks = ROUTES[route]
    F, G, ns, nt = _unequal_sides(D, wide_src)
    exp = _expected(oracle, ("unequal_oracle", D, wide_src), F[:3], G[:3], ns, nt)
    if hook:
        monkeypatch.setenv(*hook)
    nn, nc, co = _run(F, G, ns, nt)
    assert _lib.featnn_image_chunks() == chunks
    for p in range(3):
        e12, ec = exp[p]
        assert np.array_equal(nn[p, :ns[p]], e12), p
        assert int(nc[p]) == len(ec), p
        assert np.array_equal(co[p, :len(ec)], ec), p
    assert not nn[3, :ns[3]].any()


@pytest.mark.gpu
@pytest.mark.parametrize("P", [1, 9])
@pytest.mark.parametrize("sep,twin_src", TWIN_CASES)
def test_near_twins_decided_by_candidates(oracle, monkeypatch, sep, twin_src, P):
    """Near twins at separation 1e-2 and 1e-6 (targets; with twin_src sources
    too): most rows land in the threshold route (the fallback counters), and
    no row of direction 0 reaches the exact rescan -- the candidates decided
    (test_twin_inputs_fit_the_candidate_slots: every row fits its slots)."""
    F, G = _twin_batch(9, sep, twin_src)
    F, G = F[:P], G[:P]
    (r12, c21), (x12, _) = _check(oracle, monkeypatch, ("twins", sep, twin_src, P), F, G)
    assert r12 > P * F.shape[1] // 2, r12
    if twin_src:  # each J column has two sources it cannot order: more than half of J (sized by the exact argmins)
        nj = sum(len(np.unique(e12)) for e12, _ in _MEMO[("twins", sep, twin_src, P)])
        assert c21 > nj // 2, (c21, nj)
    assert x12 == 0, x12


@pytest.mark.gpu
@pytest.mark.parametrize("P", [1, 9])
def test_exact_duplicates_lowest_index(oracle, monkeypatch, P):
    """Every target (and every source) twice, bit for bit: the exact ties
    resolve to the lowest index, from the candidates (two per row)."""
    rng = np.random.default_rng(77 + P)
    a = rng.standard_normal((P, 128, 32)).astype(np.float32)
    b = (a[:, rng.permutation(128)] + 0.3 * rng.standard_normal((P, 128, 32))).astype(np.float32)
    F = np.concatenate([a, a], axis=1)[:, rng.permutation(256)]
    G = np.concatenate([b, b], axis=1)[:, rng.permutation(256)]
    (r12, c21), (x12, _) = _check(oracle, monkeypatch, ("dups", P), F, G)
    assert r12 == P * 256 and c21 > 0, (r12, c21)
    assert x12 == 0, x12


@pytest.mark.gpu
def test_more_copies_than_slots_overflow(oracle, monkeypatch):
    """kThreshK + 4 copies of one target row, and 20 sources next to it: those
    rows have more candidates than slots, go to the exact rescan (its counter)
    and still come out exact (the lowest copy)."""
    rng = np.random.default_rng(12)
    F = rng.standard_normal((1, 257, 32)).astype(np.float32)
    G = rng.standard_normal((1, 257, 32)).astype(np.float32)
    G[0, rng.permutation(257)[:K_SLOTS + 4]] = G[0, 100]
    F[0, 40:60] = G[0, 100] + (1e-3 * rng.standard_normal((20, 32))).astype(np.float32)
    _, (x12, _) = _check(oracle, monkeypatch, ("copies",), F, G)
    assert x12 >= 20, x12


@pytest.mark.gpu
def test_nonfinite_rows(oracle, monkeypatch):
    """One NaN row or one inf row in the source or the target cloud (a pair
    each, one pair with all four, one clean pair): such a pair's rows have no
    usable threshold and land in the exact rescan as before."""
    rng = np.random.default_rng(5)
    F = rng.standard_normal((6, 257, 32)).astype(np.float32)
    G = (F[:, rng.permutation(257)] + 0.4 * rng.standard_normal((6, 257, 32))).astype(np.float32)
    F[0, 70, 3] = np.nan
    F[1, 200, 31] = np.inf
    G[2, 5, 0] = np.nan
    G[3, 256, 16] = -np.inf
    F[4, 1] = np.nan
    F[4, 33, 2] = np.inf
    G[4, 31, 7] = np.nan
    G[4, 32, 8] = np.inf
    ns = np.array([257, 257, 257, 257, 257, 33], np.int32)
    nt = np.array([257, 257, 257, 257, 257, 31], np.int32)
    _check(oracle, monkeypatch, ("nonfinite",), F, G, ns, nt)


@pytest.mark.gpu
def test_pair_with_an_empty_list(oracle, monkeypatch):
    """Targets that are the sources, permuted, far from one another: every row
    and column certifies, the lists are empty (the counters stay 0) and the
    threshold kernels run over nothing -- alone, and as pair 3 of a batch whose
    other pairs are twins."""
    rng = np.random.default_rng(3)
    F = rng.standard_normal((1, 33, 32)).astype(np.float32)
    G = F[:, rng.permutation(33)].copy()
    fb, _ = _check(oracle, monkeypatch, ("empty", 1), F, G)
    assert fb == (0, 0), fb
    Ft, Gt = _twin_batch(9, 1e-2, False)
    Fb, Gb = Ft[:5].copy(), Gt[:5].copy()
    Fb[3] = rng.standard_normal((128, 32)).astype(np.float32)
    Gb[3] = np.concatenate([Fb[3], 50.0 + rng.standard_normal((128, 32)).astype(np.float32)])
    (r12, _), _ = _check(oracle, monkeypatch, ("empty", 5), Fb, Gb)
    assert r12 > 4 * 128 // 2, r12
