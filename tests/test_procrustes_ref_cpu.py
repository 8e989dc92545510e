"""CPU: the reference pair of the Procrustes / record edge tests, before any
kernel is involved.

* procrustes_ref.kabsch (numpy SVD, np.sum) against the reference's own f64
  weighted_icp outputs (tests/golden/procrustes_edges_golden.npz), at the bars
  of the GPU test: ||dR||_F <= 1e-12, ||dt|| <= 1e-12 * max(1, ||mu_s||).
* the CPU oracle (oracle.procrustes_batch on f32, oracle.procrustes_f64 on f64
  inputs) against kabsch at the same bars, and at the property bars (1e-14) for
  the inputs without a unique optimum: so the GPU bars are reachable by the
  reference pair alone.
* records_ref: the 1024-lane order equals np.sum on exactly representable
  inputs, the committed seeds tell the summation orders apart, and the
  order-free bound holds.
Origins of the bars: procrustes_ref.R_BAR / PROP_BAR.
"""
import os

import numpy as np
import pytest

import procrustes_ref as pref
import records_ref as rr

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "procrustes_edges_golden.npz")
C32 = pref.cases(np.float32)
C64 = pref.cases(np.float64)
UNIQUE32 = [k for k, v in C32.items() if v[3]]
UNIQUE64 = [k for k, v in C64.items() if v[3]]
NONUNIQUE = [k for k, v in C32.items() if not v[3]]


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def test_case_list():
    assert UNIQUE32 == [f"tail_{n}" for n in pref.TAILS] + [
        "pi_x", "pi_y", "pi_z", "pi_rand", "identity", "offset_1000", "zero_alternate",
        "negative_weights", "mixed"]
    assert UNIQUE64 == UNIQUE32[:13] + ["tiny_angle"] + UNIQUE32[13:]
    assert NONUNIQUE == ["collinear", "coincident", "zero_weights", "n_1", "n_2", "mirror_equal"]
    for name, (s, t, w, _) in C32.items():
        assert s.shape == t.shape == (pref.B, s.shape[1], 3) and w.shape == s.shape[:2], name
        assert s.dtype == t.dtype == w.dtype == np.float32


def test_named_inputs_are_what_they_claim():
    s, t, w, _ = C64["pi_x"]
    R, _, _, _, _ = pref.kabsch(s[0], t[0], w[0], 0, 1e-8)
    assert np.linalg.norm(R - np.diag([1.0, -1.0, -1.0])) < 1e-13
    assert np.array_equal(pref.half_turn((0, 0, 1)), np.diag([-1.0, -1.0, 1.0]))
    assert np.linalg.norm(pref.rot((1, 2, 3), np.pi) - pref.half_turn((1, 2, 3))) < 1e-15
    w = C32["zero_alternate"][2]
    assert np.all(w[:, 1::2] == 0) and np.all(w[:, 0::2] > 0)
    w = C32["negative_weights"][2]
    assert w.min() < -0.1 and w.max() > 0.7 and np.all(w.sum(1) > 50)
    assert np.all(C32["zero_weights"][2] == 0)
    assert np.all(C32["offset_1000"][0] > 998)
    # ranks of S: mixed = full / coplanar / mirrored, collinear = 1, mirror_equal
    # has its two weakest singular values equal
    sv = [np.linalg.svd(pref.kabsch(*[a[b] for a in C64["mixed"][:3]], 0, 1e-8)[2])[1] for b in range(3)]
    assert sv[0][2] > 1e-2 and sv[1][2] < 1e-15 < 1e-2 < sv[1][1]
    assert np.linalg.det(pref.kabsch(*[a[2] for a in C64["mixed"][:3]], 0, 1e-8)[2]) < 0
    assert sv[2][1] - sv[2][2] > 1e-2
    for b in range(3):
        S = pref.kabsch(*[a[b] for a in C64["collinear"][:3]], 0, 1e-8)[2]
        d = np.linalg.svd(S)[1]
        assert d[1] < 1e-15 * d[0]
        S = pref.kabsch(*[a[b] for a in C64["mirror_equal"][:3]], 0, 1e-8)[2]
        d = np.linalg.svd(S)[1]
        assert np.linalg.det(S) < 0 and abs(d[1] - d[2]) < 1e-15
    # coincident: S = 0 exactly only at the origin (the eps in W leaves a residue)
    S = [pref.kabsch(*[a[b] for a in C64["coincident"][:3]], 0, 1e-8)[2] for b in range(3)]
    assert not S[0].any() and S[1].any() and S[2].any()


def test_fixture_holds_the_named_inputs(gold):
    for name in UNIQUE32:
        for k, a in zip(("src", "tgt", "w"), C32[name][:3]):
            assert gold[f"{name}/{k}"].dtype == np.float32
            assert gold[f"{name}/{k}"].tobytes() == a.tobytes(), (name, k)
    assert not any(k.startswith(tuple(NONUNIQUE)) for k in gold.files)
    assert os.path.getsize(GOLD) < 512 * 1024


@pytest.mark.parametrize("name", UNIQUE32)
def test_kabsch_vs_reference_f64(gold, name):
    """kabsch on the f32 inputs widened to f64 == the reference's weighted_icp on
    the same inputs cast to f64 (absw = 0, eps = 1e-8)."""
    s, t, w, _ = C32[name]
    for b in range(pref.B):
        R, tt, _, mu_s, _ = pref.kabsch(s[b], t[b], w[b], 0, 1e-8)
        dR, dt = pref.errors_vs(np.c_[R, tt], gold[f"{name}/wicp64/R"][b], gold[f"{name}/wicp64/t"][b])
        assert dR <= pref.R_BAR and dt <= pref.t_bar(mu_s), (name, b, dR, dt)


def _oracle_T(oracle, entry, name, absw, eps):
    s, t, w, _ = (C32 if entry == "f32" else C64)[name]
    T = (oracle.procrustes_batch if entry == "f32" else oracle.procrustes_f64)(s, t, w, absw, eps)
    return s, t, w, T


@pytest.mark.parametrize("absw,eps", pref.DROPINS)
@pytest.mark.parametrize("entry", ["f32", "f64"])
def test_oracle_vs_kabsch_unique(oracle, entry, absw, eps):
    worst = (0.0, 0.0, 0.0)
    for name in (UNIQUE32 if entry == "f32" else UNIQUE64):
        s, t, w, T = _oracle_T(oracle, entry, name, absw, eps)
        for b in range(pref.B):
            R, tt, S, mu_s, _ = pref.kabsch(s[b], t[b], w[b], absw, eps)
            dR, dt = pref.errors_vs(T[b], R, tt)
            gap = pref.objective_gap(T[b, :, :3], S)
            assert dR <= pref.R_BAR and dt <= pref.t_bar(mu_s), (name, b, dR, dt)
            assert pref.orth_err(T[b, :, :3]) <= pref.PROP_BAR and abs(gap) <= pref.PROP_BAR, (name, b, gap)
            worst = (max(worst[0], dR), max(worst[1], dt / max(1.0, np.linalg.norm(mu_s))), max(worst[2], gap))
    print(f"FIG cpu-oracle {entry} absw={absw}: dR {worst[0]:.2e} dt/max(1,|mu_s|) {worst[1]:.2e} gap {worst[2]:.2e}")


@pytest.mark.parametrize("absw,eps", pref.DROPINS)
@pytest.mark.parametrize("entry", ["f32", "f64"])
@pytest.mark.parametrize("name", NONUNIQUE)
def test_oracle_nonunique_properties(oracle, name, entry, absw, eps):
    s, t, w, T = _oracle_T(oracle, entry, name, absw, eps)
    assert np.all(np.isfinite(T))
    for b in range(pref.B):
        R = T[b, :, :3]
        S = pref.kabsch(s[b], t[b], w[b], absw, eps)[2]
        assert pref.orth_err(R) <= pref.PROP_BAR
        assert abs(np.linalg.det(R) - 1.0) <= pref.PROP_BAR
        if (name, b) not in pref.GAP_UNDEFINED:
            assert abs(pref.objective_gap(R, S)) <= pref.PROP_BAR, (name, b, pref.objective_gap(R, S))


@pytest.mark.parametrize("absw,eps", pref.DROPINS)
@pytest.mark.parametrize("entry", ["f32", "f64"])
def test_oracle_exact_answers(oracle, entry, absw, eps):
    I0 = np.tile(np.c_[np.eye(3), np.zeros(3)], (pref.B, 1, 1))
    T = _oracle_T(oracle, entry, "zero_weights", absw, eps)[3]
    assert T.tobytes() == I0.tobytes()          # [I | +0] bit for bit
    s, t, w, T = _oracle_T(oracle, entry, "coincident", absw, eps)
    mu_t = pref.kabsch(s[0], t[0], w[0], absw, eps)[4]
    assert T[0, :, :3].tobytes() == np.eye(3).tobytes()
    # n same-signed terms in two orders, and W likewise: 4 n u relative (u = 2^-53)
    assert np.linalg.norm(T[0, :, 3] - mu_t) <= 4 * s.shape[1] * 2.0 ** -53 * np.linalg.norm(mu_t)
    empty = np.zeros((pref.B, 0, 3), np.float32 if entry == "f32" else np.float64)
    fn = oracle.procrustes_batch if entry == "f32" else oracle.procrustes_f64
    assert fn(empty, empty, empty[..., 0], absw, eps).tobytes() == I0.tobytes()


# ---------------------------------------------------------------------------
# records_ref
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1023, 1024, 1025, 8191, 8192, 8193, 9000])
def test_sum1024_equals_np_sum_on_exact_inputs(n):
    """Small integers: every partial sum is exact, so every order gives np.sum."""
    d = np.random.default_rng(n).integers(0, 1 << 20, (rr.P, n)).astype(np.float32)
    want = d.astype(np.int64).sum(1).astype(np.float64)
    assert np.array_equal(rr.sum1024(d), want) and np.array_equal(rr.sum256(d), want)
    assert np.array_equal(rr.sum_np(d), want)


def test_sum1024_order_by_construction():
    """2^53 + 1 + 1 rounds to 2^53 one way and 2^53 + 2 the other: pins which
    entries share a partial sum, and the order of the 16 wave totals."""
    big = np.float32(2.0 ** 53)
    d = np.zeros(2049, np.float32)
    d[0], d[1024], d[2048] = big, 1, 1             # one partial: (2^53 + 1) + 1 = 2^53
    assert rr.sum1024(d)[0] == 2.0 ** 53
    d[:] = 0
    d[2048], d[1024], d[0] = big, 1, 1             # (1 + 1) + 2^53
    assert rr.sum1024(d)[0] == 2.0 ** 53 + 2
    d[:] = 0
    d[0], d[1], d[2] = big, 1, 1                   # lanes 0, 1, 2: tree adds 1 + ... late
    # halving tree: lane 0 += lane 32 ..., lane 0 += lane 2 (h = 2), then lane 1
    # (already + lane 3) at h = 1: (2^53 + 1) + 1 = 2^53
    assert rr.sum1024(d)[0] == 2.0 ** 53
    d[:] = 0
    d[0], d[64], d[128] = big, 1, 1                # wave totals in order from 0.0
    assert rr.sum1024(d)[0] == 2.0 ** 53
    d[:] = 0
    d[128], d[0], d[64] = big, 1, 1                # (1 + 1) + 2^53
    assert rr.sum1024(d)[0] == 2.0 ** 53 + 2


@pytest.mark.parametrize("N,M", rr.SHAPES)
def test_committed_seeds_discriminate_and_hold_the_bound(N, M):
    d1, d2 = rr.distances(N, M)
    for d in (d1, d2):
        assert d.dtype == np.float32 and np.all(d >= 2.0 ** -40) and np.all(d < 2.0 ** 20)
        if d.size >= 64:                            # mantissas are full: low bits in use
            assert np.any(d.view(np.uint32) & 1) and np.any(d.view(np.uint32) & 2)
    assert rr.discriminates(d1, d2)
    if max(N, M) >= 1024:
        c = rr.chamfer_mean(d1, d2)
        assert np.any(c != rr.chamfer_mean_256(d1, d2)) and np.any(c != rr.chamfer_mean_np(d1, d2))
    # non-negative terms: a sum of n terms in ANY order is within (n - 1) u
    # relative (u = 2^-53), each division and the final addition add u; for
    # both means together that stays below (N + M) u
    ref = rr.chamfer_mean_fsum(d1, d2)
    for fn in (rr.chamfer_mean, rr.chamfer_mean_256, rr.chamfer_mean_np):
        assert np.all(np.abs(fn(d1, d2) - ref) <= (N + M) * 2.0 ** -53 * ref)
