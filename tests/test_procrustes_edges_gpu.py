"""GPU: the batched weighted Procrustes kernel (csrc/procrustes.hip) and its
drop-ins at tails, hard angles, hard conditioning and inputs without a unique
optimum -- the named inputs of tests/procrustes_ref.py, B = 3 per call.

  (a) bit for bit against the CPU oracle, f32 and f64 entries, both drop-ins'
      (abs_weights, eps), every case and N = 0;
  (b) the f32 entry against the reference's f64 weighted_icp on the same f32
      inputs (tests/golden/procrustes_edges_golden.npz);
  (c) both entries against procrustes_ref.kabsch (numpy SVD, np.sum): the one
      check descended neither from a Horn implementation nor from torch's SVD;
  (d) the drop-ins against the reference's own f32 outputs;
  (e) properties where the optimum is not unique;
  (f) N = 0 and B = 0;  (g) input validation.

Bars (origins in procrustes_ref.py): (b), (c) ||dR||_F <= 1e-12 and ||dt|| <=
1e-12 * max(1, ||mu_s||) -- the project's f64 bar (test_estimation_gpu.py), the
factor because t = mu_t - R mu_s carries dR * ||mu_s||; (d) north_star's 1e-5 on
(R, t); (e) 1e-14, one decade over the CPU oracle's measured 8e-16.
"""
import os

import numpy as np
import pytest
import torch

import procrustes_ref as pref

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "procrustes_edges_golden.npz")
C = {"f32": pref.cases(np.float32), "f64": pref.cases(np.float64)}
UNIQUE = {e: [k for k, v in C[e].items() if v[3]] for e in C}
NONUNIQUE = [k for k, v in C["f32"].items() if not v[3]]
I0 = np.tile(np.c_[np.eye(3), np.zeros(3)], (pref.B, 1, 1))


def _klass(name):
    if name.startswith("tail_"):
        return "tails"
    if name.startswith("pi_") or name in ("identity", "tiny_angle"):
        return "angles"
    return "conditioning" if name in UNIQUE["f64"] else "non-unique"


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


@pytest.fixture(scope="module")
def gpu_T():
    """The kernel's T for every (entry, case, drop-in), computed once."""
    from pointcloudregistration_amd.procrustes import procrustes_batch
    out = {}
    for entry, cs in C.items():
        for name, (s, t, w, _) in cs.items():
            for absw, eps in pref.DROPINS:
                T = procrustes_batch(torch.from_numpy(s).cuda(), torch.from_numpy(t).cuda(),
                                     torch.from_numpy(w).cuda(), absw, eps)
                assert T.dtype == torch.float64 and T.shape == (pref.B, 3, 4)
                out[entry, name, absw] = T.cpu().numpy()
    return out


def _same_bits(a, b):
    """NaN positions match; every other bit matches."""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    k = ~np.isnan(a)
    return a[k].tobytes() == b[k].tobytes()


# (a) ------------------------------------------------------------------------
@pytest.mark.parametrize("absw,eps", pref.DROPINS)
@pytest.mark.parametrize("entry", ["f32", "f64"])
def test_bitexact_vs_oracle(oracle, gpu_T, entry, absw, eps):
    fn = oracle.procrustes_batch if entry == "f32" else oracle.procrustes_f64
    for name, (s, t, w, _) in C[entry].items():
        assert _same_bits(gpu_T[entry, name, absw], fn(s, t, w, absw, eps)), name


# (b) ------------------------------------------------------------------------
def test_f32_entry_vs_reference_f64(gold, gpu_T):
    """The kernel widens f32 to f64, so the reference's weighted_icp on the same
    inputs cast to f64 solves the same problem (abs_weights = 0, eps = 1e-8)."""
    worst = {}
    for name in UNIQUE["f32"]:
        s, t, w, _ = C["f32"][name]
        for b in range(pref.B):
            mu_s = pref.kabsch(s[b], t[b], w[b], 0, 1e-8)[3]
            dR, dt = pref.errors_vs(gpu_T["f32", name, 0][b], gold[f"{name}/wicp64/R"][b],
                                    gold[f"{name}/wicp64/t"][b])
            k = worst.setdefault(_klass(name), [0.0, 0.0])
            k[0], k[1] = max(k[0], dR), max(k[1], dt / max(1.0, np.linalg.norm(mu_s)))
            assert dR <= pref.R_BAR and dt <= pref.t_bar(mu_s), (name, b, dR, dt)
    for k, v in worst.items():
        print(f"FIG gpu f32 entry vs reference f64 [{k}]: dR {v[0]:.2e} dt/max(1,|mu_s|) {v[1]:.2e}")


# (c) ------------------------------------------------------------------------
@pytest.mark.parametrize("absw,eps", pref.DROPINS)
@pytest.mark.parametrize("entry", ["f32", "f64"])
def test_vs_kabsch(gpu_T, entry, absw, eps):
    worst = {}
    for name in UNIQUE[entry]:
        s, t, w, _ = C[entry][name]
        for b in range(pref.B):
            T = gpu_T[entry, name, absw][b]
            R, tt, S, mu_s, _ = pref.kabsch(s[b], t[b], w[b], absw, eps)
            dR, dt = pref.errors_vs(T, R, tt)
            gap = pref.objective_gap(T[:, :3], S)
            k = worst.setdefault(_klass(name), [0.0, 0.0, 0.0])
            k[0], k[1] = max(k[0], dR), max(k[1], dt / max(1.0, np.linalg.norm(mu_s)))
            k[2] = max(k[2], abs(gap))
            assert dR <= pref.R_BAR and dt <= pref.t_bar(mu_s), (name, b, dR, dt)
            assert abs(gap) <= pref.PROP_BAR and pref.orth_err(T[:, :3]) <= pref.PROP_BAR, (name, b, gap)
    for k, v in worst.items():
        print(f"FIG gpu {entry} absw={absw} vs kabsch [{k}]: dR {v[0]:.2e} dt/max(1,|mu_s|) {v[1]:.2e} "
              f"gap {v[2]:.2e}")


# (d) ------------------------------------------------------------------------
def _fro(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.sqrt(((a - b) ** 2).reshape(a.shape[0], -1).sum(1)).max()


@pytest.mark.parametrize("name", UNIQUE["f32"])
def test_dropins_vs_reference_f32(gold, name):
    from pointcloudregistration_amd.procrustes import rigid_fit, weighted_icp
    s, t, w = (torch.from_numpy(gold[f"{name}/{k}"]).cuda() for k in ("src", "tgt", "w"))
    sn, tn, wn = (gold[f"{name}/{k}"] for k in ("src", "tgt", "w"))
    R, tt, moved = weighted_icp(s, t, w)
    R2, t2 = rigid_fit(s, t, w[..., None])
    assert R.dtype == tt.dtype == moved.dtype == R2.dtype == t2.dtype == torch.float32
    assert R.shape == R2.shape == (pref.B, 3, 3) and tt.shape == (pref.B, 3) and t2.shape == (pref.B, 3, 1)
    assert moved.shape == s.shape
    assert torch.all(torch.det(R.double()) > 0) and torch.all(torch.det(R2.double()) > 0)
    R, tt, moved, R2, t2 = (x.cpu().numpy() for x in (R, tt, moved, R2, t2))
    Rr, tr = gold[f"{name}/wicp32/R"], gold[f"{name}/wicp32/t"]
    Rr2, tr2 = gold[f"{name}/rfit32/R"], gold[f"{name}/rfit32/t"]
    assert tr2.shape == (pref.B, 3, 1)
    assert _fro(R, Rr) <= 1e-5 and _fro(R2, Rr2) <= 1e-5      # north_star's bar on R
    if name != "offset_1000":
        assert _fro(tt, tr) <= 1e-5 and _fro(t2, tr2) <= 1e-5  # ... and on t
        # transformed_src as test_procrustes_gpu.py holds it: 1e-4 of the
        # reference's (R, t) applied to the source
        want = np.einsum("bij,bnj->bni", Rr.astype(np.float64), sn.astype(np.float64)) + tr[:, None]
        np.testing.assert_allclose(moved, want, atol=1e-4)
    else:
        # a centroid 1000 spreads from the origin: the reference's own f32 t is
        # 2.3e-4 ... 2.8e-4 (weighted_icp) / 2.9e-4 ... 5.0e-4 (rigid_fit) from
        # the f64 answer on the same inputs, far past 1e-5, so the drop-in (f64
        # sums, one rounding of t to f32: 1.2e-9 ... 1.0e-8 / 8.9e-9 ... 1.6e-8
        # away, measured with the CPU oracle in the kernel's place) must be
        # CLOSER to the f64 answer than the reference's f32 run is.  The f64 answer:
        # the fixture's weighted_icp f64 run; for rigid_fit (|w|, eps = 1e-4,
        # which the reference cannot run in f64: it returns R as float)
        # procrustes_ref.kabsch, pinned to that fixture by the CPU test
        t64 = gold[f"{name}/wicp64/t"]
        k64 = np.stack([pref.kabsch(sn[b], tn[b], wn[b], 1, 1e-4)[1] for b in range(pref.B)])
        for b in range(pref.B):
            mine, ref = np.linalg.norm(tt[b] - t64[b]), np.linalg.norm(tr[b] - t64[b])
            mine2, ref2 = np.linalg.norm(t2[b, :, 0] - k64[b]), np.linalg.norm(tr2[b, :, 0] - k64[b])
            print(f"FIG offset t, item {b}: weighted_icp {mine:.2e} (reference f32 {ref:.2e}), "
                  f"rigid_fit {mine2:.2e} (reference f32 {ref2:.2e})")
            assert mine < ref and mine2 < ref2
        # transformed_src: outputs up to ~1733 in magnitude, where one f32 ulp
        # is 1.2e-4; against the f64 answer applied in f64, ten f32 roundings
        # (R's entries, three products, three sums, t) at that magnitude
        R64 = gold[f"{name}/wicp64/R"]
        want = np.einsum("bij,bnj->bni", R64, sn.astype(np.float64)) + t64[:, None]
        assert np.abs(moved - want).max() <= 10 * 2.0 ** -24 * np.abs(want).max()


# (e) ------------------------------------------------------------------------
@pytest.mark.parametrize("absw,eps", pref.DROPINS)
@pytest.mark.parametrize("entry", ["f32", "f64"])
@pytest.mark.parametrize("name", NONUNIQUE)
def test_nonunique_properties(gpu_T, name, entry, absw, eps):
    s, t, w, _ = C[entry][name]
    T = gpu_T[entry, name, absw]
    assert np.all(np.isfinite(T))
    worst = [0.0, 0.0, 0.0]
    for b in range(pref.B):
        R = T[b, :, :3]
        S = pref.kabsch(s[b], t[b], w[b], absw, eps)[2]
        worst[0] = max(worst[0], pref.orth_err(R))
        worst[1] = max(worst[1], abs(np.linalg.det(R) - 1.0))
        assert pref.orth_err(R) <= pref.PROP_BAR
        assert abs(np.linalg.det(R) - 1.0) <= pref.PROP_BAR
        if (name, b) not in pref.GAP_UNDEFINED:
            gap = pref.objective_gap(R, S)
            worst[2] = max(worst[2], abs(gap))
            assert abs(gap) <= pref.PROP_BAR, (name, b, gap)
    print(f"FIG gpu {entry} absw={absw} [non-unique {name}]: orth {worst[0]:.2e} det-1 {worst[1]:.2e} "
          f"gap {worst[2]:.2e}")


@pytest.mark.parametrize("absw,eps", pref.DROPINS)
@pytest.mark.parametrize("entry", ["f32", "f64"])
def test_exact_answers(gpu_T, entry, absw, eps):
    """Where the contract fixes the answer: all-zero weights make every sum zero,
    T = [I | +0] bit for bit; coincident sources at the origin with positive
    weights make S zero, R = I exactly and t = mu_t - mu_s = mu_t."""
    assert gpu_T[entry, "zero_weights", absw].tobytes() == I0.tobytes()
    s, t, w, _ = C[entry]["coincident"]
    T = gpu_T[entry, "coincident", absw]
    mu_t = pref.kabsch(s[0], t[0], w[0], absw, eps)[4]
    assert T[0, :, :3].tobytes() == np.eye(3).tobytes()
    # mu_t per coordinate: n same-signed terms q * (w_i / W) summed in two orders
    # (the kernel's 256 lanes, np.sum), each within (n - 1) u of the exact sum,
    # and W itself likewise: 4 n u relative, u = 2^-53
    assert np.linalg.norm(T[0, :, 3] - mu_t) <= 4 * s.shape[1] * 2.0 ** -53 * np.linalg.norm(mu_t)


# (f) ------------------------------------------------------------------------
@pytest.mark.parametrize("absw,eps", pref.DROPINS)
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_empty_inputs(oracle, dtype, absw, eps):
    """N = 0: no term in any sum, so every item is [I | 0] (the oracle's answer
    too); the pointers of the empty tensors are null and must be accepted.
    B = 0: an empty (0, 3, 4) result."""
    from pointcloudregistration_amd.procrustes import procrustes_batch
    e = torch.empty(pref.B, 0, 3, dtype=dtype, device="cuda")
    T = procrustes_batch(e, e, e[..., 0], absw, eps)
    assert T.shape == (pref.B, 3, 4) and T.cpu().numpy().tobytes() == I0.tobytes()
    z = np.zeros((pref.B, 0, 3), np.float32 if dtype == torch.float32 else np.float64)
    fn = oracle.procrustes_batch if dtype == torch.float32 else oracle.procrustes_f64
    assert _same_bits(T.cpu().numpy(), fn(z, z, z[..., 0], absw, eps))
    e = torch.empty(0, 7, 3, dtype=dtype, device="cuda")
    T = procrustes_batch(e, e, e[..., 0], absw, eps)
    assert T.shape == (0, 3, 4) and T.dtype == torch.float64


# (g) ------------------------------------------------------------------------
def test_input_validation():
    from pointcloudregistration_amd import _lib
    from pointcloudregistration_amd.procrustes import procrustes_batch, rigid_fit, weighted_icp
    s = torch.zeros(3, 10, 3, device="cuda")
    w = torch.ones(3, 10, device="cuda")
    for bad in (torch.zeros(3, 11, 3, device="cuda"), torch.zeros(4, 10, 3, device="cuda")):
        with pytest.raises(ValueError):
            procrustes_batch(s, bad, w, 0, 1e-8)
    with pytest.raises(ValueError):
        procrustes_batch(s[..., :2], s[..., :2], w, 0, 1e-8)
    with pytest.raises(_lib.PcrError):
        weighted_icp(s.cpu(), s.cpu(), w.cpu())
    with pytest.raises(_lib.PcrError):
        rigid_fit(s.cpu(), s.cpu(), w.cpu()[..., None])


@pytest.mark.parametrize("entry", ["f32", "f64"])
def test_noncontiguous_src_same_bits(gpu_T, entry):
    from pointcloudregistration_amd.procrustes import procrustes_batch
    s, t, w, _ = C[entry]["tail_257"]
    sv = torch.from_numpy(np.ascontiguousarray(s.transpose(0, 2, 1))).cuda().transpose(1, 2)
    assert not sv.is_contiguous() and torch.equal(sv.cpu(), torch.from_numpy(s))
    T = procrustes_batch(sv, torch.from_numpy(t).cuda(), torch.from_numpy(w).cuda(), 0, 1e-8)
    assert T.cpu().numpy().tobytes() == gpu_T[entry, "tail_257", 0].tobytes()
