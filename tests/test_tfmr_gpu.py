"""GPU: pcr_similarity_topk / pcr_tfmr_select and the matching module against the
CPU restatement of the contract (tests/tfmr_ref.py) -- bit for bit, since the
f32 MFMA computes the contract's fmaf chain -- and against what the reference's
TFMRModule.forward returned (tests/golden/tfmr_golden.npz) under the rules of
tests/test_tfmr_cpu.py."""
import functools
import os

import numpy as np
import pytest
import torch

import tfmr_ref as tr
from pointcloudregistration_amd import matching

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, "tests", "golden", "tfmr_golden.npz"))
F32 = np.float32

# (B, N1, M1, C, k): one lane / one tile / tile edges on every axis, odd C, C not a
# multiple of 4 (scalar staging), more than one source and target tile (128),
# every k instantiation (1, 2, 3, 8), C = 960 and 1024 (30 and 32 chunks)
SHAPES = [(1, 1, 1, 1, 1), (3, 5, 3, 2, 3), (1, 31, 33, 3, 1), (2, 32, 32, 32, 3), (1, 33, 31, 33, 8),
          (2, 65, 257, 191, 3), (1, 64, 65, 960, 3), (2, 129, 131, 64, 1), (1, 40, 70, 1024, 2)]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def top_prob_for(n_keep, N1):
    return 1.0 if n_keep == N1 else (n_keep + 0.5) / N1


def run_gpu(fx, fy, tgt, k, n_keep):
    """Every output of the two entries through the module, as numpy."""
    B, N1, _ = fx.shape
    src = torch.arange(B * N1 * 3, dtype=torch.float32, device="cuda").view(B, N1, 3)
    x_ol = torch.arange(B * N1, dtype=torch.float32, device="cuda").view(B, N1)
    p = top_prob_for(n_keep, N1)
    assert int(p * N1) == n_keep
    val, idx = matching.similarity_topk(fx, fy, k)
    s, corr, icp, sel, det = matching.tfmr_match(fx, fy, src, tgt, x_ol, p, k, return_details=True)
    torch.cuda.synchronize()
    bi = torch.arange(B, device="cuda")[:, None]
    assert torch.equal(s, src[bi, sel]) and torch.equal(icp, x_ol[bi, sel])
    assert sel.dtype == torch.int64 and idx.dtype == torch.int64
    return dict(val=val.cpu().numpy(), idx=idx.cpu().numpy(), sel=sel.cpu().numpy(),
                w=det["weights"].cpu().numpy(), tgt_corr=corr.cpu().numpy(),
                idx_keep=det["idx"].cpu().numpy())


def assert_bit_equal(got, want, what=""):
    for key in ("val", "idx", "sel", "idx_keep", "w", "tgt_corr"):
        assert got[key].shape == want[key].shape, (what, key, got[key].shape, want[key].shape)
        assert np.array_equal(bits(got[key]), bits(want[key].astype(got[key].dtype))), (what, key)


def check(fx, fy, tgt, k, n_keeps, what=""):
    S = tr.chain(fx, fy)
    dfx, dfy, dtgt = dev(fx), dev(fy), dev(tgt)
    for n_keep in n_keeps:
        assert_bit_equal(run_gpu(dfx, dfy, dtgt, k, n_keep), tr.restate(fx, fy, tgt, k, n_keep, S=S),
                         f"{what} n_keep={n_keep}")


@functools.lru_cache(maxsize=None)
def shape_case(shape):
    B, N1, M1, C, k = shape
    fx, fy, _, tgt, _ = tr.prepare(tr.make_case(B, N1, M1, C, (11,) + shape))
    return fx, fy, tgt


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_bit_equal_to_the_restatement(shape):
    B, N1, M1, C, k = shape
    fx, fy, tgt = shape_case(shape)
    check(fx, fy, tgt, k, sorted({0, 1, int(0.4 * N1), N1}), str(shape))


@pytest.mark.parametrize("k", [4, 5, 6, 7])
def test_remaining_k(k):
    """k = 4 has its own sweep; 5 .. 7 run the 8-entry one and keep the first k."""
    fx, fy, tgt = shape_case((1, 20, 140, 12, 8))
    check(fx, fy, tgt, k, (8,), f"k={k}")


@pytest.mark.parametrize("name", sorted(tr.GOLDEN_CASES))
def test_golden_reference_outputs(name):
    """tfmr_correspondences on the raw inputs (its own normalise / sort / gather)
    against the reference's stored outputs: indices and icp_weights exact,
    tgt_corr within the recorded spread."""
    B, N1, M1, C, k, p = tr.GOLDEN_CASES[name]
    c = {n: dev(v) for n, v in tr.golden_case(name).items()}
    src, corr, icp, inds = matching.tfmr_correspondences(
        c["f_x_attn"], c["f_y_attn"], c["src"], c["tgt"], c["x_ol_score"], c["y_ol_score"], N1, M1, p, k)
    torch.cuda.synchronize()
    assert np.array_equal(inds.cpu().numpy(), G[f"{name}/similarity_max_inds"].astype(np.int64))
    assert icp.cpu().numpy().tobytes() == G[f"{name}/icp_weights"].tobytes()
    spread = float(G[f"{name}/spread"])
    err = float(np.abs(G[f"{name}/tgt_corr"].astype(np.float64) - corr.cpu().numpy()).max())
    assert err <= spread < 1e-6
    assert tuple(src.shape) == (B, int(p * N1), 3)


def float_case(B, N1, M1, C, seed):
    """General f32 features (not the generator's integer rows), normalised."""
    rng = np.random.default_rng(seed)
    fx = rng.standard_normal((B, N1, C)).astype(F32)
    fy = rng.standard_normal((B, M1, C)).astype(F32)
    fx /= np.linalg.norm(fx, axis=-1, keepdims=True).astype(F32)
    fy /= np.linalg.norm(fy, axis=-1, keepdims=True).astype(F32)
    return fx, fy, rng.uniform(-1, 1, (B, M1, 3)).astype(F32)


def test_duplicated_targets_tie_to_the_lowest_index():
    fx, fy, tgt = float_case(2, 70, 150, 40, 1)
    fy[:, 75:] = fy[:, :75]          # every target twice: exact ties, 75 apart (across tiles too)
    check(fx, fy, tgt, 3, (28, 70), "dup targets")
    r = run_gpu(dev(fx), dev(fy), dev(tgt), 2, 70)
    assert (r["val"][..., 0] == r["val"][..., 1]).all() and (r["idx"][..., 0] < r["idx"][..., 1]).all()


def test_all_targets_identical():
    fx, fy, tgt = float_case(1, 37, 140, 24, 2)
    fy[:] = fy[:, :1]
    check(fx, fy, tgt, 3, (14, 37), "identical targets")
    r = run_gpu(dev(fx), dev(fy), dev(tgt), 3, 37)
    assert (r["idx"] == np.arange(3)).all()


def test_duplicated_sources_cut_by_n_keep():
    fx, fy, tgt = float_case(2, 66, 90, 32, 3)
    best = tr.topk(tr.chain(fx, fy), 1)[0][..., 0].argmax(-1)       # each batch's most confident row
    for b in range(2):
        fx[b, 10:40] = fx[b, best[b]]                                # a tie group of >= 30 rows at the top
    check(fx, fy, tgt, 2, (1, 7, 29, 30, 31, 66), "dup sources")


def test_zero_source_row():
    fx, fy, tgt = float_case(1, 40, 50, 16, 4)
    fx[0, 7] = 0.0
    fx[0, 8] = -0.0
    check(fx, fy, tgt, 3, (40,), "zero row")
    r = run_gpu(dev(fx), dev(fy), dev(tgt), 3, 40)
    for row in (7, 8):
        at = int(np.where(r["sel"][0] == row)[0][0])
        assert r["idx"][0, row].tolist() == [0, 1, 2] and (bits(r["val"][0, row]) == 0).all()
        assert (r["w"][0, at] == 0).all() and (r["tgt_corr"][0, at] == 0).all()


def test_all_negative_similarities():
    fx, fy, tgt = float_case(2, 45, 67, 20, 5)
    check(np.abs(fx), -np.abs(fy), tgt, 3, (18, 45), "negative")


@pytest.mark.parametrize("scale", [1e-3, 1e3])
def test_scaled_features(scale):
    fx, fy, tgt = float_case(1, 50, 60, 48, 6)
    check((fx * F32(scale)).astype(F32), fy, tgt, 3, (20, 50), f"scale {scale}")


def test_subnormal_products_are_not_flushed():
    fx, fy, tgt = float_case(1, 34, 45, 64, 7)
    fx, fy = (fx * F32(8) * F32(1e-22)).astype(F32), (fy * F32(8) * F32(1e-22)).astype(F32)
    S = tr.chain(fx, fy)
    tiny = np.finfo(F32).tiny
    assert (np.abs(S) < tiny).all() and (S != 0).mean() > 0.9      # all subnormal, hardly any zero
    check(fx, fy, tgt, 3, (13, 34), "subnormal")


def test_non_finite_features_stay_in_range():
    fx, fy, tgt = float_case(2, 70, 140, 36, 8)
    fx[0, 5] = np.nan
    fy[1, 9, 3] = np.inf
    fx[1, 11, 3] = -1.0
    for k in (1, 3, 8):
        r = run_gpu(dev(fx), dev(fy), dev(tgt), k, 40)
        assert r["idx"].min() >= 0 and r["idx"].max() < 140
        assert r["idx_keep"].min() >= 0 and r["idx_keep"].max() < 140
        assert r["sel"].min() >= 0 and r["sel"].max() < 70
        assert all(len(set(row.tolist())) == 40 for row in r["sel"])


def test_correspondences_equal_match_on_their_own_tensors():
    rng = np.random.default_rng(9)
    B, N, M, C, N1, M1, k, p = 2, 80, 90, 40, 64, 70, 3, 0.6
    fxa, fya = dev(rng.standard_normal((B, N, C)).astype(F32)), dev(rng.standard_normal((B, M, C)).astype(F32))
    src, tgt = dev(rng.uniform(-1, 1, (B, N, 3)).astype(F32)), dev(rng.uniform(-1, 1, (B, M, 3)).astype(F32))
    xs = dev((rng.integers(0, 20, (B, N)) / 20).astype(F32))       # ties: the stable order decides
    ys = dev((rng.integers(0, 20, (B, M)) / 20).astype(F32))
    got = matching.tfmr_correspondences(fxa, fya, src, tgt, xs, ys, N1, M1, p, k)
    fxn = fxa / (torch.norm(fxa, dim=-1, keepdim=True) + 1e-8)
    fyn = fya / (torch.norm(fya, dim=-1, keepdim=True) + 1e-8)
    xi = torch.from_numpy(np.argsort(-xs.cpu().numpy(), axis=-1, kind="stable")).cuda()
    yi = torch.from_numpy(np.argsort(-ys.cpu().numpy(), axis=-1, kind="stable")).cuda()[:, :M1]
    bi = torch.arange(B, device="cuda")[:, None]
    want = matching.tfmr_match(fxn[bi, xi[:, :N1]], fyn[bi, yi], src[bi, xi[:, :N1]], tgt[bi, yi],
                               xs[bi, xi], p, k)
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    assert tuple(got[0].shape) == (B, int(p * N1), 3)


def test_non_contiguous_inputs_and_side_stream():
    fx, fy, tgt = float_case(2, 70, 150, 40, 10)
    want = run_gpu(dev(fx), dev(fy), dev(tgt), 3, 28)
    wide = lambda a: dev(np.repeat(a, 2, axis=-1))[..., ::2]   # noqa: E731  stride 2 along the last axis
    nfx, nfy, ntgt = wide(fx), wide(fy), dev(np.repeat(tgt, 2, axis=1))[:, ::2]
    assert not nfx.is_contiguous() and not ntgt.is_contiguous()
    assert_bit_equal(run_gpu(nfx, nfy, ntgt, 3, 28), want, "non-contiguous")
    dfx, dfy, dtgt = dev(fx), dev(fy), dev(tgt)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        got = run_gpu(dfx, dfy, dtgt, 3, 28)
    assert_bit_equal(got, want, "side stream")


def dense_reference(fx, fy, tgt, k, n_keep):
    """TFMR.py:226-254 as the reference writes it (dense tensors)."""
    B = fx.shape[0]
    S = torch.bmm(fx, fy.permute(0, 2, 1).contiguous())
    inds = torch.sort(S.max(dim=-1)[0], dim=-1, descending=True)[1][:, :n_keep]
    bi = torch.arange(B, device=fx.device)[:, None]
    Sg = S[bi, inds]
    ti = torch.topk(Sg, k=k, dim=-1)[1]
    mask = torch.zeros_like(Sg).scatter_(-1, ti, 1.0).detach()
    Sm = Sg * mask
    w = Sm / (torch.sum(Sm, dim=-1, keepdim=True) + 1e-8)
    return torch.bmm(w, tgt), inds


def test_gradient_mode():
    B, N1, M1, C, k, p = 2, 33, 35, 64, 3, 0.6
    fx, fy, tgt = float_case(B, N1, M1, C, 12)
    n_keep = int(p * N1)

    def grads(fn, fx_t, fy_t, tgt_t):
        fx_t, fy_t = fx_t.clone().requires_grad_(True), fy_t.clone().requires_grad_(True)
        corr, inds = fn(fx_t, fy_t, tgt_t)
        corr.sum().backward()
        return fx_t.grad.double().cpu(), fy_t.grad.double().cpu(), inds.cpu()

    gx64, gy64, i64 = grads(lambda a, b, t: dense_reference(a, b, t, k, n_keep),
                            torch.from_numpy(fx).double(), torch.from_numpy(fy).double(),
                            torch.from_numpy(tgt).double())
    gx32, gy32, i32 = grads(lambda a, b, t: dense_reference(a, b, t, k, n_keep), dev(fx), dev(fy), dev(tgt))
    src = torch.zeros(B, N1, 3, device="cuda")
    x_ol = torch.zeros(B, N1, device="cuda")

    def ours(a, b, t):
        out = matching.tfmr_match(a, b, src, t, x_ol, p, k)
        assert out[1].requires_grad and out[1].grad_fn is not None      # took the torch re-evaluation
        return out[1], out[3]

    gx, gy, isel = grads(ours, dev(fx), dev(fy), dev(tgt))
    assert torch.equal(isel, i64) and torch.equal(i32, i64)             # no near tie: one selection
    ex32, ey32 = float((gx32 - gx64).abs().max()), float((gy32 - gy64).abs().max())
    ex, ey = float((gx - gx64).abs().max()), float((gy - gy64).abs().max())
    print(f"grad error fx {ex:.3e} (dense f32 {ex32:.3e})  fy {ey:.3e} (dense f32 {ey32:.3e})")
    assert ex <= 4 * ex32 and ey <= 4 * ey32
    # without grad the kernels' values come back, and they carry no graph
    with torch.no_grad():
        out = matching.tfmr_match(dev(fx).requires_grad_(True), dev(fy), src, dev(tgt), x_ol, p, k)
    assert not out[1].requires_grad
    plain = matching.tfmr_match(dev(fx), dev(fy), src, dev(tgt), x_ol, p, k)
    assert not plain[1].requires_grad and torch.equal(plain[1], out[1])
    with pytest.raises(RuntimeError, match="forward-only"):
        matching.similarity_topk(dev(fx).requires_grad_(True), dev(fy), k)


def test_cpu_tensors_raise():
    fx, fy, tgt = (torch.from_numpy(a) for a in float_case(1, 8, 9, 4, 13))
    with pytest.raises(ValueError, match="no CPU path"):
        matching.similarity_topk(fx, fy, 1)
    with pytest.raises(ValueError, match="no CPU path"):
        matching.tfmr_match(fx, fy, torch.zeros(1, 8, 3), tgt, torch.zeros(1, 8), 0.5, 1)
    with pytest.raises(ValueError, match="k=9"):
        matching.similarity_topk(fx.cuda(), fy.cuda(), 9)
