"""CPU: tests/ndp_ldmk_ref.py pinned to torch -- the restatement against f64
autograd, every derived bound against torch in f32 (the reference's own
expression, registration.py:218-221), the stated f32 gradient formula against
torch's f32 autograd bit for bit, and the sensitivity guard of every case the GPU
test runs."""
import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

import ndp_ldmk_ref as ref
import ndp_loop_ref as loop


def _torch_loss(x, t, d1, d2, s, w_cd, dtype, trunc=loop.TRUNC, w_reg=loop.W_REG):
    """registration.py:218-221, 240-244 on the distances (the truncation of
    loss.py: torch.where(d >= trunc, 0, d), sums over the full lengths)."""
    x = torch.from_numpy(np.asarray(x)).to(dtype).requires_grad_(True)
    t = torch.from_numpy(np.asarray(t)).to(dtype)
    loss = torch.mean(torch.sum((x - t) ** 2, dim=-1))
    if d1 is not None:
        cd = 0.0
        for d in (d1, d2):
            d = torch.from_numpy(d).to(dtype)
            d = torch.where(d >= torch.tensor(np.float32(trunc)).to(dtype), torch.zeros_like(d), d)
            cd = cd + d.sum() / d.numel()
        loss = loss + (float(np.float32(w_cd)) if dtype == torch.float64 else w_cd) * cd
    if s is not None:
        # 1 - s is an f32 quantity in the restatement (as the kernels and torch f32 have it)
        p = 1.0 - (torch.from_numpy(np.float32(1.0) - s).to(dtype)) if dtype == torch.float64 \
            else torch.from_numpy(s)
        w = float(np.float32(w_reg)) if dtype == torch.float64 else w_reg
        loss = loss + w * Fn.binary_cross_entropy(p, torch.zeros_like(p))
    return loss, x


def _draws(L, seed):
    rng = np.random.default_rng([7, L, seed])
    return (rng.uniform(-1, 1, (L, 3)).astype(np.float32), rng.uniform(-1, 1, (L, 3)).astype(np.float32))


@pytest.mark.parametrize("L", ref.LDMK_SIZES)
def test_restatement_is_torch_f64(L):
    for x, t in (_draws(L, 0), ref.make_ldmk(L)):
        loss, xt = _torch_loss(x, t, None, None, None, 0.0, torch.float64)
        (g,) = torch.autograd.grad(loss, xt)
        want = ref.ldmk_loss(x, t)
        assert abs(float(loss.detach()) - want) <= 1e-13 * abs(want)
        g64 = ref.ldmk_grad64(x, t)
        assert np.abs(g.numpy() - g64).max() <= 1e-14 * np.abs(g64).max()
        # the f32 formula is the f64 gradient to two roundings and f32(2 / L)
        assert np.all(np.abs(ref.ldmk_grad32(x, t) - g64) <= 3 * ref.U * np.abs(g64) + ref.TINY)


@pytest.mark.parametrize("L", ref.LDMK_SIZES + (2, 3, 97, 1000))
def test_gradient_formula_is_torch_f32_autograd_bit_for_bit(L):
    for seed in range(3):
        x, t = _draws(L, seed)
        loss, xt = _torch_loss(x, t, None, None, None, 0.0, torch.float32)
        (g,) = torch.autograd.grad(loss, xt)
        assert g.numpy().tobytes() == ref.ldmk_grad32(x, t).tobytes(), (L, seed)


@pytest.mark.parametrize("mode", ["A", "B"])
@pytest.mark.parametrize("regime", [r for r in ref.REGIMES if r != "nan"])
def test_composed_loss_and_bounds_against_torch(mode, regime):
    worst = 0.0
    for L in ref.LDMK_SIZES:
        for w_cd in ref.W_CDS:
            x, t, d1, d2, s = ref.make_case(L, mode, regime)
            want = ref.level_loss(x, t, d1, d2, s, w_cd)
            l64, _ = _torch_loss(x, t, d1, d2, s, w_cd, torch.float64)
            assert abs(float(l64.detach()) - want["loss"]) <= 1e-12 * abs(want["loss"]), (L, w_cd)
            l32, _ = _torch_loss(x, t, d1, d2, s, w_cd, torch.float32)
            bound = ref.loss_bound(want, x, t)
            worst = max(worst, abs(float(l32.detach()) - want["loss"]) / bound)
            assert abs(float(l32.detach()) - want["loss"]) <= bound, (L, w_cd, float(l32.detach()), want["loss"], bound)
            if regime == "alltrunc":
                assert want["loss"] == want["ldmk"]
            # the guard: one landmark dropped or doubled moves the loss >= 100 bounds
            assert ref.terms_exact(x, t) and loop.sum_is_exact(want["terms"])
            assert ref.guard_ratio(want, x, t) >= ref.GUARD_MIN, (L, w_cd, ref.guard_ratio(want, x, t))
            if L > 1:
                drop = ref.level_loss(x[1:], t[1:], d1, d2, s, w_cd)
                # (the mean's divisor changes too; the term itself must show)
                moved = abs(drop["ldmk"] * (L - 1) / L - want["ldmk"])
                assert moved >= ref.GUARD_MIN * bound
    print(f"ldmk loss {mode} {regime}: torch f32 error / bound {worst:.3f}")


def test_rounded_terms_bound_against_torch_f32():
    """Draws off the grid: every difference, square and add rounds; the f32 result
    of torch stays within the 8 u + sum_roundings u bound."""
    worst = 0.0
    for L in ref.LDMK_SIZES:
        for seed in range(4):
            x, t = _draws(L, seed)
            want = ref.level_loss(x, t, None, None, None, 0.0)
            assert not ref.terms_exact(x, t)
            l32, _ = _torch_loss(x, t, None, None, None, 0.0, torch.float32)
            bound = ref.loss_bound(want, x, t)
            worst = max(worst, abs(float(l32.detach()) - want["loss"]) / bound)
            assert abs(float(l32.detach()) - want["loss"]) <= bound
    print(f"ldmk loss, rounded terms: torch f32 error / bound {worst:.3f}")


def test_nan_landmark_gives_nan():
    x, t, d1, d2, s = ref.make_case(33, "A", "nan")
    assert np.isnan(ref.level_loss(x, t, d1, d2, s, 0.5)["loss"])


def test_compose_g():
    x, t = _draws(5, 0)
    xo = np.concatenate([x, _draws(4, 1)[0]])
    gsub = _draws(4, 2)[0]
    g = ref.compose_g(xo, t, gsub, 0.3)
    assert g[:5].tobytes() == ref.ldmk_grad32(x, t).tobytes()
    assert g[5:].tobytes() == (gsub * np.float32(0.3)).tobytes()
    assert not ref.compose_g(xo, t, None, 0.3)[5:].any()
