"""CPU: the f64 restatements of tests/ndp_loop_ref.py (Adam step, level loss,
early-stop rule) against torch in f64 to 1e-13, their derived rounding bounds
against torch in f32 (a bound torch's own f32 arithmetic breaks is a wrong
count, not a wrong torch), the sensitivity guard of every loss case, the case
lists, and the recorded f32 floor of the warp (tests/golden/
ndp_loop_bounds.npz) -- so a wrong bound, a blunt case or a stale bounds file
is caught without a GPU."""
import os

import numpy as np
import pytest
import torch

import ndp_loop_ref as ref

BOUNDS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ndp_loop_bounds.npz")


# --------------------------------------------------------------------------
# Adam
# --------------------------------------------------------------------------

def _torch_adam(p, dtype, state=None):
    pt = torch.nn.Parameter(torch.from_numpy(p).to(dtype).clone())   # from_numpy shares memory
    opt = torch.optim.Adam([pt], lr=ref.LR, betas=(ref.B1, ref.B2), eps=ref.EPS, foreach=False)
    if state is not None:
        t, m, v = state
        opt.state[pt] = {"step": torch.tensor(float(t)), "exp_avg": torch.from_numpy(m).to(dtype).clone(),
                         "exp_avg_sq": torch.from_numpy(v).to(dtype).clone()}
    return pt, opt


def _close(a, b):
    """1e-13 of the tensor's largest entry (both sides f64; m' cancels near 0)."""
    assert np.abs(a - b).max() <= 1e-13 * np.abs(b).max(), np.abs(a - b).max() / np.abs(b).max()


def test_adam_step_matches_torch_f64():
    """Twenty steps of torch.optim.Adam(foreach=False) in f64 from a fresh state,
    fresh gradients each step, against adam_step iterated on its own f64 state."""
    n = 257
    rng = np.random.default_rng(11)
    p0 = rng.uniform(-1.0, 1.0, n).astype(np.float32)
    pt, opt = _torch_adam(p0, torch.float64)
    p, m, v = p0.astype(np.float64), np.zeros(n), np.zeros(n)
    for t in range(1, 21):
        g = ref.fresh_grad(n, t)
        pt.grad = torch.from_numpy(g).double()
        opt.step()
        # adam_step takes f32 inputs; iterate the same formulas on the f64 state
        m = m + (1.0 - ref.B1) * (g.astype(np.float64) - m)
        v = ref.B2 * v + (1.0 - ref.B2) * g.astype(np.float64) ** 2
        p = ref._param(p, m, v, t, ref.LR, ref.B1, ref.B2, ref.EPS)
        st = opt.state[pt]
        _close(st["exp_avg"].numpy(), m)
        _close(st["exp_avg_sq"].numpy(), v)
        _close(pt.detach().numpy(), p)
        if t == 1:  # and the public functions, on f32 inputs, are those formulas
            p1, m1, v1 = ref.adam_step(p0, g, np.zeros(n, np.float32), np.zeros(n, np.float32), 1)
            _close(p1, p)
            _close(m1, m)
            _close(v1, v)
            m32, v32 = m.astype(np.float32), v.astype(np.float32)
            want = ref._param(p0.astype(np.float64), m32.astype(np.float64), v32.astype(np.float64), 1,
                              ref.LR, ref.B1, ref.B2, ref.EPS)
            assert np.array_equal(ref.adam_param(p0, m32, v32, 1), want)


@pytest.mark.parametrize("regime", ref.ADAM_REGIMES)
def test_adam_bounds_hold_for_torch_f32(regime):
    """torch f32 Adam, seeded for every t with the case's f32 state, stays inside
    the derived bounds: m', v' of adam_step, p' of adam_param on torch's own f32
    m', v'.  Non-finite values sit where the f32-rounded reference has them."""
    worst = {"m": 0.0, "v": 0.0, "p": 0.0}
    for n in ref.ADAM_SIZES:
        p, g, m, v = ref.make_adam_case(regime, n)
        for t in ref.ADAM_STEPS:
            pt, opt = _torch_adam(p, torch.float32, (t - 1, m, v))
            pt.grad = torch.from_numpy(g)
            opt.step()
            st = opt.state[pt]
            assert float(st["step"]) == t
            m1, v1, p1 = st["exp_avg"].numpy(), st["exp_avg_sq"].numpy(), pt.detach().numpy()
            _, wm, wv = ref.adam_step(p, g, m, v, t)
            wp = ref.adam_param(p, m1, v1, t)
            worst["m"] = max(worst["m"], ref.error_ratio(m1, wm, ref.adam_bound_m(g, m)))
            worst["v"] = max(worst["v"], ref.error_ratio(v1, wv, ref.adam_bound_v(g, v)))
            worst["p"] = max(worst["p"], ref.error_ratio(p1, wp, ref.adam_bound_p(p, wp)))
            if regime in ("zero", "overflow"):
                assert np.array_equal(p1, p)
            if regime == "nan":
                assert np.isnan(p1).sum() == 1 and np.isnan(p1[n // 2])
    print(f"torch f32 / bound, {regime}: {worst}")
    assert max(worst.values()) <= 1.0, worst


def test_adam_case_list_is_the_issue_list():
    assert ref.ADAM_SIZES == (1, 255, 256, 257, 1025) and ref.ADAM_STEPS == (1, 2, 3, 10, 100, 1000, 5000)
    assert ref.ADAM_REGIMES == ("normal1e-3", "normal1", "zero", "underflow", "overflow", "nan")
    f = np.float32
    p, g, m, v = ref.make_adam_case("zero", 257)
    assert not g.any() and not m.any() and not v.any() and p.any()
    p, g, m, v = ref.make_adam_case("underflow", 257)
    assert (g == f(1e-25)).all() and (g * g == 0).all() and not m.any() and not v.any()
    p, g, m, v = ref.make_adam_case("overflow", 257)
    assert (np.abs(g) == f(1e25)).all() and np.isinf(g * g).all()
    p, g, m, v = ref.make_adam_case("nan", 257)
    assert np.isnan(g).sum() == 1 and np.isnan(g[128])
    for r, sc in (("normal1e-3", 1e-3), ("normal1", 1.0)):
        p, g, m, v = ref.make_adam_case(r, 1025)
        assert 0.8 * sc < g.std() < 1.2 * sc and np.isfinite(g).all() and (v > 0).all()


# --------------------------------------------------------------------------
# the level loss
# --------------------------------------------------------------------------

def _torch_loss(d1, d2, s, dtype):
    """registration.py:231-244 in torch; 1 - s in f32 whatever the dtype."""
    w = float(np.float32(ref.W_REG))
    a, b = torch.from_numpy(d1).to(dtype), torch.from_numpy(d2).to(dtype)
    loss = torch.where(a >= ref.TRUNC, torch.zeros_like(a), a).mean() + \
        torch.where(b >= ref.TRUNC, torch.zeros_like(b), b).mean()
    if s is not None:
        om = (1 - torch.from_numpy(s)).to(dtype)
        loss = loss + w * torch.mean(-torch.clamp(torch.log(om), min=-100.0))
    return float(loss)


LOSS_CASES = [(K, M, N, r) for (K, M, N) in ref.LOSS_SHAPES for r in ref.LOSS_REGIMES]


@pytest.mark.parametrize("regime", ref.LOSS_REGIMES)
def test_level_loss_matches_torch(regime):
    """f64 torch to 1e-13; f32 torch inside the derived bound of either kernel."""
    worst = 0.0
    for K, M, N in ref.LOSS_SHAPES:
        d1, d2, s = ref.make_loss_case(K, M, N, regime)
        out = ref.level_loss(d1, d2, s)
        want = _torch_loss(d1, d2, s, torch.float64)
        got32 = _torch_loss(d1, d2, s, torch.float32)
        if regime in ref.LOSS_NAN_REGIMES:
            assert np.isnan(out["loss"]) and np.isnan(want) and np.isnan(got32)
            continue
        assert abs(out["loss"] - want) <= 1e-13 * abs(want), (K, M, N, out["loss"], want)
        bound = min(ref.loss_bound(out, k) for k in ref.KERNELS)
        worst = max(worst, abs(got32 - out["loss"]) / bound)
        # the seeds are torch's gradient of the mean, 0 where truncated
        assert np.array_equal(out["gd1"], np.where(d1 >= np.float32(ref.TRUNC), 0, np.float32(1.0 / K)).astype(np.float32))
        assert np.array_equal(out["gd2"], np.where(d2 >= np.float32(ref.TRUNC), 0, np.float32(1.0 / M)).astype(np.float32))
        if regime == "s_all_one":
            assert out["bce"] == 100.0
        if regime == "alltrunc":
            assert out["c1"] == 0.0 and out["c2"] == 0.0
        if regime == "nos":
            assert out["bce"] is None and out["loss"] == out["c1"] + out["c2"]
    print(f"torch f32 / bound, {regime}: {worst:.3f}")
    assert worst <= 1.0


def test_level_loss_nan_and_clamp_edges():
    f = np.float32
    d = np.array([1.0, 2.0], f)
    # NaN in d stays (NaN >= trunc is false); its seed is 1/K like any kept term
    out = ref.level_loss(np.array([1.0, np.nan], f), d, None)
    assert np.isnan(out["loss"]) and np.array_equal(out["gd1"], np.full(2, 0.5, f))
    # d == trunc is truncated, the f32 below it is not
    below = np.nextafter(f(ref.TRUNC), f(0))
    out = ref.level_loss(np.array([ref.TRUNC, below], f), d, None)
    assert out["c1"] == float(below) / 2 and np.array_equal(out["gd1"], np.array([0, 0.5], f))
    # s == 1: exactly -100; s > 1: NaN survives the clamp; 1 - s in f32: s = 2^-30 is 0
    assert ref.level_loss(d, d, np.array([1.0], f))["bce"] == 100.0
    assert np.isnan(ref.level_loss(d, d, np.array([0.5, 1.5], f))["loss"])
    assert ref.level_loss(d, d, np.array([2.0 ** -30], f))["bce"] == 0.0


@pytest.mark.parametrize("K,M,N,regime", LOSS_CASES)
def test_sensitivity_guard(K, M, N, regime):
    """One kept Chamfer term over its count is >= 100 x the case's bound (the
    larger of the two kernels'): an element dropped, doubled or taken from the
    neighbouring range cannot hide.  With every s equal to 1 the same holds for
    one BCE term as far as the issue's own count allows: it stays above the
    bound at every N (25 x at N = 8193)."""
    if regime in ref.LOSS_NAN_REGIMES:
        return
    out = ref.level_loss(*ref.make_loss_case(K, M, N, regime))
    r = ref.guard_ratios(out)
    assert ("d1" in r) == ("d2" in r) == (regime != "alltrunc")
    for part in ("d1", "d2"):
        if part in r:
            assert r[part] >= 100.0, (part, r)
    if regime == "s_all_one":
        assert r["s"] > 1.0, r
    # the distances sum without rounding: the bound of those parts is the divisions'
    assert ref.sum_is_exact(out["t1"]) and ref.sum_is_exact(out["t2"])


def test_sum_is_exact():
    f = np.float32
    assert ref.sum_is_exact(np.full(2 ** 14, 1.0 - 2.0 ** -10, f))
    assert not ref.sum_is_exact(np.full(2 ** 15, 1.0 - 2.0 ** -10, f))      # 2^15 > 2^24 2^-10
    assert not ref.sum_is_exact(np.array([1.0, 2.0 ** -24], f))             # 1 + 2^-24 is no f32
    assert ref.sum_is_exact(np.array([1.0, 2.0 ** -23], f))
    assert ref.sum_is_exact(np.full(8193, 100.0, f)) and ref.sum_is_exact(np.zeros(3, f))
    assert not ref.sum_is_exact(np.array([1.0, np.nan], f))
    # and f32 addition agrees: any order of an exact set gives the f64 sum
    rng = np.random.default_rng(0)
    d, _, _ = ref.make_loss_case(8193, 1, 1, "draws")
    for _ in range(3):
        acc = f(0)
        for x in rng.permutation(d):
            acc = f(acc + x)
        assert float(acc) == d.astype(np.float64).sum()


def test_loss_case_list_is_the_issue_list():
    assert ref.LOSS_SIZES == (1, 31, 32, 33, 255, 256, 257, 1023, 1024, 1025, 8191, 8192, 8193)
    want = {(1, 1, 1)}
    for n in ref.LOSS_SIZES:
        want |= {(n, 33, 33), (33, n, 33), (33, 33, n)}
    assert set(ref.LOSS_SHAPES) == want and len(ref.LOSS_SHAPES) == len(want) == 38
    tr = np.float32(ref.TRUNC)
    for K, M, N in ref.LOSS_SHAPES:
        d1, d2, s = ref.make_loss_case(K, M, N, "draws")
        assert (d1.size, d2.size, s.size) == (K, M, N)
        for d in (d1, d2):
            assert (d >= 0.5 * ref.LOSS_SCALE).all() and (d <= ref.LOSS_SCALE).all()
        t = -np.log(1.0 - s.astype(np.float64))
        assert (t > 0.49).all() and (t < 1.01).all()
        d1, d2, s = ref.make_loss_case(K, M, N, "trunc")
        for d in (d1, d2):
            if d.size >= 2:
                assert (d == tr).any() and (d < tr).any()
            if d.size >= 5:
                assert (d > tr).any()
        d1, d2, s = ref.make_loss_case(K, M, N, "alltrunc")
        assert (d1 >= tr).all() and (d2 >= tr).all() and (d1 == tr).any()
        d1, d2, s = ref.make_loss_case(K, M, N, "nan")
        assert np.isnan(d1).sum() == 1 and np.isfinite(d2).all()
        assert (ref.make_loss_case(K, M, N, "s_all_one")[2] == 1).all()
        s = ref.make_loss_case(K, M, N, "s_some_one")[2]
        assert (s == 1).any() and (s <= 1).all()
        s = ref.make_loss_case(K, M, N, "s_over")[2]
        assert (s > 1).sum() == 1 and (N < 6 or (s == 1).any())
        assert ref.make_loss_case(K, M, N, "nos")[2] is None
    assert [ref.sum_roundings(8193, k) for k in ("glue", "blocks")] == [9 + 6 + 16, 2 + 6 + 4 + 32]
    assert [ref.sum_roundings(1, k) for k in ("glue", "blocks")] == [1 + 6 + 16, 1 + 6 + 4 + 32]


# --------------------------------------------------------------------------
# the early-stop rule
# --------------------------------------------------------------------------

def _host_loop(seq, ratio, mb):
    """The host restatement test_ndp_opt_gpu.py::test_early_stop_rule_on_device inlines."""
    host, bc, prev, alive = [], 0, 1e6, True
    for L in seq:
        L = float(np.float32(L))
        if not alive:
            host.append(0)
            continue
        if L < 1e-4:
            alive = False
            host.append(0)
            continue
        if abs(prev - L) < prev * ratio:
            bc += 1
        if bc >= mb:
            alive = False
            host.append(0)
            continue
        prev = L
        host.append(1)
    return host


def test_stop_rule_reproduces_the_host_loop():
    assert ref.RULE_SEQ == (0.5, 0.4999, 0.49985, 0.3, 0.29999, 0.299985, 0.2999849, 0.2, 5e-5, 0.1)
    assert ref.RULE_PAIRS == ((0.001, 2), (0.001, 15), (1e-6, 2))
    flags = {}
    for ratio, mb in ref.RULE_PAIRS:
        out = ref.stop_rule(ref.RULE_SEQ, ratio, mb)
        flags[(ratio, mb)] = [f for f, _ in out]
        assert flags[(ratio, mb)] == _host_loop(ref.RULE_SEQ, ratio, mb)
        steps = 0
        for i, (f, (active, count, prev, st, last, ev)) in enumerate(out):
            steps += f
            assert st == steps and (f == 0 or active == 1.0)
            if f:
                assert prev == last == float(np.float32(ref.RULE_SEQ[i])) and ev == i + 1
        assert out[-1][1][0] == 0.0           # every pair stops within the sequence
        stop = out[-1][1][5]                  # ... and nothing after the stop is evaluated
        assert stop < len(ref.RULE_SEQ) and out[-1][1] == out[int(stop) - 1][1]
    # the sequence has the three ways through the rule: the flat stretch stops the
    # first pair early, the value below stop_loss stops the second, the 1e-7 step
    # counts once for the third before stop_loss ends it
    assert flags[(0.001, 2)] == [1, 1, 0, 0, 0, 0, 0, 0, 0, 0]
    assert flags[(0.001, 15)] == [1, 1, 1, 1, 1, 1, 1, 1, 0, 0]
    assert flags[(1e-6, 2)] == [1, 1, 1, 1, 1, 1, 1, 1, 0, 0]
    assert ref.stop_rule(ref.RULE_SEQ, 1e-6, 2)[6][1][1] == 1.0


# --------------------------------------------------------------------------
# the warp cases and their recorded floor
# --------------------------------------------------------------------------

def test_warp_case_list_is_the_issue_list():
    by = {c["name"]: c for c in ref.WARP_CASES}
    assert len(by) == len(ref.WARP_CASES) == 6 * 4 * 3 + 3
    assert {(c["N"], c["width"], c["depth"]) for c in ref.WARP_CASES[:72]} == \
        {(N, W, d) for N in (1, 31, 32, 33, 63, 65) for W in (32, 64, 96, 128) for d in (1, 2, 5)}
    assert all(c["nr"] == (0, 1, 1) and c["zero_rot"] is None and c["gain"] == 1.0 for c in ref.WARP_CASES[:72])
    c = by["cap16"]
    assert (c["N"], c["width"], c["depth"], len(c["nr"])) == (33, 128, 3, 16)
    assert by["nr-first"]["nr"] == (1, 0, 1) and by["zero-rot"]["zero_rot"] == 1
    levels, x = ref.make_warp_case(by["zero-rot"])
    assert not levels[1]["rot_brach.weight"].any() and not levels[1]["rot_brach.bias"].any()
    assert "nr_branch.weight" in ref.make_warp_case(by["nr-first"])[0][0]


def test_warp_floor_is_reproduced_and_not_looser_than_before(oracle):
    """The committed floors are what the f32 mirror gives here (pooled over the
    case list, a factor 4 either way: the largest error moves with the BLAS), the
    file has every case, and the bars the GPU test takes from it (4 x the pooled
    floor) are not looser than the 1e-5 / 1e-6 test_ndp_gpu.py asserts."""
    z = np.load(BOUNDS)
    assert set(z.files) == {c["name"] for c in ref.WARP_CASES} | {"floor_xyz", "floor_s"}
    now = []
    for c in ref.WARP_CASES:
        levels, x = ref.make_warp_case(c)
        y, data = oracle.ndp_warp(levels, x)
        finite = np.isfinite(y).all(1)
        assert c["zero_rot"] is not None or (finite.all() and np.abs(y - x).max() > 1e-3)
        now.append(ref.warp_errors(ref.mirror_warp(levels, x), [data[i] for i in range(len(levels))]))
        assert np.isfinite(z[c["name"]]).all()
    for key, cur in (("floor_xyz", max(e[0] for e in now)), ("floor_s", max(e[1] for e in now))):
        rec = float(z[key])
        assert rec == max(float(z[c["name"]][int(key == "floor_s")]) for c in ref.WARP_CASES)
        assert cur <= 4 * rec and rec <= 4 * cur, (key, rec, cur)
    bx, bs = ref.warp_bars(BOUNDS)
    assert 0 < bx <= ref.WARP_OLD_XYZ and 0 < bs <= ref.WARP_OLD_S
    assert (ref.WARP_OLD_XYZ, ref.WARP_OLD_S) == (1e-5, 1e-6)
