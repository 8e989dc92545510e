"""f64 restatements of the pieces of one NDP loop iteration that follow the fused
MLP and the level Chamfer (include/pcr_api.h: pcr_adam_masked,
pcr_ndp_chamfer_glue / pcr_ndp_chamfer_loss, pcr_ndp_control), their derived
rounding bounds, and the case lists of tests/test_ndp_loop_gpu.py and
tests/test_ndp_warp_edges_gpu.py.  numpy only; written from the semantics
(torch's _single_tensor_adam, registration.py:231-256), not from the kernels.
tests/test_ndp_loop_ref_cpu.py pins every restatement to torch in f64 and checks
every derived bound against torch in f32; the GPU tests then stand on them.

Bounds.  One unit is u = 2^-24, the relative error of one f32 rounding; every
bound adds one subnormal ulp 2^-149 (TINY) as its absolute floor.  The count of
roundings is written next to each formula.  None of them is measured.
"""
import math

import numpy as np

U = 2.0 ** -24
TINY = 2.0 ** -149
F32 = np.float32


# --------------------------------------------------------------------------
# Adam
# --------------------------------------------------------------------------

LR, B1, B2, EPS = 0.01, 0.9, 0.999, 1e-8   # what ndp_opt._Level.step passes


def _f64(a):
    return np.asarray(a, F32).astype(np.float64)


def _param(p, m1, v1, t, lr, b1, b2, eps):
    with np.errstate(all="ignore"):
        step_size = lr / (1.0 - b1 ** t)
        denom = np.sqrt(v1) / math.sqrt(1.0 - b2 ** t) + eps
        return p - step_size * (m1 / denom)


def adam_param(p, m1, v1, t, lr=LR, b1=B1, b2=B2, eps=EPS):
    """p' of torch's _single_tensor_adam from f32 moments that are already
    updated: p - lr / (1 - b1^t) * m' / (sqrt(v') / sqrt(1 - b2^t) + eps), in f64."""
    return _param(_f64(p), _f64(m1), _f64(v1), t, lr, b1, b2, eps)


def adam_step(p, g, m, v, t, lr=LR, b1=B1, b2=B2, eps=EPS):
    """One Adam step (step count t >= 1 *after* the increment) in f64 on the f32
    inputs: (p', m', v'), p' from the unrounded m', v'."""
    g, m, v = _f64(g), _f64(m), _f64(v)
    with np.errstate(all="ignore"):
        m1 = m + (1.0 - b1) * (g - m)
        v1 = b2 * v + (1.0 - b2) * (g * g)
    return _param(_f64(p), m1, v1, t, lr, b1, b2, eps), m1, v1


def adam_bound_m(g, m):
    """m' = m + f32(1 - b1) (g - m): 4 roundings (the constant, the difference,
    the product, the sum), each of a quantity <= |m| + |g|."""
    with np.errstate(all="ignore"):
        return 4.0 * U * (np.abs(_f64(m)) + np.abs(_f64(g))) + TINY


def adam_bound_v(g, v):
    """v' = v f32(b2) + f32(1 - b2) (g g): 6 roundings (two constants, g g, two
    products, the sum), each of a quantity <= |v| + g^2."""
    with np.errstate(all="ignore"):
        return 6.0 * U * (np.abs(_f64(v)) + _f64(g) ** 2) + TINY


def adam_bound_p(p, p1):
    """p' against adam_param on the f32 moments the device (or torch f32) itself
    produced: 8 roundings of the step D = p' - p (sqrt, f32(sqrt(1 - b2^t)) and
    f32(eps), the two divisions, the eps add, the product with the step size, and
    one for f32(lr / (1 - b1^t)) whose b1^t may come from repeated multiplication
    instead of pow), plus the final sum's rounding of p'.  Counting the sum
    sqrt(v')/c + eps as the larger of its operands' errors gives 7; the 8th is
    kept for the second-order terms."""
    p, p1 = _f64(p), np.asarray(p1, np.float64)
    with np.errstate(all="ignore"):
        return 8.0 * U * np.abs(p1 - p) + U * np.abs(p1) + TINY


def error_ratio(got, want, bound):
    """max |got - want| / bound over the entries whose reference is finite as an
    f32; where the reference rounds to +-inf or is NaN the f32 result must be that
    same value (asserted).  `got` f32, `want` / `bound` f64."""
    got = np.asarray(got, F32).reshape(-1)
    want = np.asarray(want, np.float64).reshape(-1)
    bound = np.broadcast_to(np.asarray(bound, np.float64), want.shape).reshape(-1)
    with np.errstate(over="ignore"):
        w32 = want.astype(F32)
    bad = ~np.isfinite(w32)
    assert np.array_equal(got[bad], w32[bad], equal_nan=True), (got[bad], w32[bad])
    if bad.all():
        return 0.0
    ok = ~bad
    return float((np.abs(got[ok].astype(np.float64) - want[ok]) / bound[ok]).max())


ADAM_SIZES = (1, 255, 256, 257, 1025)
ADAM_STEPS = (1, 2, 3, 10, 100, 1000, 5000)
ADAM_REGIMES = ("normal1e-3", "normal1", "zero", "underflow", "overflow", "nan")


def make_adam_case(regime, n, seed=0):
    """(p, g, m, v) f32 of one tensor of n elements."""
    rng = np.random.default_rng([20250920, ADAM_REGIMES.index(regime), n, seed])
    p = rng.uniform(-1.0, 1.0, n).astype(F32)
    sc = 1e-3 if regime == "normal1e-3" else 1.0
    g = (rng.standard_normal(n) * sc).astype(F32)
    m = (rng.standard_normal(n) * sc * 0.5).astype(F32)
    v = (rng.uniform(0.25, 1.0, n) * sc * sc).astype(F32)
    if regime == "zero":          # p must not move
        g[:], m[:], v[:] = 0.0, 0.0, 0.0
    elif regime == "underflow":   # g^2 underflows: v' = 0, the denominator is eps
        g[:], m[:], v[:] = 1e-25, 0.0, 0.0
    elif regime == "overflow":    # g^2 overflows: v' = inf, the step is 0
        g[:] = np.where(rng.random(n) < 0.5, 1e25, -1e25).astype(F32)
    elif regime == "nan":         # only that element becomes NaN
        g[n // 2] = np.nan
    return p, g, m, v


def fresh_grad(n, it, seed=0):
    """The gradient of iteration `it` of the consecutive-step tests."""
    return np.random.default_rng([20250921, n, it, seed]).standard_normal(n).astype(F32)


# --------------------------------------------------------------------------
# the level loss
# --------------------------------------------------------------------------

W_REG, TRUNC = 0.05, 1e9     # NDPConfig.w_reg, the trunc of registration.py:236

# reduction shape of the two kernels: T threads per block, W wave partials, B
# block partials (0: one block)
KERNELS = {"glue": dict(T=1024, W=16, B=0), "blocks": dict(T=256, W=4, B=32)}


def sum_is_exact(terms):
    """True when every partial sum of `terms` (f32 values), in any order, is an
    f32: all terms are multiples of one power of two q and sum |term| <= 2^24 q.
    Then no addition of the reduction rounds, whatever its order."""
    t = np.abs(np.asarray(terms, np.float64).reshape(-1))
    t = t[t != 0]
    if t.size == 0:
        return True
    if not np.isfinite(t).all():
        return False
    mant, ex = np.frexp(t)
    mi = np.round(mant * 2.0 ** 24).astype(np.int64)   # exact: f32 has 24 bits
    q = (np.ldexp((mi & -mi).astype(np.float64), ex - 24)).min()
    return bool(t.sum() <= 2.0 ** 24 * q)


def sum_roundings(n, kernel):
    """Roundings on the longest path of one term through a part's sum:
    ceil(n / (T blocks)) serial adds in a thread, 6 shuffle levels, W wave
    partials, B block partials.  (The first add of each serial stage starts
    from an exact 0, so the true count is 3 less; the slack covers the
    second-order terms.)"""
    k = KERNELS[kernel]
    return -(-n // (k["T"] * max(k["B"], 1))) + 6 + k["W"] + k["B"]


def level_loss(d1, d2, s, w_reg=W_REG, trunc=TRUNC):
    """sum(d1') / K + sum(d2') / M (+ w_reg mean(-max(log(1 - s), -100))), d' = 0
    where d >= trunc (NaN stays), in f64 on the f32 inputs; 1 - s is rounded to
    f32 first and w_reg, trunc are the f32 values, as torch and the kernels have
    them.  K, M >= 1.  Returns a dict: loss; c1, c2, bce (the three parts, bce
    None without s); t1, t2, t3 (the terms, for the bound and the guard); gd1,
    gd2 (the dist-gradient seeds f32(1/K), f32(1/M) or 0 where truncated)."""
    d1, d2 = np.asarray(d1, F32).reshape(-1), np.asarray(d2, F32).reshape(-1)
    K, M = d1.size, d2.size
    tr = float(F32(trunc))
    out = dict(K=K, M=M, N=0, bce=None, t3=None)

    def part(d):
        d = d.astype(np.float64)
        with np.errstate(invalid="ignore"):
            cut = d >= tr
        return np.where(cut, 0.0, d), cut
    out["t1"], cut1 = part(d1)
    out["t2"], cut2 = part(d2)
    out["gd1"] = np.where(cut1, F32(0), F32(1.0 / K)).astype(F32)
    out["gd2"] = np.where(cut2, F32(0), F32(1.0 / M)).astype(F32)
    out["c1"], out["c2"] = out["t1"].sum() / K, out["t2"].sum() / M
    loss = out["c1"] + out["c2"]
    if s is not None:
        s = np.asarray(s, F32).reshape(-1)
        om = (F32(1.0) - s).astype(np.float64)
        with np.errstate(all="ignore"):
            out["t3"] = -np.maximum(np.log(om), -100.0)
        out["N"] = s.size
        out["w"] = float(F32(w_reg))
        with np.errstate(all="ignore"):
            out["bce"] = out["t3"].sum() / s.size
        loss = loss + out["w"] * out["bce"]
    out["loss"] = float(loss)
    return out


def loss_bound(ref, kernel):
    """|kernel loss - level_loss| for a finite loss.  Per part, sum_roundings u
    of sum |term| (0 where sum_is_exact: no addition rounds), 2 u more per BCE
    term for logf; then 4 u of |L| for the divisions, f32(w_reg)'s product and
    the final sums (3 on the longest path; |L| = the sum of the parts'
    magnitudes, which is L for the non-negative terms of every case here)."""
    b, mag = 0.0, 0.0
    for t, n in ((ref["t1"], ref["K"]), (ref["t2"], ref["M"])):
        a = np.abs(t).sum()
        mag += a / n
        if not sum_is_exact(t):
            b += sum_roundings(n, kernel) * U * a / n
    if ref["t3"] is not None:
        a, n = np.abs(ref["t3"]).sum(), ref["N"]
        mag += ref["w"] * a / n
        # -100 (the clamp) is exact; a computed log carries logf's 1 ulp = 2 u
        logs = np.abs(ref["t3"][ref["t3"] != 100.0]).sum()
        r = 0 if sum_is_exact(ref["t3"]) else sum_roundings(n, kernel)
        b += ref["w"] * (r * a + 2.0 * logs) * U / n
    return b + 4.0 * U * mag + TINY


def guard_ratios(ref):
    """{part: smallest single non-zero term / its count / the larger of the two
    kernels' bounds}: how far above the bound the loss moves when one element is
    dropped, doubled or taken from the neighbouring range."""
    bound = max(loss_bound(ref, k) for k in KERNELS)
    out = {}
    for name, t, n, w in (("d1", ref["t1"], ref["K"], 1.0), ("d2", ref["t2"], ref["M"], 1.0),
                          ("s", ref["t3"], ref["N"], ref.get("w", 0.0))):
        if t is None:
            continue
        nz = np.abs(t[t != 0])
        if nz.size:
            out[name] = float(w * nz.min() / n / bound)
    return out


LOSS_SIZES = (1, 31, 32, 33, 255, 256, 257, 1023, 1024, 1025, 8191, 8192, 8193)
LOSS_HOLD = 33
LOSS_SHAPES = tuple(dict.fromkeys(
    [(1, 1, 1)] + [(n, LOSS_HOLD, LOSS_HOLD) for n in LOSS_SIZES]
    + [(LOSS_HOLD, n, LOSS_HOLD) for n in LOSS_SIZES] + [(LOSS_HOLD, LOSS_HOLD, n) for n in LOSS_SIZES]))
# draws: every term in [0.5, 1]; trunc: a third of d truncated, half of those at
# d == trunc exactly; alltrunc: nothing left of the Chamfer part; nan: one NaN in
# d1; s_some_one: every fifth s is 1; s_all_one: every s is 1 (BCE = 100 w_reg);
# s_over: entries equal to 1 and one above 1 (NaN); nos: no BCE term
LOSS_REGIMES = ("draws", "trunc", "alltrunc", "nan", "s_some_one", "s_all_one", "s_over", "nos")
LOSS_NAN_REGIMES = ("nan", "s_over")
LOSS_SCALE = 64.0


def make_loss_case(K, M, N, regime):
    """(d1, d2, s) f32; s None for "nos".  The distances are draws from
    [0.5, 1] LOSS_SCALE on a grid of 2^-10 LOSS_SCALE: up to 2^14 of them sum
    without rounding (sum_is_exact), so the bound of a Chamfer part is the final
    divisions' alone.  With the rounding count of a rounded 8193-term sum one
    element in 8193 could not stay 100 x above the bound (the sensitivity guard):
    0.5 / 8193 of the mean against 100 x 35 u of it.  LOSS_SCALE = 64 keeps the
    BCE part's rounding (up to 45 u of a mean of 21 w_reg when a fifth of s is 1)
    below the Chamfer terms as well.  The BCE terms -log(1 - s) are draws from
    [0.5, 1] (not on a grid: a log is not)."""
    rng = np.random.default_rng([20250922, K, M, N, LOSS_REGIMES.index(regime)])

    def dist(n):
        d = ((512 + rng.integers(0, 513, n)) * (2.0 ** -10 * LOSS_SCALE)).astype(F32)
        if regime == "trunc":      # i = 1, 4, 7, ...: d == trunc, 2 trunc, d == trunc, ...
            i = np.arange(1, n, 3)
            d[i] = np.where((i // 3) % 2 == 0, F32(TRUNC), F32(2 * TRUNC))
        elif regime == "alltrunc":
            d[:] = np.where(np.arange(n) % 2 == 0, F32(TRUNC), F32(np.inf))
        return d
    d1, d2 = dist(K), dist(M)
    if regime == "nan":
        d1[K // 2] = np.nan
    if regime == "nos":
        return d1, d2, None
    s = (1.0 - np.exp(-rng.uniform(0.5, 1.0, N))).astype(F32)
    if regime == "s_some_one":
        s[::5] = 1.0
    elif regime == "s_all_one":
        s[:] = 1.0
    elif regime == "s_over":
        s[::5] = 1.0
        s[N // 2] = 1.5
    return d1, d2, s


# --------------------------------------------------------------------------
# the early-stop rule
# --------------------------------------------------------------------------

STATE0 = (1.0, 0.0, 1e6, 0.0, 0.0, 0.0, 0.0, 0.0)   # ndp_opt._Level.reset
STOP_LOSS = 1e-4
# a flat stretch, a value below stop_loss in the middle, values after the stop
# (the sequence and the pairs of test_ndp_opt_gpu.py::test_early_stop_rule_on_device)
RULE_SEQ = (0.5, 0.4999, 0.49985, 0.3, 0.29999, 0.299985, 0.2999849, 0.2, 5e-5, 0.1)
RULE_PAIRS = ((0.001, 2), (0.001, 15), (1e-6, 2))


def stop_rule(losses, ratio, max_break, stop_loss=STOP_LOSS):
    """registration.py:246-256 on float(np.float32(L)):
        if loss < stop_loss: break
        if |loss_prev - loss| < loss_prev * ratio: count += 1
        if count >= max_break: break
        loss_prev = loss; (step)
    Per iteration (step flag, (active, break_count, loss_prev, steps, last_loss,
    evaluated)): the device state words 5 and 0, 1, 2, 3, 4, 6 after it."""
    active, count, prev, steps, last, evaluated = True, 0, STATE0[2], 0, 0.0, 0
    out = []
    for L in losses:
        L = float(np.float32(L))
        flag = 0
        if active:
            evaluated += 1
            last = L
            if L < stop_loss:
                active = False
            else:
                if abs(prev - L) < prev * ratio:
                    count += 1
                if count >= max_break:
                    active = False
                else:
                    prev = L
                    steps += 1
                    flag = 1
        out.append((flag, (float(active), float(count), prev, float(steps), last, float(evaluated))))
    return out


# --------------------------------------------------------------------------
# warp cases (tests/test_ndp_warp_edges_gpu.py, tests/golden/make_ndp_loop_bounds.py)
# --------------------------------------------------------------------------

WARP_NS = (1, 31, 32, 33, 63, 65)
WARP_WIDTHS = (32, 64, 96, 128)
WARP_DEPTHS = (1, 2, 5)
WARP_OLD_XYZ, WARP_OLD_S = 1e-5, 1e-6   # what test_ndp_gpu.py asserts


def _wcase(name, N, width, depth, nr, zero_rot=None, gain=1.0):
    return dict(name=name, N=N, width=width, depth=depth, nr=tuple(nr), zero_rot=zero_rot, gain=gain)


WARP_CASES = (
    [_wcase(f"n{N}-w{W}-d{d}", N, W, d, (0, 1, 1)) for N in WARP_NS for W in WARP_WIDTHS for d in WARP_DEPTHS]
    # 16 levels: every level feeds its f32 rounding to the next through an encoding
    # of up to 2^8 x, so the branches are drawn at a quarter of the scale (at the
    # full scale the f32 mirror itself is 1.2e-5 from the oracle, above the 1e-5
    # the warp has always been held to); the cloud still moves by 0.07
    + [_wcase("cap16", 33, 128, 3, (0,) + (1,) * 15, gain=0.25),
       _wcase("nr-first", 33, 128, 3, (1, 0, 1)),      # the branch on level 0, none on level 1
       _wcase("zero-rot", 33, 128, 3, (0, 1, 1), zero_rot=1)]
)


def make_warp_case(c):
    """(levels, x): one state dict per level (level i: m = i + 1, k0 = -8), drawn
    as in test_ndp_gpu.py::test_ndp_warp_vs_oracle_configs so the warp visibly
    moves the points; x (N, 3) f32 in [-1.5, 1.5]."""
    W, depth = c["width"], c["depth"]
    rng = np.random.default_rng([20250923, WARP_CASES_INDEX[c["name"]]])
    levels = []
    for i, has_nr in enumerate(c["nr"]):
        sd = {"input.0.weight": rng.normal(0, 0.6, (W, 6)), "input.0.bias": rng.normal(0, 0.1, W)}
        for k in range(depth - 1):
            sd[f"mlp.pts_linears.{k}.weight"] = rng.normal(0, 1.5 / np.sqrt(W), (W, W))
            sd[f"mlp.pts_linears.{k}.bias"] = rng.normal(0, 0.1, W)
        for b, o in (("rot_brach", 3), ("trn_branch", 3)):
            sd[f"{b}.weight"] = rng.normal(0, 3.0, (o, W)) * c["gain"]
            sd[f"{b}.bias"] = rng.normal(0, 0.5, o) * c["gain"]
        if has_nr:
            sd["nr_branch.weight"] = rng.normal(0, 3.0, (1, W)) * c["gain"]
            sd["nr_branch.bias"] = rng.normal(0, 0.5, 1) * c["gain"]
        if c["zero_rot"] == i:      # r = 0: theta = 0, r / theta = 0 / 0
            sd["rot_brach.weight"][:], sd["rot_brach.bias"][:] = 0.0, 0.0
        levels.append({k: v.astype(F32) for k, v in sd.items()})
    x = rng.uniform(-1.5, 1.5, (c["N"], 3)).astype(F32)
    return levels, x


WARP_CASES_INDEX = {c["name"]: i for i, c in enumerate(WARP_CASES)}


def mirror_warp(levels, x):
    """The mirror pyramid (ndp_opt.NDPLayer, f32, CPU) on a case: per level
    (points (N, 3), nonrigidity (N) or None) as f32 numpy."""
    import torch
    from pointcloudregistration_amd import ndp_opt
    xt = torch.from_numpy(np.asarray(x, F32)).reshape(-1, 3)
    out = []
    with torch.no_grad():
        for i, sd in enumerate(levels):
            depth = 1 + sum(1 for k in sd if k.startswith("mlp.pts_linears.") and k.endswith(".weight"))
            L = ndp_opt.NDPLayer(depth, sd["input.0.weight"].shape[0], -8, i + 1,
                                 nonrigidity_est="nr_branch.weight" in sd)
            L.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
            xt, nr = L(xt)
            xt = xt.reshape(-1, 3)
            out.append((xt.numpy().copy(), None if nr is None else nr.reshape(-1).numpy().copy()))
    return out


def warp_errors(got, want):
    """(largest |points - oracle|, largest |nonrigidity - oracle|) over the levels
    of one case; got / want: per level (points, nonrigidity or None).  Non-finite
    values must sit where the oracle's do (asserted) and are left out."""
    ex, es = 0.0, 0.0
    for (gx, gs), (wx, ws) in zip(got, want):
        assert (gs is None) == (ws is None)
        for a, b, is_s in ((gx, wx, False),) + (((gs, ws, True),) if ws is not None else ()):
            a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
            assert a.shape == b.shape, (a.shape, b.shape)
            ok = np.isfinite(b)
            assert np.array_equal(np.isfinite(a), ok) and np.array_equal(a[~ok], b[~ok], equal_nan=True)
            e = float(np.abs(a[ok] - b[ok]).max()) if ok.any() else 0.0
            if is_s:
                es = max(es, e)
            else:
                ex = max(ex, e)
    return ex, es


def warp_bars(path):
    """(points bar, nonrigidity bar) of the GPU test: 4 x the pooled floors
    recorded in ndp_loop_bounds.npz."""
    z = np.load(path)
    return 4.0 * float(z["floor_xyz"]), 4.0 * float(z["floor_s"])
