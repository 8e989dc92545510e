"""numpy f64 restatement of the pcr_pointwise_forward contract (include/pcr_api.h)
in the REFERENCE's form -- subtract, concatenate, Conv1d(k=1), GroupNorm,
activation, residual add, max over points (ROPNet/src/models/CG.py:15-106,
TFMR.py:76-130) -- with a derived error bound per stage.  Inputs are f32 arrays
taken as exact; everything is f64; clouds are channel-major (B, C, N).  The
layer, the statistics and the normalisation are tests/groupmlp_ref.py's
(imported, not copied): the kernels share the rule.

Stages, each checked from the call's own previous one (y, stats, out, max).

Operand.  row[c] = src[c] - sub[c] is ONE rounded f32 subtraction where a sub is
given (a copy, exact, where not): e_row = u |src - sub|.  The concatenation
copies.

Product.  y = W row over n = cin inputs.  For n <= 4095 it is groupmlp_ref.layer
with its constant (n + 2) u (unary_ref's argument: g_n <= (n + 1) u  <=>
n (n + 1) u <= 1).  cin reaches 4608 here (and 6144 in the reference's unsplit
decoder layer), past that argument, so for n > 4095 the bound uses the exact
constant of an n-term f32 dot product in any order, g_n = n u / (1 - n u)
(Higham, Accuracy and Stability, Lemma 3.1 and (3.4)), which already holds the
second order, plus u for the products u e_in:

  e_y = |W| e_in + (g_n + u) |W| (|row| + e_in) + n 2^-149

test_pointwise_cpu checks g_n <= (n + 1) u up to 4095, its failure at 4096 and
(1 + u)^n - 1 <= g_n at the widths used, in exact rational arithmetic.

Biases.  t = (y + bias) + cbias: each one rounded f32 add (exact where its
result is subnormal): e <- e + u (|t| + e).

Statistics.  groupmlp_ref.moments_bound over the n points x gw channels of a
(cloud, group): m = n gw values.

Norm and activation.  groupmlp_ref.norm_act with the call's slope (slope 1: the
identity, for a call without activation; that adds one rounding the kernel does
not make, which only widens the bound).  Without a norm pre = t and the
activation is 1-Lipschitz for |slope| <= 1, its product one rounding where
slope is neither 0 nor 1: e <- e + u (|out| + e) + 2^-149.

Residual.  out = z + res AFTER the activation (TFMR.py:104-105), one rounded
add, res known to e_res: e <- (e + e_res) + u (|out| + e + e_res).

Max.  Exact in any order and 1-Lipschitz: from the call's own out it is met bit
for bit; end to end its bound is the largest of its members'.

No constant here is fitted to a result.
"""
import numpy as np

from groupmlp_ref import D, SUB, U, f64, layer, moments, moments_bound, norm_act, ratio  # noqa: F401

N_FIRST_ORDER = 4095    # the largest n with g_n <= (n + 1) u


def gamma_n(n):
    return n * U / (1 - n * U)


def operand(sources, subs=None):
    """(row (B, cin, N) f64, e_row): sources side by side, each minus its sub where one is given."""
    subs = [None] * len(sources) if subs is None else subs
    rows, errs = [], []
    for s, u in zip(sources, subs):
        if u is None:
            rows.append(f64(s))
            errs.append(np.zeros(np.shape(s)))
        else:
            d = f64(s) - f64(u)
            rows.append(d)
            errs.append(U * np.abs(d))
    return np.concatenate(rows, axis=1), np.concatenate(errs, axis=1)


def product(w, row, e_in=None):
    """w (cout, cin), row (B, cin, N) known to e_in -> (y (B, cout, N), bound)."""
    w = f64(w)
    n = w.shape[1]
    h = np.swapaxes(f64(row), 1, 2)
    e = np.zeros_like(h) if e_in is None else np.swapaxes(np.broadcast_to(f64(e_in), row.shape), 1, 2)
    if n <= N_FIRST_ORDER:
        y, b = layer(w, h, e)
    else:
        aw = np.abs(w).T
        y = h @ w.T
        b = e @ aw + (gamma_n(n) + U) * ((np.abs(h) + e) @ aw) + n * SUB
    return np.swapaxes(y, 1, 2), np.swapaxes(b, 1, 2)


def add_bias(y, e, bias=None, cbias=None, e_cbias=0.0):
    """t = (y + bias[o]) + cbias[b][o] and its bound; cbias known to e_cbias (B, cout)."""
    t, e = f64(y), np.broadcast_to(f64(e), np.shape(y))
    if bias is not None:
        t = t + f64(bias)[None, :, None]
        e = e + U * (np.abs(t) + e)
    if cbias is not None:
        t = t + f64(cbias)[:, :, None]
        e = e + np.broadcast_to(f64(e_cbias), np.shape(cbias))[:, :, None]
        e = e + U * (np.abs(t) + e)
    return t, e


def stats(t, gw):
    """t (B, cout, N) -> (mean, var) (B, cout // gw) and their bounds for t exact."""
    out = [[], [], [], []]
    for tb in f64(t):
        m, v = moments(tb.T, gw)
        em, ev = moments_bound(tb.T, 0.0, gw)
        for lst, a in zip(out, (m, v, em, ev)):
            lst.append(a)
    return tuple(np.stack(a) for a in out)


def finish(t, e, gw=0, gamma=None, beta=None, eps=1e-5, act=False, slope=0.0, res=None, e_res=0.0):
    """t (B, cout, N) known to e -> (out, bound) through norm, activation and residual."""
    if abs(slope) > 1:
        raise ValueError("pointwise_ref: the activation bound needs |slope| <= 1")
    t = f64(t)
    e = np.broadcast_to(f64(e), t.shape)
    s = slope if act else 1.0
    if gw:
        z, e_z = np.empty_like(t), np.empty_like(t)
        for b in range(t.shape[0]):
            zb, eb = norm_act(t[b].T, e[b].T, gamma, beta, eps, s, gw)
            z[b], e_z[b] = zb.T, eb.T
    else:
        z = np.where(t > 0, t, s * t)
        e_z = e if s in (0.0, 1.0) else e + U * (np.abs(z) + e) + SUB
    if res is not None:
        z = z + f64(res)
        e_z = e_z + e_res
        e_z = e_z + U * (np.abs(z) + e_z)
    return z, e_z


def pointwise(sources, w, subs=None, bias=None, cbias=None, gw=0, gamma=None, beta=None, eps=1e-5, act=False,
              slope=0.0, res=None, e_in=None, e_cbias=0.0):
    """End to end from exact inputs (or sources known to e_in (B, cin, N)): dict of out, bound, y, e_y, max, e_max."""
    row, e_row = operand(sources, subs)
    if e_in is not None:
        e_row = e_row + e_in + U * e_in
    y, e_y = product(w, row, e_row)
    t, e_t = add_bias(y, e_y, bias, cbias, e_cbias)
    out, e_out = finish(t, e_t, gw, gamma, beta, eps, act, slope, res)
    r = dict(out=out, bound=e_out, y=y, e_y=e_y)
    if out.shape[2]:
        r["max"], r["e_max"] = out.max(2), e_out.max(2)
    return r


# ---- the reference's modules, stage by stage ---------------------------------------------

def backbone(layers, x, e_in=None, first=None):
    """A PointNet backbone from x (B, C, N): layers = [dict(w, bias, gw, gamma, beta, eps, act, slope)].
    first: (w, cbias, e_cbias) for the first layer instead of its own weight and bias (the CG's split
    decoder layer, whose bias is inside cbias).  Returns [(out, bound)] per layer, the bound carried
    from the input."""
    outs, e = [], e_in
    for i, L in enumerate(layers):
        if i == 0 and first is not None:
            L = dict(L, w=first[0], bias=None)
        r = pointwise([x], L["w"], bias=L.get("bias"), cbias=first[1] if i == 0 and first is not None else None,
                      e_cbias=first[2] if i == 0 and first is not None else 0.0, gw=L.get("gw", 0),
                      gamma=L.get("gamma"), beta=L.get("beta"), eps=L.get("eps", 1e-5), act=L.get("act", False),
                      slope=L.get("slope", 0.0), e_in=e)
        x, e = r["out"], r["bound"]
        outs.append((x, e))
    return outs
