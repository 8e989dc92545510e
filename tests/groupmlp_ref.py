"""numpy f64 restatement of the pcr_edge_conv / pcr_group_mlp contracts
(include/pcr_api.h) in the REFERENCE's form -- Wa f_i + Wb (f_j - f_i) for the
edge conv, conv -> norm -> activation -> max for the MLP -- with a derived error
bound per stage.  Inputs are f32 arrays taken as exact; everything is f64.

The restatement is in stages because a bound carried through every layer has
few teeth (it multiplies through |W| and through 1 / sqrt(var)); the entries
return every stage boundary (R|Q, y_l, mean/var) so that a test checks each
stage from the call's own previous one.  u = 2^-24 (f32), d = 2^-53 (f64).

Layer.  y[o] = sum_c W[o][c] h[c], in the kernel one fmaf chain of n links over
c ascending from +0, with an input known to e_in:

  e_y = |W| e_in + (n + 2) u |W| (|h| + e_in) + n 2^-149

  n u     n roundings, each at most u of a partial sum that |W| |h| dominates
  2       1 for the second order of (1 + u)^n - 1 <= n u (1 + n u), n <= 512,
          1 for the products u e_in the first term leaves out
  2^-149  a link with a subnormal result loses absolute accuracy
(the form of pointnet_ref.layer without a bias).  Any f32 dot product of n terms,
in any order, keeps this bound.

Edge conv.  P = Wa f_i and Q = Wb f_i are layers (e_P, e_Q).  R = P - Q is one
rounded subtraction: e_R = e_P + e_Q + u (|P - Q| + e_P + e_Q).  y = R_i + Q_j is
one rounded add: e_y = e_R + e_Q + u (|y| + e_R + e_Q) (an f32 add with a
subnormal result is exact).  The reference's form W [f_i ; f_j - f_i] rounds
f_j - f_i first and is a 2c-term dot product: the same bound covers it with
n = 2 c + 1 (test_groupmlp_cpu checks the golden against it).

Statistics of m values y known to e (per channel m = rows, per group of 32
channels m = 32 rows).  The kernel adds the f32 values and their exact f64
squares in f64, m - 1 roundings each, and divides:
  e_mean = mean(e) + (m + 2) d mean|y|
  e_var  = 2 sqrt(var) rms(e) + rms(e)^2 + 3 (m + 4) d mean(y^2)
The first terms are the values' own errors: |mean(y + e) - mean(y)| <= mean(e),
and for the centred second moment |var' - var| <= 2 sqrt(var) rms(e) + rms(e)^2
(Cauchy-Schwarz on mean((y - mu) de) plus mean(de^2); centring only lowers
it).  The d terms: S / m carries (m + 1) d mean|y|; S2 / m carries (m + 1) d
mean(y^2); mean^2 carries 2 |mean| e_mean' + d mean^2 <= (2 m + 5) d mean(y^2)
as |mean| mean|y| <= mean(y^2); the subtraction d mean(y^2): (3 m + 7) d
mean(y^2) in all, rounded up to 3 (m + 4) for the second order.

Normalise and activate.  a* = gamma rstd, b* = beta - mean a*, rstd = (var +
eps)^-1/2.  The kernel's rstd is off by the relative r = e_var / (2 (var + eps -
e_var)) + 4 d (first order of the -1/2 power with the worst denominator; sqrt,
divide and the product with gamma in f64), a and b are rounded once to f32:
  e_a = |a*| (r + u (1 + r))
  e_b = t + u (|b*| + t),  t = |a*| e_mean (1 + r) + |mean a*| r + 4 d (|beta| + |mean a*|)
  pre = fmaf(y, a, b):  e_pre = (|y| + e) e_a + |a*| e + e_b, then one rounding:
  e_pre' = e_pre + u (|y a* + b*| + e_pre) + 2^-149
act is 1-Lipschitz for |slope| <= 1; the slope's product is one more rounding
u (|h| + e_pre') where slope != 0.  With slope = 0 a unit whose pre + e_pre' < 0
is +0 exactly.  The max over the neighbours is exact and 1-Lipschitz: its bound
is the largest of its members' bounds (and the kernel's act(fmaf(max y, a, b))
IS the max of its activated values, bit for bit: both maps are monotone).

No constant here is fitted to a result.
"""
import numpy as np

U = 2.0 ** -24
D = 2.0 ** -53
SUB = 2.0 ** -149
C_LAYER = 2


def f64(a):
    return np.asarray(a, np.float64)


def ratio(got, want, bound):
    """max |got - want| / bound over every element; an element whose bound is 0 (a unit that is
    certainly dead) must be met exactly."""
    diff = np.abs(f64(got) - f64(want))
    bound = np.broadcast_to(f64(bound), diff.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bound > 0, diff / bound, np.where(diff == 0, 0.0, np.inf))
    return float(r.max()) if r.size else 0.0


def layer(w, h, e_in=None, n=None):
    """w (out, n), h (..., n) -> (y (..., out), bound)."""
    w, h = f64(w), f64(h)
    n = w.shape[1] if n is None else n
    e = np.zeros_like(h) if e_in is None else f64(e_in)
    aw = np.abs(w).T
    return h @ w.T, e @ aw + (n + C_LAYER) * U * ((np.abs(h) + e) @ aw) + n * SUB


def act(v, slope):
    return np.where(v > 0, v, slope * v)


def moments(y, group=1):
    """y (rows, c) of one cloud -> mean, var (c // group,), two-pass in f64."""
    rows, c = y.shape
    yy = f64(y).reshape(rows, c // group, group)
    mean = yy.mean((0, 2))
    return mean, ((yy - mean[None, :, None]) ** 2).mean((0, 2))


def moments_bound(y, e, group=1):
    """(e_mean, e_var) (c // group,) of the kernel's statistics of y (rows, c) known to e."""
    rows, c = y.shape
    m = rows * group
    yy = f64(y).reshape(rows, c // group, group)
    ee = np.broadcast_to(f64(e), y.shape).reshape(rows, c // group, group)
    _, var = moments(y, group)
    rms = np.sqrt((ee * ee).mean((0, 2)))
    e_mean = ee.mean((0, 2)) + (m + 2) * D * np.abs(yy).mean((0, 2))
    e_var = 2 * np.sqrt(var) * rms + rms * rms + 3 * (m + 4) * D * (yy * yy).mean((0, 2))
    return e_mean, e_var


def norm_act(y, e, gamma, beta, eps, slope, group=1):
    """y (rows, c) of one cloud known to e -> (h*, e_h), both (rows, c)."""
    if abs(slope) > 1:
        raise ValueError("groupmlp_ref: the activation bound needs |slope| <= 1")
    y = f64(y)
    rows, c = y.shape
    e = np.broadcast_to(f64(e), y.shape)
    mean, var = moments(y, group)
    e_mean, e_var = moments_bound(y, e, group)
    if not (e_var < var + eps).all():
        raise ValueError("groupmlp_ref: the variance's bound reaches var + eps")
    r = e_var / (2 * (var + eps - e_var)) + 4 * D
    mean, var, e_mean, r = (np.repeat(v, group) for v in (mean, var, e_mean, r))
    gamma = np.ones(c) if gamma is None else f64(gamma)
    beta = np.zeros(c) if beta is None else f64(beta)
    a = gamma / np.sqrt(var + eps)
    b = beta - mean * a
    e_a = np.abs(a) * (r + U * (1 + r))
    t = np.abs(a) * e_mean * (1 + r) + np.abs(mean * a) * r + 4 * D * (np.abs(beta) + np.abs(mean * a))
    e_b = t + U * (np.abs(b) + t)
    pre = y * a + b
    e_pre = (np.abs(y) + e) * e_a + np.abs(a) * e + e_b
    e_pre = e_pre + U * (np.abs(pre) + e_pre) + SUB
    h = act(pre, slope)
    if slope == 0:
        return h, np.where(pre + e_pre < 0, 0.0, e_pre)
    return h, e_pre + U * (np.abs(h) + e_pre)


# ---- edge conv ---------------------------------------------------------------------------

def edge_rq(w, f, e_f=None):
    """w (co, 2c), f (n, c) known to e_f -> R, Q, e_R, e_Q (n, co)."""
    c = f.shape[1]
    w = f64(w)
    p, e_p = layer(w[:, :c], f, e_f)
    q, e_q = layer(w[:, c:], f, e_f)
    r = p - q
    return r, q, e_p + e_q + U * (np.abs(r) + e_p + e_q), e_q


def edge_y(r, q, idx, e_r=0.0, e_q=0.0):
    """y (n, kk, co) = R_i + Q_j and its bound, for R, Q known to e_r, e_q."""
    r, q = f64(r), f64(q)
    y = r[:, None, :] + q[idx]
    e = np.broadcast_to(f64(e_r), r.shape)[:, None, :] + np.broadcast_to(f64(e_q), q.shape)[idx]
    return y, e + U * (np.abs(y) + e)


def edge_y_reference(w, f, idx):
    """The reference's form: W [f_i ; f_j - f_i] (n, kk, co)."""
    w, f = f64(w), f64(f)
    c = f.shape[1]
    return (f @ w[:, :c].T)[:, None, :] + (f[idx] - f[:, None, :]) @ w[:, c:].T


def pool(h, e):
    """max over axis 1 of h (n, k, c) with the largest member bound."""
    return h.max(1), e.max(1)


def edge_out(y, e, eps, slope):
    """y (n, kk, co) known to e -> out (n, co), bound."""
    n, kk, co = y.shape
    h, e_h = norm_act(y.reshape(n * kk, co), np.broadcast_to(f64(e), y.shape).reshape(n * kk, co), None, None, eps,
                      slope)
    return pool(h.reshape(n, kk, co), e_h.reshape(n, kk, co))


def edge_conv(w, f, idx, eps=1e-5, slope=0.2, e_f=None):
    """One cloud end to end from f (n, c) known to e_f (None: exact): (out (n, co), carried bound)."""
    r, q, e_r, e_q = edge_rq(w, f, e_f)
    y, e = edge_y(r, q, idx, e_r, e_q)
    return edge_out(y, e, eps, slope)


# ---- grouped MLP -------------------------------------------------------------------------

def mlp_next(w, y, e, gamma, beta, eps, slope, group):
    """y_l (n, K, c_l) known to e -> (y_{l+1}, bound) through norm, activation and the layer w."""
    n, k, c = y.shape
    h, e_h = norm_act(f64(y).reshape(n * k, c), np.broadcast_to(f64(e), y.shape).reshape(n * k, c), gamma, beta,
                      eps, slope, group)
    y2, e2 = layer(w, h, e_h)
    return y2.reshape(n, k, -1), e2.reshape(n, k, -1)


def mlp_out(y, e, gamma, beta, eps, slope, group):
    """Last layer's y (n, K, c) known to e -> (out (n, c), bound)."""
    n, k, c = y.shape
    h, e_h = norm_act(f64(y).reshape(n * k, c), np.broadcast_to(f64(e), y.shape).reshape(n * k, c), gamma, beta,
                      eps, slope, group)
    return pool(h.reshape(n, k, c), e_h.reshape(n, k, c))


def group_mlp(x, weights, gammas=None, betas=None, eps=1e-5, slope=0.0, group=1):
    """One cloud end to end from exact x (n, K, cin): (out (n, c_L), carried bound, [y_l])."""
    nl = len(weights)
    gammas = gammas or [None] * nl
    betas = betas or [None] * nl
    n, k, cin = x.shape
    y, e = layer(weights[0], f64(x).reshape(n * k, cin))
    y, e = y.reshape(n, k, -1), e.reshape(n, k, -1)
    ys = [y]
    for i in range(1, nl):
        y, e = mlp_next(weights[i], y, e, gammas[i - 1], betas[i - 1], eps, slope, group)
        ys.append(y)
    out, bound = mlp_out(y, e, gammas[-1], betas[-1], eps, slope, group)
    return out, bound, ys
