"""numpy f64 restatements of the pcr_attention_forward and
pcr_offset_attention_forward contracts (include/pcr_api.h), each with the
derived error bound per output.

Attention (one batch element and head; q (d,n), k (d,m), v (dv,m)):

  s_ij = scale sum_c q[c,i] k[c,j],  p = softmax_j s,  out[c,i] = sum_j p_ij v[c,j]

Bound.  u = 2^-24, x_ij = s_ij - max_j s_ij <= 0, T = ceil(m / 32) key tiles.

  delta_ij = |scale| (d + 3) u sum_c |q_ci| |k_cj|
      the score's error: a d-long fmaf chain (d u relative to the sum of the
      products' magnitudes), the product with the scale (1 u), 2 u of slack for
      the second order.
  eta_ij = expm1(2 delta_ij + 2 |x_ij| u + K u),   K = 43 + 4 T
      the relative error of weight j as it enters out_i, numerator or
      denominator.  2 delta: the score's error and the maximum's.  2 |x| u: the
      roundings of the exponents' arguments -- score minus running maximum
      (|x| u at most), and the rescale factors' arguments old max - new max,
      which telescope to at most |x_ij| over the tiles (and the key split)
      after j's.  K counts, in units of u, what the kernel does to a weight:
        2        expf of the weight (1 ulp)
        3 T      one rescale per later tile: expf of the factor (2) and the
                 product with the accumulator or the sum (1)
        17 + T   the sum of the weights: 16 adds inside a tile and lane half,
                 one add per tile, one for the other lane half
        19       the key split's fold: expf of a run's factor (2), its
                 product (1), up to 16 runs added
        5        the final division (2.5 ulp, were it not correctly rounded)
  bound_ci = sum_j p_ij eta_ij (|v_cj| + |out_ci|) / (1 - max_j eta_ij)
             + (m + 18) u sum_j p_ij |v_cj| + 2^-126 sum_j |v_cj|
      first term: out = N / L with both sums over weights in error by eta;
      second: the value products' own chain, at most m nonzero steps of the
      MFMA (dv <= 4: 16 T + 2 separately rounded operations); third: weights and
      rescaled partial sums below the normal range lose absolute, not
      relative, accuracy (at most 2^-126 each, with sum L >= 1).

Offset form (one batch element; q, k (d,n), v (dv,n), r (n,) or None):

  a_ij = r_i sum_c q[c,i] k[c,j],  P = softmax_j a,  c_j = sum_i P_ij,
  out[ch,j] = sum_i v[ch,i] P_ij / (f32(1e-9) + c_j)

  eta1_ij = expm1(2 delta_ij + 2 |x_ij| u + (19 + 4 T) u): sweep 1's weights (as
      above without the split and the division), so the row sum L_i is off by
      etaL_i = sum_j P_ij eta1_ij / (1 - max_j eta1_ij), relatively.
  eta2_ij = (1 + expm1(2 delta_ij + 2 |x_ij| u + 8 u)) (1 + etaL_i / (1 - etaL_i)) - 1:
      sweep 2's weight expf(a - max) * (1 / L): expf (2), the reciprocal (5), the
      product (1), and L's own error.
  E_N = sum_i |v_i| P_ij eta2_ij + (n + 18) u (1 + max eta2) sum_i |v_i| P_ij + 2^-126 sum_i |v_i|
  E_c = sum_i P_ij eta2_ij + (n + 18) u (1 + max eta2) c_j + u (1e-9 + c_j) + 2^-126 n
  bound = (E_N + |out| E_c) / (1e-9 + c_j - E_c) + 6 u |out|
      (the chains over i: 16 adds inside a tile and lane half, one per tile, one
      for the other half; weights below the normal range lose at most 2^-126
      absolute each; the rounding of 1e-9 + c_j; the quotient rule; the
      division's 5 u and 1 u of slack).

Inputs are f32 arrays; everything here is f64.
"""
import numpy as np

U = 2.0 ** -24
TINY = 2.0 ** -126
TILE = 32
EPS_COL = float(np.float32(1e-9))


def k_attention(m):
    return 43 + 4 * (-(-m // TILE))


def _scores(q, k, scale_rows):
    """scale_rows (n,1) f64 -> s (n,m), delta (n,m)."""
    d = q.shape[0]
    s = scale_rows * (q.T @ k)
    delta = np.abs(scale_rows) * (d + 3) * U * (np.abs(q).T @ np.abs(k))
    return s, delta


def attention(q, k, v, scale):
    """q (d,n), k (d,m), v (dv,m) f32 -> (out (dv,n), bound (dv,n), p (n,m), eta (n,m)), f64."""
    q, k, v = (np.asarray(a, np.float64) for a in (q, k, v))
    n, m = q.shape[1], k.shape[1]
    s, delta = _scores(q, k, np.full((n, 1), float(scale)))
    x = s - s.max(1, keepdims=True)
    e = np.exp(x)
    p = e / e.sum(1, keepdims=True)
    out = v @ p.T
    eta = np.expm1(2 * delta + 2 * np.abs(x) * U + k_attention(m) * U)
    emax = eta.max(1)
    if not (emax < 1).all():
        raise ValueError("attention_ref: the bound needs eta < 1")
    pe = p * eta
    bound = (np.abs(v) @ pe.T + np.abs(out) * pe.sum(1)[None, :]) / (1 - emax)[None, :]
    bound = bound + (m + 18) * U * (np.abs(v) @ p.T) + TINY * np.abs(v).sum(1, keepdims=True)
    return out, bound, p, eta


def multi_head(query, key, value, scale=None):
    """The layout of multi_head_attention: (B,d,h,N), (B,d,h,M), (B,dv,h,M) -> out, bound (B,dv,h,N)."""
    b, d, h, n = query.shape
    dv = value.shape[1]
    sc = 1.0 / np.sqrt(d) if scale is None else scale
    out = np.zeros((b, dv, h, n))
    bound = np.zeros_like(out)
    for bi in range(b):
        for hi in range(h):
            o, bd, _, _ = attention(query[bi, :, hi], key[bi, :, hi], value[bi, :, hi], sc)
            out[bi, :, hi], bound[bi, :, hi] = o, bd
    return out, bound


def overlap_scores(feats_norm, attn_scores, len_src, temperature):
    """NgeNet.py:173-179 from the contract: feats_norm (n,C), attn_scores (n,1) -> out, bound (n,1)."""
    f = np.asarray(feats_norm, np.float64).T
    a = np.asarray(attn_scores, np.float64).T
    n1 = int(len_src)
    sc = float(np.float32(1.0 / float(temperature)))   # the f32 the call receives
    o1, b1, _, _ = attention(f[:, :n1], f[:, n1:], a[:, n1:], sc)
    o2, b2, _, _ = attention(f[:, n1:], f[:, :n1], a[:, :n1], sc)
    return np.concatenate([o1, o2], 1).T, np.concatenate([b1, b2], 1).T


def offset_attention(q, k, v, r=None, cols=None):
    """q, k (d,n), v (dv,n), r (n,) or None, f32 -> (out (dv,n), bound (dv,n), P (n,n)), f64.
    cols: an index array; out, bound and P are then restricted to those columns j (the rows' softmax
    still runs over every column)."""
    q, k, v = (np.asarray(a, np.float64) for a in (q, k, v))
    n = q.shape[1]
    t = -(-n // TILE)
    rr = np.ones((n, 1)) if r is None else np.asarray(r, np.float64).reshape(n, 1)
    s, delta = _scores(q, k, rr)
    x = s - s.max(1, keepdims=True)
    e = np.exp(x)
    p = e / e.sum(1, keepdims=True)
    arg = 2 * delta + 2 * np.abs(x) * U
    eta1 = np.expm1(arg + (19 + 4 * t) * U)
    if not (eta1.max(1) < 1).all():
        raise ValueError("attention_ref: the bound needs eta1 < 1")
    eta_l = (p * eta1).sum(1) / (1 - eta1.max(1))
    if not (eta_l < 1).all():
        raise ValueError("attention_ref: the bound needs etaL < 1")
    if cols is not None:
        p, arg = p[:, cols], arg[:, cols]
    c = p.sum(0)
    num = v @ p
    out = num / (EPS_COL + c)[None, :]
    eta2 = (1 + np.expm1(arg + 8 * U)) * (1 + eta_l / (1 - eta_l))[:, None] - 1
    pe = p * eta2
    chain = (n + 18) * U * (1 + eta2.max())
    e_n = np.abs(v) @ pe + chain * (np.abs(v) @ p) + TINY * np.abs(v).sum(1, keepdims=True)
    e_c = pe.sum(0) + chain * c + U * (EPS_COL + c) + TINY * n
    den = EPS_COL + c - e_c
    if not (den > 0).all():
        raise ValueError("attention_ref: the bound needs 1e-9 + c_j above its own error")
    bound = (e_n + np.abs(out) * e_c[None, :]) / den[None, :] + 6 * U * np.abs(out)
    return out, bound, p


def offset_batched(x_q, x_k, x_v, ol=None):
    """(B,d,N), (B,d,N), (B,C,N), (B,N) or None -> out, bound (B,C,N)."""
    outs, bounds = [], []
    for bi in range(x_q.shape[0]):
        o, bd, _ = offset_attention(x_q[bi], x_k[bi], x_v[bi], None if ol is None else ol[bi])
        outs.append(o)
        bounds.append(bd)
    return np.stack(outs), np.stack(bounds)
