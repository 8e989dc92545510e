"""numpy f64 restatement of the pcr_kpconv_forward / pcr_neighbor_max contracts
(include/pcr_api.h), with the derived error bound per output.

  out[i,o]   = sum_e sum_c (sum_j h[i,j,e] f[j,c]) W[e,c,o] / cnt_i
  cnt_i      = max(1, #{real j : rowsum32(f[j,:]) > 0})
  bound[i,o] = 2^-24 sum_{j real, e, c} ((k + K C_in + 16) h64 + 8) |f| |W| / cnt_i

The first term of the bound is the worst-case f32 summation error over the
k-long and the K C_in-long chains in any order (each of the at most
k + K C_in additions and the two products lose at most 2^-24 relative, and the
products' magnitudes are h |f| |W|; the 16 covers the padded steps, the
division and the second-order terms at these sizes); the +8 is the absolute
error of an f32 h in units of 2^-24 (difference, squares and their sum, square
root, division, subtraction: h <= 1 and every intermediate is O(1)).

A pad is an index outside [0, m).  The inputs are f32 arrays; everything but
the row flags (an f32 sum in ascending channel order, as the kernel's) is f64.
"""
import numpy as np

EPS = 2.0 ** -24


def row_flags(f):
    """rowsum > 0 with the f32 sum taken channel by channel."""
    s = np.zeros(f.shape[0], np.float32)
    for c in range(f.shape[1]):
        s = (s + f[:, c]).astype(np.float32)
    return s > 0


def kpconv(q, s, f, idx, kp, W, extent, influence="linear"):
    """-> (out f64 (n,C_out), bound f64 (n,C_out), allpad bool (n,))."""
    n, k = idx.shape
    m, c_in = f.shape
    K = kp.shape[0]
    idx = idx.astype(np.int64)
    real = (idx >= 0) & (idx < m)
    ii = np.where(real, idx, 0)
    q64, s64, f64, kp64, W64 = (np.asarray(a, np.float64) for a in (q, s, f, kp, W))
    rel = s64[ii] - q64[:, None, :]                              # (n,k,3)
    d = rel[:, :, None, :] - kp64[None, None, :, :]              # (n,k,K,3)
    d2 = (d ** 2).sum(-1) + 1e-8
    if influence == "linear":
        h = np.maximum(0.0, 1.0 - np.sqrt(d2) / float(extent))
    elif influence == "constant":
        h = np.ones_like(d2)
    else:
        raise ValueError(influence)
    rm = real[:, :, None].astype(np.float64)
    h = h * rm
    fn = f64[ii] * rm                                            # (n,k,C_in)
    cnt = np.maximum(1, (real & row_flags(np.asarray(f, np.float32))[ii]).sum(1)).astype(np.float64)
    kf = np.einsum("nke,nkc->nec", h, fn)
    out = np.einsum("nec,eco->no", kf, W64) / cnt[:, None]
    hb = ((k + K * c_in + 16) * h + 8.0) * rm
    kb = np.einsum("nke,nkc->nec", hb, np.abs(fn))
    bound = EPS * np.einsum("nec,eco->no", kb, np.abs(W64)) / cnt[:, None]
    return out, bound, ~real.any(1)


def neighbor_max(feats, idx):
    """MaxPoolBlock: max over the columns, a pad reading 0.  Exact in f32."""
    m = feats.shape[0]
    idx = idx.astype(np.int64)
    real = (idx >= 0) & (idx < m)
    padded = np.concatenate([feats, np.zeros_like(feats[:1])], 0)
    return padded[np.where(real, idx, m)].max(1)
