"""numpy f64 restatement of the pcr_unary_forward contract (include/pcr_api.h) in
the REFERENCE's form -- gather, concatenate, Linear, InstanceNorm1d, residual
add, LeakyReLU (c2p-net/ngenet/models/KPConv/blocks.py:135-290) -- with a
derived error bound per stage.  Inputs are f32 arrays taken as exact;
everything is f64.  The layer, the statistics and the normalisation are
tests/groupmlp_ref.py's (imported, not copied): the kernels share the rule.

Stages, each checked from the call's own previous one (y, stats, out).

Operand.  row_i = [x0[g_i] | x1[i]], a g_i outside [0, m0) a row of zeros:
copies, exact.

Product.  y = W row_i is groupmlp_ref.layer: n = c0 + c1 roundings bounded by
(n + 2) u |W| |row| + n 2^-149, for ANY order of the n terms (the MFMA's, the
reference's BLAS).  layer's comment argues its second-order constant for
n <= 512; here n reaches 2048.  The argument: the exact constant of an n-term
f32 dot product is g_n = n u / (1 - n u) (Higham, Accuracy and Stability,
3.1), and g_n <= (n + 1) u  <=>  n <= (n + 1)(1 - n u)  <=>  n (n + 1) u <= 1.
At n = 2048, n (n + 1) u = 2048 * 2049 * 2^-24 < 0.2502.  So (n + 1) u covers
first and second order up to n = 4095 and the bound's (n + 2) u leaves the
last u for the products u e_in, as there.  test_unary_cpu re-checks the
inequality in exact arithmetic.

Statistics.  groupmlp_ref.moments_bound with m = n rows (group 1).

Norm.  groupmlp_ref.norm_act with slope 1 (its activation is then the
identity): pre = fmaf(y, a, b) and its bound e_pre; that call adds one
rounding u (|pre| + e_pre) for a slope product the kernel does not make here,
which only widens the bound.
Bias (norm = 0).  pre = y + bias is one rounded f32 add (exact where its result
is subnormal): e_pre = e_y + u (|pre| + e_y).
Residual.  z = pre + res, one rounded add, res known to e_res:
e_z = (e_pre + e_res) + u (|z| + e_pre + e_res).
Activation.  z -> (z > 0 ? z : slope z) is 1-Lipschitz for |slope| <= 1; the
product is one rounding where slope is neither 0 nor 1 (and may be subnormal):
e_out = e_z + u (|out| + e_z) + 2^-149.

No constant here is fitted to a result.
"""
import numpy as np

from groupmlp_ref import D, SUB, U, f64, layer, moments, moments_bound, norm_act, ratio  # noqa: F401


def operand(x0, gather=None, x1=None):
    """(n, c0 + c1) f64: row i = [x0[gather[i]] | x1[i]], an index outside [0, m0) a row of zeros."""
    x0 = f64(x0)
    if gather is None:
        rows = x0
    else:
        g = np.asarray(gather).astype(np.int64)
        ok = (g >= 0) & (g < x0.shape[0])
        rows = np.where(ok[:, None], x0[np.where(ok, g, 0)], 0.0)
    if x1 is not None:
        rows = np.concatenate([rows, f64(x1)], axis=1)
    return rows


def product(w, x0, gather=None, x1=None, e_in=None):
    """y (n, cout) and its bound; w None: the operand itself, exact (or known to e_in)."""
    rows = operand(x0, gather, x1)
    if w is None:
        return rows, np.zeros_like(rows) if e_in is None else np.broadcast_to(f64(e_in), rows.shape)
    return layer(w, rows, e_in)


def finish(y, e, bias=None, norm=True, eps=1e-5, slope=0.1, act=True, res=None, e_res=0.0):
    """y (n, cout) known to e -> (out, bound) through norm or bias, residual (known to e_res) and
    activation."""
    if abs(slope) > 1:
        raise ValueError("unary_ref: the activation bound needs |slope| <= 1")
    y = f64(y)
    e = np.broadcast_to(f64(e), y.shape)
    if norm:
        if bias is not None:
            raise ValueError("unary_ref: bias together with norm")
        z, e_z = norm_act(y, e, None, None, eps, 1.0)
    elif bias is not None:
        z = y + f64(bias)
        e_z = e + U * (np.abs(z) + e)
    else:
        z, e_z = y, e
    if res is not None:
        z = z + f64(res)
        e_z = e_z + e_res
        e_z = e_z + U * (np.abs(z) + e_z)
    if not act:
        return z, e_z
    out = np.where(z > 0, z, slope * z)
    if slope in (0.0, 1.0):
        return out, e_z
    return out, e_z + U * (np.abs(out) + e_z) + SUB


def unary(w, x0, gather=None, x1=None, bias=None, norm=True, eps=1e-5, slope=0.1, act=True, res=None, e_in=None):
    """End to end from exact inputs (or an operand known to e_in): (out, carried bound, y)."""
    y, e = product(w, x0, gather, x1, e_in)
    out, bound = finish(y, e, bias, norm, eps, slope, act, res)
    return out, bound, y


# ---- the reference's blocks, stage by stage ----------------------------------------------

def block_stages(kind, case, conv_in, conv_out, eps=1e-5, slope=0.1):
    """SimpleBlock / ResnetBottleneckBlock.forward (blocks.py:222-233, 271-290) from a case of
    tests/golden/unary_cases.make_block and the f32 tensors a run recorded around its KPConv (taken as
    exact, so that no bound is carried through the convolution and its neighbour count).  Returns
    {stage: (value, bound)} for conv_in (None when the block has no unary1), conv_out and out."""
    import kpconv_conv_ref as kr
    p, b = case["params"], case["batch"]
    strided = "strided" in kind
    q, idx = (b["points"][1], b["pools"][0]) if strided else (b["points"][0], b["neighbors"][0])
    st = {"conv_in": None}
    if "unary1.mlp.weight" in p:
        st["conv_in"] = unary(p["unary1.mlp.weight"], case["f"], eps=eps, slope=slope)[:2]
    st["conv_out"] = kr.kpconv(q, b["points"][0], conv_in, idx, case["kp"], p["KPConv.weights"], case["extent"])[:2]
    bias = p.get("bn.bias")
    h, e_h = finish(conv_out, 0.0, bias, bias is None, eps, slope, True)
    if kind == "simple":
        st["out"] = (h, e_h)
        return st
    short = kr.neighbor_max(case["f"], idx) if strided else case["f"]
    e_sc = 0.0
    if "unary_shortcut.mlp.weight" in p:
        short, e_sc, _ = unary(p["unary_shortcut.mlp.weight"], short, eps=eps, act=False)
    y2, e2 = layer(p["unary2.mlp.weight"], h, e_h)
    st["out"] = finish(y2, e2, None, True, eps, slope, True, short, e_sc)
    return st
