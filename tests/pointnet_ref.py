"""numpy f64 restatement of the pcr_pointnet_forward contract (include/pcr_api.h)
from the FOLDED f32 weights, with the derived error bound per output.

The restatement is in stages, each from inputs taken as exact, because the same
form carried through all eight layers has no teeth (the bound reaches 0.44 on a
unit vector while the true f32 error is 4e-7 of it): the entry returns every
stage boundary (xtrans, mx, hid, f) so that a test can check

  point stage   x (3, P) -> conv1 -> ReLU -> conv2 -> ReLU -> max, argmax over points
  fc1           mx (256) -> hid (128), post-ReLU
  fc2           hid (128) -> f_raw (dim)
  normalise     f_raw -> f_raw / max(|f_raw|, 1e-12)

each from the call's own previous output.

Layer.  y[o] = b'[o] + sum_c W'[o][c] h[c], in the kernel one fmaf chain of n
links over c ascending that starts from the bias (3-input layers: VALU fmaf;
the others: v_mfma_f32_32x32x2_f32, bias as the accumulator's initial value).
With u = 2^-24 and an input known to e_in:

  e_out = |W'| e_in + (n + C) u (|W'| (|h| + e_in) + |b'|) + n 2^-149

  n u    the chain's n roundings, one per link (the bias enters unrounded), each
         at most u of a partial sum that |W'| |h| + |b'| dominates
  C = 2  1 for the second order of (1 + u)^n - 1 <= n u (1 + n u) with n <= 256,
         1 for the products u e_in that the first term leaves out
  2^-149 a link whose result is subnormal loses absolute, not relative, accuracy
ReLU (max(y, +0)) and the max over points are exact and 1-Lipschitz: the pooled
value's bound is the largest of its points' bounds.

Normalisation, from an exact f_raw of `dim` channels: dim rounded squares and
dim adds to +0 (the first exact) make s within (dim + 1) u; the correctly rounded
sqrt halves that and adds u; the clamp is exact; the division adds u:

  |err| <= ((dim + 1) / 2 + 2 + C_N) u |f|,   C_N = 1 (second order)

valid while every square is normal or zero (|f_raw| >= 2^-63 where nonzero);
normalise raises otherwise.

Transform: exact in f32 (transform_f32 redoes the kernel's five rounded
operations), so it has no bound.

Inputs are f32 arrays; everything here is f64 unless it says f32.
"""
import numpy as np

U = 2.0 ** -24
SUB = 2.0 ** -149
C_LAYER = 2
C_NORM = 1
EPS_NORM = float(np.float32(1e-12))


def layer(w, b, h, e_in=None):
    """w (out, n), b (out,), h (n,) or (n, P) -> (y, bound) of the pre-activation, f64."""
    w, b, h = (np.asarray(a, np.float64) for a in (w, b, h))
    n = w.shape[1]
    bb = b if h.ndim == 1 else b[:, None]
    e = np.zeros_like(h) if e_in is None else np.asarray(e_in, np.float64)
    aw = np.abs(w)
    y = w @ h + bb
    bound = aw @ e + (n + C_LAYER) * U * (aw @ (np.abs(h) + e) + np.abs(bb)) + n * SUB
    return y, bound


def relu(y):
    return np.maximum(y, 0.0)


def point_stage(l1, l2, x):
    """l1 = (W1', b1'), l2 = (W2', b2'), x (3, P) f32, exact.  Returns a dict: h2, e2 (256, P) the
    post-ReLU output of conv2 and its bound, y2 its pre-activation, mx, e_mx (256,), amx (256,)
    the lowest index of the f64 maximum."""
    y1, e1 = layer(l1[0], l1[1], x)
    y2, e2 = layer(l2[0], l2[1], relu(y1), e1)
    h2 = relu(y2)
    return {"h2": h2, "e2": e2, "y2": y2, "mx": h2.max(1), "e_mx": e2.max(1), "amx": h2.argmax(1)}


def fc1(l3, mx):
    """hid (128,) post-ReLU and its bound from an exact mx (256,)."""
    y, e = layer(l3[0], l3[1], mx)
    return relu(y), e


def fc2(l4, hid):
    """f_raw (dim,) and its bound from an exact hid (128,)."""
    return layer(l4[0], l4[1], hid)


def normalise(f_raw):
    """(f, bound) from an exact f_raw (dim,)."""
    f_raw = np.asarray(f_raw, np.float64)
    nz = np.abs(f_raw[f_raw != 0])
    if nz.size and nz.min() < 2.0 ** -63:
        raise ValueError("pointnet_ref: the normalisation bound needs every square to be normal")
    dim = f_raw.shape[0]
    f = f_raw / max(np.sqrt((f_raw * f_raw).sum()), EPS_NORM)
    return f, ((dim + 1) / 2 + 2 + C_NORM) * U * np.abs(f)


def add_identity_f32(t):
    """trans = t + I as the contract does it: one f32 add per element (the zeros of I too)."""
    return (np.asarray(t, np.float32).reshape(-1, 9) + np.eye(3, dtype=np.float32).reshape(1, 9)).astype(np.float32)


def transform_f32(trans, x):
    """xtrans (B, 3, P) f32 bit for bit: (T[r][0] x + T[r][1] y) + T[r][2] z, every operation
    rounded to f32.  trans (B, 9) f32, x (B, 3, P) f32."""
    t = np.asarray(trans, np.float32).reshape(-1, 3, 3)
    x = np.asarray(x, np.float32)
    p = [(t[:, :, k, None] * x[:, None, k, :]).astype(np.float32) for k in range(3)]
    return ((p[0] + p[1]).astype(np.float32) + p[2]).astype(np.float32)


def decidable(res, margin=2.0):
    """Channels of one patch whose argmax is decided by the bounds.  Returns (dead, clear): `dead`
    -- the pre-activation plus its bound is negative at every point, so mx = +0 and amx = 0
    whatever the rounding; `clear` -- the f64 maximum leads every other point by more than
    `margin` bounds (its own plus the other's), so amx is the f64 argmax."""
    y2, e2, h2 = res["y2"], res["e2"], res["h2"]
    dead = (y2 + e2 < 0).all(1)
    top = res["amx"]
    rows = np.arange(h2.shape[0])
    gap = h2[rows, top][:, None] - h2 - margin * 0.5 * (e2[rows, top][:, None] + e2)
    gap[rows, top] = np.inf
    clear = (gap > 0).all(1) & ~dead
    return dead, clear


# ---- whole networks: folded layers as numpy arrays, and the stage-by-stage comparison ----

LAYERS = ("conv1", "conv2", "fc1", "fc2")


def folded_layers(net):
    """{"stn": [(W', b')] * 4, "main": [(W', b')] * 4} as f32 numpy arrays, through pointnet.fold."""
    from pointcloudregistration_amd import pointnet

    def branch(mod):
        out = []
        for name in LAYERS:
            layer_, bn = pointnet._parts(getattr(mod, name), name)
            w, b = pointnet.fold(layer_, bn)
            out.append((w.numpy(), b.numpy()))
        return out
    return {"stn": branch(net.stn3d), "main": branch(net)}


def net_from_arrays(sd, dim=32):
    """This package's dip.PointNetFeature(dim), eval mode, loaded (strictly) with a state dict of arrays."""
    import torch
    from pointcloudregistration_amd import dip
    net = dip.PointNetFeature(dim)
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    return net.eval()


def stage_ratios(folded, g):
    """max |reference - restatement| / bound per stage, for one patch's recorded stage outputs `g`
    (the keys of pointnet_golden.npz without the patch name), each stage restated from the
    RECORDED previous stage.  Two stages are f32 operations of the reference outside the layer
    form and get their own roundings: trans = fc2 + I (one add: u |trans| on top of fc2's bound) and
    xtrans = bmm(trans, x) (three products, two sums in some order: (3 + C) u |T| |x|)."""
    stn, main = folded["stn"], folded["main"]
    x = g["x"]
    r = {}

    def ratio(ref, want, bound):
        return float((np.abs(np.asarray(ref, np.float64) - want) / bound).max())
    ps = point_stage(stn[0], stn[1], x)
    r["stn_point"] = ratio(g["stn_mx"], ps["mx"], ps["e_mx"])
    r["stn_fc1"] = ratio(g["stn_hid"], *fc1(stn[2], g["stn_mx"]))
    t, e = fc2(stn[3], g["stn_hid"])
    t = t + np.eye(3).reshape(9)
    r["trans"] = ratio(g["trans"], t, e + U * np.abs(t))
    tm = np.asarray(g["trans"], np.float64).reshape(3, 3)
    r["xtrans"] = ratio(g["xtrans"], tm @ x, (3 + C_LAYER) * U * (np.abs(tm) @ np.abs(x)) + 3 * SUB)
    pm = point_stage(main[0], main[1], g["xtrans"])
    r["point"] = ratio(g["mx"], pm["mx"], pm["e_mx"])
    r["fc1"] = ratio(g["fc1"], *fc1(main[2], g["mx"]))
    r["fc2"] = ratio(g["fc2"], *fc2(main[3], g["fc1"]))
    f, e = normalise(g["fc2"])
    r["norm"] = ratio(g["f"], f, e + SUB)
    return r


def _live(y, e):
    """A bound after ReLU: a unit whose pre-activation plus bound is negative is +0 exactly."""
    return np.where(y + e < 0, 0.0, e)


def chain(folded, x, tnet=True, l2norm=True):
    """The whole network on one exact patch x (3, P): (f, E) with E a bound on |f32 result - f| for
    ANY implementation whose stages each keep their stage bound, so two such implementations
    differ by at most 2 E.  The sum is formed stage by stage: a stage's bound is the layer form
    with e_in the bound carried so far (|W'| e_in + own roundings), set to 0 after a ReLU where
    the unit is certainly dead; the pool takes the largest bound of its points; trans adds
    u |trans|; xtrans = T x carries e_T |x| + (3 + C) u (|T| + e_T) |x| (each term passes three
    roundings); the normalisation of g = f_raw known to e turns into 2 |e|_2 / (|g|_2 - |e|_2) on
    every component (the direction's change plus the norm's) plus its own bound.  This sum has
    few teeth (it multiplies bounds through |W'|); the stage checks are the sharp ones."""
    x = np.asarray(x, np.float64)
    ex = np.zeros_like(x)

    def branch(ls, xin, ein):
        y1, e1 = layer(ls[0][0], ls[0][1], xin, ein)
        y2, e2 = layer(ls[1][0], ls[1][1], relu(y1), _live(y1, e1))
        mx, emx = relu(y2).max(1), _live(y2, e2).max(1)
        y3, e3 = layer(ls[2][0], ls[2][1], mx, emx)
        return layer(ls[3][0], ls[3][1], relu(y3), _live(y3, e3))

    if tnet:
        t, et = branch(folded["stn"], x, ex)
        t = t + np.eye(3).reshape(9)
        et = et + U * (np.abs(t) + et)
        tm, etm = t.reshape(3, 3), et.reshape(3, 3)
        ex = etm @ np.abs(x) + (3 + C_LAYER) * U * ((np.abs(tm) + etm) @ np.abs(x)) + 3 * SUB
        x = tm @ x
    g, eg = branch(folded["main"], x, ex)
    if not l2norm:
        return g, eg
    norm, en = np.sqrt((g * g).sum()), np.sqrt((eg * eg).sum())
    if not norm - en > EPS_NORM:
        raise ValueError("pointnet_ref: the chained bound needs |f_raw| above its own error")
    f, e = normalise(g)
    return f, 2 * en / (norm - en) + e * (1 + 2 * en / (norm - en))
