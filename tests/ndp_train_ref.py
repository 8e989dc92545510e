"""f64 restatement of one fused NDP level step (include/pcr_api.h:
pcr_ndp_train_forward / pcr_ndp_train_backward), written from the semantics --
NDPLayer.forward (positional encoding, MLP, branches, axis-angle Rodrigues,
optional nonrigidity blend) and the chain rule in vector form -- not from the
kernels.  numpy only in `level_step`; tests/test_ndp_train_ref_cpu.py pins it to
f64 torch autograd of ndp_opt.NDPLayer (`autograd_step` below), and the GPU
tests then stand on it.

The loss whose gradient the backward returns is
    L = sum(x' * g) + bce_scale * sum_p -log(1 - s_p)
(g = dL/dx' from the Chamfer pass, bce_scale = w_reg / N: the mean BCE(s, 0)).

Layouts are the kernels' (csrc/ndp_train.hip), feature-major:
    pe  [6][N]          sin, cos of 2^(m + k0) x per coordinate
    H   [depth][W][N]   H_0 = relu(input layer), H_l = relu(hidden layer l)
    aux [8][N]          r = 1e-3 o_rot (3), y = R x + t (3), s, 0
    x_out (N, 3)
    dO  [8][N]          dL/d(branch pre-activation): rot (3), trn (3), nr, 0
    D   [depth][W][N]   dL/d(pre-activation) of layer l
    grads               [w_in (W,6), b_in (W)] + [w_hid_k (W,W), b_hid_k (W)] * (depth - 1)
                        + [w_branch (7,W), b_branch (7)]  (rows rot 0-2, trn 3-5, nr 6)
    min_preact          min |pre-activation| over all hidden units, layers and points

Also here, shared by the CPU test, the GPU tests and tests/golden/
make_ndp_train_bounds.py: the case list (`CASES`, `BIG_CASES`), the case data
(`make_case`: numpy Generator streams only, so the data do not depend on a
torch version), the tensor groups and the error measure (`group_errors`).
"""
import numpy as np

SCALE = 1e-3        # NDPLayer.mlp_scale
WIDTH = 128
GUARD = 1e-5        # the f64 min |pre-activation| every case must keep (ReLU kinks)
ULP4 = 4.0 * 2.0 ** -23   # 4 f32 ulps of a tensor's largest entry


# --------------------------------------------------------------------------
# the restatement
# --------------------------------------------------------------------------

def params_of(layer):
    """The f64 parameter dict of an ndp_opt.NDPLayer (any dtype / device)."""
    sd = {k: v.detach().cpu().double().numpy() for k, v in layer.state_dict().items()}
    nhid = sum(1 for k in sd if k.startswith("mlp.pts_linears.") and k.endswith(".weight"))
    return dict(m=int(layer.m), k0=int(layer.k0),
                w_in=sd["input.0.weight"], b_in=sd["input.0.bias"],
                w_hid=[sd[f"mlp.pts_linears.{k}.weight"] for k in range(nhid)],
                b_hid=[sd[f"mlp.pts_linears.{k}.bias"] for k in range(nhid)],
                w_rot=sd["rot_brach.weight"], b_rot=sd["rot_brach.bias"],
                w_trn=sd["trn_branch.weight"], b_trn=sd["trn_branch.bias"],
                w_nr=sd.get("nr_branch.weight"), b_nr=sd.get("nr_branch.bias"))


def _cross(a, b):
    return np.stack([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])


def level_step(P, x, g, bce_scale):
    """One level's forward and backward in f64.  P: `params_of`; x (N,3); g (N,3)
    = dL/dx'; bce_scale = w_reg / N (0: no BCE term).  N >= 1."""
    f = np.float64
    X = np.asarray(x, f).reshape(-1, 3).T            # (3, N)
    G = np.asarray(g, f).reshape(-1, 3).T
    N = X.shape[1]
    W = P["w_in"].shape[0]
    depth = len(P["w_hid"]) + 1
    has_nr = P["w_nr"] is not None

    # ---- forward
    v = X * 2.0 ** (P["m"] + P["k0"])
    pe = np.empty((6, N), f)
    pe[0::2] = np.sin(v)
    pe[1::2] = np.cos(v)
    Z = np.empty((depth, W, N), f)
    Z[0] = P["w_in"].astype(f) @ pe + P["b_in"].astype(f)[:, None]
    for k in range(depth - 1):
        Z[k + 1] = P["w_hid"][k].astype(f) @ np.maximum(Z[k], 0.0) + P["b_hid"][k].astype(f)[:, None]
    H = np.maximum(Z, 0.0)
    fea = H[-1]
    r = SCALE * (P["w_rot"].astype(f) @ fea + P["b_rot"].astype(f)[:, None])     # (3, N)
    t = SCALE * (P["w_trn"].astype(f) @ fea + P["b_trn"].astype(f)[:, None])
    th = np.sqrt((r * r).sum(0))
    w = r / th
    a, b = np.sin(th), 1.0 - np.cos(th)
    wx = _cross(w, X)                     # K x
    wwx = w * (w * X).sum(0) - X          # K K x = w (w.x) - x for |w| = 1
    y = X + a * wx + b * wwx + t
    if has_nr:
        s = 1.0 / (1.0 + np.exp(-SCALE * (P["w_nr"].astype(f) @ fea + P["b_nr"].astype(f)[:, None])[0]))
        xo = X + s * (y - X)
    else:
        s = np.zeros(N, f)
        xo = y
    aux = np.zeros((8, N), f)
    aux[0:3], aux[3:6], aux[6] = r, y, s

    # ---- backward
    dO = np.zeros((8, N), f)
    gy = G
    if has_nr:
        ds = (G * (y - X)).sum(0) + bce_scale / (1.0 - s)      # d(-log(1 - s))/ds = 1 / (1 - s)
        dO[6] = SCALE * ds * s * (1.0 - s)
        gy = G * s
    dO[3:6] = SCALE * gy
    # y = x + sin(th) w x x + (1 - cos th) (w (w.x) - x), w = r / th, th = |r|
    dth = (gy * (np.cos(th) * wx + a * wwx)).sum(0)
    dw = a * _cross(X, gy) + b * ((w * X).sum(0) * gy + (gy * w).sum(0) * X)
    dO[0:3] = SCALE * (dth * w + (dw - (dw * w).sum(0) * w) / th)
    Wb = [P["w_rot"], P["w_trn"]] + ([P["w_nr"]] if has_nr else [np.zeros((1, W))])
    Wb = np.concatenate(Wb, 0).astype(f)                        # (7, W)
    D = np.empty((depth, W, N), f)
    D[-1] = (Wb.T @ dO[:7]) * (Z[-1] > 0)
    for k in range(depth - 2, -1, -1):
        D[k] = (P["w_hid"][k].astype(f).T @ D[k + 1]) * (Z[k] > 0)
    grads = [D[0] @ pe.T, D[0].sum(1)]
    for k in range(depth - 1):
        grads += [D[k + 1] @ H[k].T, D[k + 1].sum(1)]
    grads += [dO[:7] @ fea.T, dO[:7].sum(1)]
    return dict(pe=pe, H=H, aux=aux, x_out=np.ascontiguousarray(xo.T), dO=dO, D=D, grads=grads,
                min_preact=float(np.abs(Z).min()))


# --------------------------------------------------------------------------
# torch autograd of ndp_opt.NDPLayer in the same layouts (any dtype, CPU or GPU)
# --------------------------------------------------------------------------

def autograd_step(layer, x, g, bce_scale):
    """NDPLayer.forward + torch.autograd.grad of the loss above.  The per-point
    quantities are the Linear modules' outputs (forward hooks) and the gradients
    with respect to them; y = R x + t comes from a second forward with the
    nonrigidity blend switched off.  Returns numpy f64 arrays (the values of the
    layer's dtype, widened)."""
    import torch
    N = x.shape[0]
    outs = {}
    mods = {"in": layer.input[0], "rot": layer.rot_brach, "trn": layer.trn_branch}
    for k, lin in enumerate(layer.mlp.pts_linears):
        mods[f"hid{k}"] = lin
    if layer.nonrigidity_est:
        mods["nr"] = layer.nr_branch
    hooks = [m.register_forward_hook(lambda _m, _i, o, n=n: outs.__setitem__(n, o)) for n, m in mods.items()]
    try:
        xo, nr = layer(x)
    finally:
        for h in hooks:
            h.remove()
    xo = xo.reshape(N, 3)
    loss = (xo * g).sum()
    if nr is not None:
        nr = nr.reshape(N)
        loss = loss - bce_scale * torch.log(1 - nr).sum()
    names = list(mods)
    params = dict(layer.named_parameters())
    pg = torch.autograd.grad(loss, [outs[n] for n in names] + list(params.values()))
    dz = dict(zip(names, pg[:len(names)]))
    dp = dict(zip(params, pg[len(names):]))
    with torch.no_grad():
        keep, layer.nonrigidity_est = layer.nonrigidity_est, False
        try:
            y = layer(x)[0].reshape(N, 3)
        finally:
            layer.nonrigidity_est = keep
        pe = layer.posenc(x)

    def n64(t):
        return t.detach().cpu().double().numpy()
    depth = len(layer.mlp.pts_linears) + 1
    zs = [outs["in"]] + [outs[f"hid{k}"] for k in range(depth - 1)]
    H = np.stack([np.maximum(n64(z), 0.0).T for z in zs])
    D = np.stack([n64(dz[n]).T for n in ["in"] + [f"hid{k}" for k in range(depth - 1)]])
    aux = np.zeros((8, N))
    aux[0:3] = SCALE * n64(outs["rot"]).T
    aux[3:6] = n64(y).T
    dO = np.zeros((8, N))
    dO[0:3], dO[3:6] = n64(dz["rot"]).T, n64(dz["trn"]).T
    W = H.shape[1]
    gwb, gbb = np.zeros((7, W)), np.zeros(7)
    gwb[0:3], gbb[0:3] = n64(dp["rot_brach.weight"]), n64(dp["rot_brach.bias"])
    gwb[3:6], gbb[3:6] = n64(dp["trn_branch.weight"]), n64(dp["trn_branch.bias"])
    if nr is not None:
        aux[6] = n64(nr)
        dO[6] = n64(dz["nr"])[:, 0]
        gwb[6], gbb[6] = n64(dp["nr_branch.weight"])[0], n64(dp["nr_branch.bias"])[0]
    grads = [n64(dp["input.0.weight"]), n64(dp["input.0.bias"])]
    for k in range(depth - 1):
        grads += [n64(dp[f"mlp.pts_linears.{k}.weight"]), n64(dp[f"mlp.pts_linears.{k}.bias"])]
    grads += [gwb, gbb]
    return dict(pe=n64(pe).T, H=H, aux=aux, x_out=n64(xo), dO=dO, D=D, grads=grads,
                min_preact=float(min(np.abs(n64(z)).min() for z in zs)))


# --------------------------------------------------------------------------
# tensor groups and the error measure
# --------------------------------------------------------------------------

GROUPS = ("xy", "r", "s", "pe", "H", "D", "dO_rot", "dO_trn", "dO_nr",
          "gw_in", "gw_hid", "gw_rot", "gw_trn", "gw_nr",
          "gb_in", "gb_hid", "gb_rot", "gb_trn", "gb_nr")
GRAD_GROUPS = tuple(n for n in GROUPS if n.startswith("g"))


def tensors(out):
    """[(group, label, array)] of one step's outputs: every tensor whose error is
    measured against its own largest reference entry."""
    depth = out["H"].shape[0]
    ts = [("xy", "x_out", out["x_out"]), ("xy", "y", out["aux"][3:6]), ("r", "r", out["aux"][0:3]),
          ("s", "s", out["aux"][6]), ("pe", "pe", out["pe"])]
    ts += [("H", f"H{k}", out["H"][k]) for k in range(depth)]
    ts += [("D", f"D{k}", out["D"][k]) for k in range(depth)]
    ts += [("dO_rot", "dO_rot", out["dO"][0:3]), ("dO_trn", "dO_trn", out["dO"][3:6]),
           ("dO_nr", "dO_nr", out["dO"][6])]
    gr = out["grads"]
    ts += [("gw_in", "gw_in", gr[0]), ("gb_in", "gb_in", gr[1])]
    for k in range(depth - 1):
        ts += [("gw_hid", f"gw_hid{k}", gr[2 + 2 * k]), ("gb_hid", f"gb_hid{k}", gr[3 + 2 * k])]
    gw, gb = gr[-2], gr[-1]
    ts += [("gw_rot", "gw_rot", gw[0:3]), ("gw_trn", "gw_trn", gw[3:6]), ("gw_nr", "gw_nr", gw[6]),
           ("gb_rot", "gb_rot", gb[0:3]), ("gb_trn", "gb_trn", gb[3:6]), ("gb_nr", "gb_nr", gb[6:7])]
    return ts


def group_errors(got, ref):
    """{group: largest over its tensors of max |got - ref| / max |ref|}.  A tensor
    whose reference is identically zero (the nr rows of a level without the
    branch) must be zero exactly: it counts 0 if it is and inf if not."""
    err = {}
    for (grp, label, a), (_, _, b) in zip(tensors(got), tensors(ref)):
        a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
        assert a.shape == b.shape, (label, a.shape, b.shape)
        top = np.abs(b).max()
        d = np.abs(a - b).max() if np.isfinite(a).all() else np.inf
        e = (0.0 if d == 0 else np.inf) if top == 0 else d / top
        err[grp] = max(err.get(grp, 0.0), float(e))
    return err


def bounds(floors):
    """Per-group bound of the f32 kernels against the f64 restatement: 4 x the
    recorded f32-autograd floor of the group (pooled over the cases given), at
    least 4 f32 ulps of the tensor's largest entry."""
    return {g: max(4.0 * float(v), ULP4) for g, v in floors.items()}


def load_floors(path, big=False):
    """{group: floor} from ndp_train_bounds.npz, pooled over the edge case list
    (or over it and BIG_CASES)."""
    z = np.load(path)
    names = [str(n) for n in z["cases"]]
    rows = [i for i, n in enumerate(names) if big or not n.startswith("big-")]
    groups = [str(g) for g in z["groups"]]
    return {g: float(z["floor"][rows, j].max()) for j, g in enumerate(groups)}


# --------------------------------------------------------------------------
# cases
# --------------------------------------------------------------------------

def _case(name, N, depth, level, seed, bce=True, chunks=(128,), K=None):
    return dict(name=name, N=N, depth=depth, level=level, seed=seed, bce=bce, chunks=tuple(chunks), K=K)


# seeds: the first at or after 100 x the case's position whose f64 minimum
# |pre-activation| is >= GUARD (make_ndp_train_bounds.py --seeds lists them)
CASES = (
    [_case(f"n{N}", N, 3, 1, s) for N, s in
     [(1, 0), (31, 100), (32, 200), (33, 300), (63, 400), (64, 500), (65, 600), (127, 701),
      (128, 800), (129, 901), (257, 1001)]]
    + [_case(f"d{d}-l{lv}", 129, d, lv, s) for (d, lv), s in
       [((1, 0), 1100), ((2, 0), 1200), ((3, 0), 1300), ((5, 0), 1400),
        ((1, 2), 1500), ((2, 2), 1601), ((3, 2), 1701), ((5, 2), 1800)]]
    + [_case("nobce", 129, 3, 1, 1900, bce=False)]
    + [_case("chunks", 513, 2, 1, 2000, chunks=(64, 128, 192, 576))]
    + [_case("sub1", 65, 3, 1, 2100, K=1), _case("sub23", 65, 3, 1, 2200, K=23)]
)
# the shape test_ndp_train_gpu.py has always run: N = 3000, depth 3, levels 0, 1, 5
BIG_CASES = [_case(f"big-l{lv}", 3000, 3, lv, s) for lv, s in [(0, 3005), (1, 3127), (5, 3576)]]
W_REG = 0.05


def make_case(c):
    """The data of a case: parameter dict (f32 values held as f32 arrays), x, g
    (the full dL/dx'; for a subset case scattered from gsub), inds / gsub, bce_scale."""
    rng = np.random.default_rng([20250117, c["seed"]])
    W, F = WIDTH, np.float32
    has_nr = c["level"] > 0

    def lin(fo, fi):  # xavier_uniform x 3 (far from the identity warp of a fresh init), bias +-0.2
        bnd = np.sqrt(6.0 / (fo + fi)) * 3.0
        return rng.uniform(-bnd, bnd, (fo, fi)).astype(F), rng.uniform(-0.2, 0.2, fo).astype(F)
    P = dict(m=c["level"] + 1, k0=-8)
    P["w_in"], P["b_in"] = lin(W, 6)
    hid = [lin(W, W) for _ in range(c["depth"] - 1)]
    P["w_hid"], P["b_hid"] = [h[0] for h in hid], [h[1] for h in hid]
    P["w_rot"], P["b_rot"] = lin(3, W)
    P["w_trn"], P["b_trn"] = lin(3, W)
    P["w_nr"], P["b_nr"] = lin(1, W) if has_nr else (None, None)
    N = c["N"]
    x = rng.uniform(-0.8, 0.8, (N, 3)).astype(F)
    out = dict(P=P, x=x, bce_scale=(W_REG / N) if (c["bce"] and has_nr) else 0.0, inds=None, gsub=None)
    if c["K"] is None:
        out["g"] = rng.standard_normal((N, 3)).astype(F)
    else:
        K = c["K"]
        inds = np.array([40]) if K == 1 else np.sort(np.append(rng.choice(N - 1, K - 1, replace=False), N - 1))
        gsub = rng.standard_normal((K, 3)).astype(F)
        g = np.zeros((N, 3), F)
        g[inds] = gsub
        out.update(g=g, inds=inds, gsub=gsub)
    return out


def make_layer(P, dtype, device="cpu"):
    """An ndp_opt.NDPLayer holding the parameters P."""
    import torch
    from pointcloudregistration_amd import ndp_opt
    depth = len(P["w_hid"]) + 1
    L = ndp_opt.NDPLayer(depth, P["w_in"].shape[0], P["k0"], P["m"], nonrigidity_est=P["w_nr"] is not None)
    sd = {"input.0.weight": P["w_in"], "input.0.bias": P["b_in"],
          "rot_brach.weight": P["w_rot"], "rot_brach.bias": P["b_rot"],
          "trn_branch.weight": P["w_trn"], "trn_branch.bias": P["b_trn"]}
    for k in range(depth - 1):
        sd[f"mlp.pts_linears.{k}.weight"], sd[f"mlp.pts_linears.{k}.bias"] = P["w_hid"][k], P["b_hid"][k]
    if P["w_nr"] is not None:
        sd["nr_branch.weight"], sd["nr_branch.bias"] = P["w_nr"], P["b_nr"]
    L.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    return L.to(dtype=dtype, device=device)
