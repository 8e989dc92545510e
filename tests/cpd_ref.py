"""The CPD contract of include/pcr_api.h restated in numpy f64 (Myronenko & Song
2010 with probreg's conventions as far as they are known; not pinned against
probreg, which is not available to this project).  This file is the yardstick of
tests/test_cpd_cpu.py and tests/test_cpd_gpu.py.

``estep`` is the contract in f64 (dense), ``estep_matrix_free`` the same sums
without any (M, N) array, and ``estep_f32`` probreg's dense formulation in f32,
the program whose own distance from f64 sets the GPU tests' tolerances.
"""
import numpy as np

F32 = np.float32
FLT_EPSILON = float(np.finfo(np.float32).eps)
FLUSH_ARG = -87.0     # a term whose argument is below this may be kept, flushed or skipped
RIGID, RIGID_SCALE, AFFINE = 0, 1, 2


def initial_sigma2(Y, X):
    """sum_mn |x_n - y_m|^2 / (3 M N) in f64, by the closed form about x_0."""
    X, Y = np.asarray(X, np.float64), np.asarray(Y, np.float64)
    c = X[0]
    xc, yc = X - c, Y - c
    M, N = len(Y), len(X)
    tot = M * (xc * xc).sum() + N * (yc * yc).sum() - 2.0 * xc.sum(0) @ yc.sum(0)
    return float(tot / (3.0 * M * N))


def apply_T(T, Y):
    """y^ = (float)(T y), T (>=3, 4) applied in f64 as ((T0 x + T1 y) + T2 z) + T3."""
    Y = np.asarray(Y, np.float64)
    if T is None:
        return np.asarray(Y, F32)
    T = np.asarray(T, np.float64)
    out = np.empty((len(Y), 3))
    for a in range(3):
        out[:, a] = ((T[a, 0] * Y[:, 0] + T[a, 1] * Y[:, 1]) + T[a, 2] * Y[:, 2]) + T[a, 3]
    return out.astype(F32)


def sqdist_f32(ys, X):
    """(M, N) f32: d = (dx dx + dy dy) + dz dz, each operation rounded to f32."""
    ys, X = np.asarray(ys, F32), np.asarray(X, F32)
    dx = ys[:, None, 0] - X[None, :, 0]
    dy = ys[:, None, 1] - X[None, :, 1]
    dz = ys[:, None, 2] - X[None, :, 2]
    return (dx * dx + dy * dy) + dz * dz


def const_c(sigma2, w, M, N):
    return (2.0 * np.pi * sigma2) ** 1.5 * w / (1.0 - w) * M / N


def column_max_args(ys, X, sigma2):
    """Per target column the largest exponent argument -d / (2 sigma2)."""
    return (-sqdist_f32(ys, X).astype(np.float64) / (2.0 * sigma2)).max(0)


def estep(ys, X, sigma2, w):
    """The contract's E-step in f64 on the f32 transformed sources `ys`:
    (pt1 (N), p1 (M), px (M,3), n_p).  Dense; for tests only."""
    ys, X = np.asarray(ys, F32), np.asarray(X, F32)
    M, N = len(ys), len(X)
    arg = -sqdist_f32(ys, X).astype(np.float64) / (2.0 * sigma2)
    k = np.where(arg >= FLUSH_ARG, np.exp(arg), 0.0)
    den = k.sum(0)
    den[den == 0.0] = FLT_EPSILON
    r = den + const_c(sigma2, w, M, N)
    p = k / r
    p1 = p.sum(1)
    return den / r, p1, p @ X.astype(np.float64), float(p1.sum())


def estep_matrix_free(ys, X, sigma2, w):
    """The same sums by a column sweep and a row sweep: O(M + N) memory."""
    ys, X = np.asarray(ys, F32), np.asarray(X, F32)
    M, N = len(ys), len(X)
    X64 = X.astype(np.float64)
    c = const_c(sigma2, w, M, N)

    def kern(a, B):    # one point against a cloud
        dx, dy, dz = a[0] - B[:, 0], a[1] - B[:, 1], a[2] - B[:, 2]
        arg = -((dx * dx + dy * dy) + dz * dz).astype(np.float64) / (2.0 * sigma2)
        return np.where(arg >= FLUSH_ARG, np.exp(arg), 0.0)

    den = np.array([kern(X[n], ys).sum() for n in range(N)])
    den[den == 0.0] = FLT_EPSILON
    inv = 1.0 / (den + c)
    p1, px = np.empty(M), np.empty((M, 3))
    for m in range(M):
        v = kern(ys[m], X) * inv
        p1[m] = v.sum()
        px[m] = v @ X64
    return den * inv, p1, px, float(p1.sum())


def estep_f32(ys, X, sigma2, w):
    """probreg's dense formulation evaluated in f32 (numpy, CPU): distances, one
    exp over the (M, N) matrix, column sums, the FLT_EPSILON rule, one divide,
    two reductions and a matrix product, every array f32."""
    ys, X = np.asarray(ys, F32), np.asarray(X, F32)
    M, N = len(ys), len(X)
    pmat = np.exp(-sqdist_f32(ys, X) / F32(2.0 * sigma2))
    den = pmat.sum(0)
    den[den == 0] = F32(FLT_EPSILON)
    r = den + F32(const_c(sigma2, w, M, N))
    pmat = pmat / r
    p1 = pmat.sum(1)
    assert pmat.dtype == F32 and p1.dtype == F32
    return den / r, p1, pmat @ X, float(p1.astype(np.float64).sum())


def rotation_of(A):
    """argmax tr(A^T R) over rotations: U diag(1, 1, det(U V^T)) V^T."""
    U, _, Vt = np.linalg.svd(A)
    C = np.diag([1.0, 1.0, np.linalg.det(U @ Vt)])
    return U @ C @ Vt


def mstep(kind, Y, X, pt1, p1, px):
    """The rigid / rigid + scale / affine M-step in f64.  Returns (B, t, scale,
    sigma2, q) with sigma2 floored at FLT_EPSILON before q."""
    Y, X = np.asarray(Y, np.float64), np.asarray(X, np.float64)
    pt1, p1, px = (np.asarray(a, np.float64) for a in (pt1, p1, px))
    n_p = p1.sum()
    mux, muy = px.sum(0) / n_p, Y.T @ p1 / n_p
    Yc, Xc = Y - muy, X - mux
    A = px.T @ Yc - np.outer(mux, p1 @ Yc)
    G = Yc.T @ (p1[:, None] * Yc)
    tr_xpx = float(pt1 @ (Xc * Xc).sum(1))
    scale = 1.0
    with np.errstate(all="ignore"):
        if kind == AFFINE:
            B = np.linalg.solve(G.T, A.T).T
            tr_ab = float((A * B).sum())
            sigma2 = (tr_xpx - tr_ab) / (3.0 * n_p)
            resid = tr_xpx - 2.0 * tr_ab + float(np.trace(B @ G @ B.T))
        else:
            R = rotation_of(A)
            tr_ar, tr_g = float((A * R).sum()), float(np.trace(G))
            if kind == RIGID_SCALE:
                scale = tr_ar / tr_g
                sigma2 = (tr_xpx - scale * tr_ar) / (3.0 * n_p)
            else:
                sigma2 = (tr_xpx - 2.0 * tr_ar + tr_g) / (3.0 * n_p)
            B = scale * R
            resid = tr_xpx - 2.0 * scale * tr_ar + scale * scale * tr_g
        if sigma2 < FLT_EPSILON:
            sigma2 = FLT_EPSILON
        q = resid / (2.0 * sigma2) + 1.5 * n_p * np.log(sigma2)
    return B, mux - B @ muy, scale, float(sigma2), float(q)


def register(Y, X, kind, w=0.0, maxiter=50, tol=1e-3, init=None, estep_fn=estep):
    """The loop of pcr_cpd_register.  Returns a dict: T (4,4), scale, sigma2, q,
    iters (iterations run), status, and the traces `qs` (q per iteration),
    `colmax` (per iteration every target's largest exponent argument) and
    `min_colmax` (its smallest value per iteration)."""
    Y, X = np.asarray(Y, F32), np.asarray(X, F32)
    T = np.eye(4) if init is None else np.array(init, np.float64).reshape(4, 4)
    T[3] = (0.0, 0.0, 0.0, 1.0)
    out = dict(T=T, scale=1.0, sigma2=0.0, q=0.0, iters=0, status=0, qs=[], colmax=[], min_colmax=[])
    if len(Y) == 0 or len(X) == 0:
        out["status"] = 1
        return out
    sigma2 = out["sigma2"] = initial_sigma2(Y, X)
    for it in range(maxiter):
        ys = apply_T(T, Y)
        out["colmax"].append(column_max_args(ys, X, sigma2))
        out["min_colmax"].append(float(out["colmax"][-1].min()))
        pt1, p1, px, _ = estep_fn(ys, X, sigma2, w)
        with np.errstate(all="ignore"):
            B, t, scale, sigma2, q = mstep(kind, Y, X, pt1, p1, px)
        out.update(sigma2=sigma2, q=q, iters=it + 1)
        if not (np.isfinite(sigma2) and np.isfinite(q)):
            out["status"] = 2
            break
        T[:3, :3], T[:3, 3] = B, t
        out["scale"] = scale
        out["qs"].append(q)
        if it >= 1 and abs(q - out["qs"][-2]) < tol:
            break
    return out


def gram(Y, beta):
    Y = np.asarray(Y, np.float64)
    d = ((Y[:, None, :] - Y[None, :, :]) ** 2).sum(2)
    return np.exp(-d / (2.0 * beta * beta))


def nonrigid(Y, X, beta=2.0, lmd=2.0, w=0.0, maxiter=50, tol=1e-3, estep_fn=estep):
    """Non-rigid CPD: (dP1 G + lmd sigma2 I) W = PX - dP1 Y, T(Y) = Y + G W, the
    paper's sigma2 and q (with the regulariser lmd / 2 tr(W^T G W))."""
    Y32, X = np.asarray(Y, F32), np.asarray(X, F32)
    Y, X64 = Y32.astype(np.float64), X.astype(np.float64)
    M = len(Y)
    G = gram(Y, beta)
    W = np.zeros((M, 3))
    sigma2 = initial_sigma2(Y32, X)
    out = dict(g=G, w=W, sigma2=sigma2, q=0.0, iters=0, qs=[])
    for it in range(maxiter):
        ys = (Y + G @ W).astype(F32)
        pt1, p1, px, _ = (np.asarray(a, np.float64) if np.ndim(a) else a for a in estep_fn(ys, X, sigma2, w))
        n_p = p1.sum()
        W = np.linalg.solve(p1[:, None] * G + lmd * sigma2 * np.eye(M), px - p1[:, None] * Y)
        TY = Y + G @ W
        resid = float(pt1 @ (X64 * X64).sum(1)) - 2.0 * float((px * TY).sum()) + float(p1 @ (TY * TY).sum(1))
        sigma2 = max(resid / (3.0 * n_p), FLT_EPSILON)
        q = resid / (2.0 * sigma2) + 1.5 * n_p * np.log(sigma2) + 0.5 * lmd * float((W * (G @ W)).sum())
        out.update(w=W, sigma2=float(sigma2), q=float(q), iters=it + 1)
        out["qs"].append(float(q))
        if it >= 1 and abs(q - out["qs"][-2]) < tol:
            break
    return out


def rel_err(got, want):
    """max |got - want| over the largest magnitude of `want` (1 if that is 0)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    s = float(np.abs(want).max()) if want.size else 0.0
    return float(np.abs(got - want).max() / (s if s > 0 else 1.0)) if want.size else 0.0


def rot_z(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def stop_rule_pair(seed=3, angle=0.5):
    """The stop-rule pair of the GPU tests: a 65-point rotated, shifted, noisy
    subset of 130 uniform points."""
    rng = np.random.default_rng(seed)
    x = rng.random((130, 3))
    idx = rng.permutation(130)[:65]
    y = (x[idx] - np.array([0.1, 0.2, -0.1])) @ rot_z(angle) + rng.normal(0.0, 0.002, (65, 3))
    return y.astype(F32), x.astype(F32)
