"""Point-to-plane ICP with robust kernels: the f64 contract of csrc/icp_plane.hip.

A restatement of Open3D 0.13's RegistrationICP with TransformationEstimationPointToPlane
(and its RobustKernel weights) written from memory; parity against Open3D itself is not
pinned.  The loop is the oracle's icp_core (oracle/pcr_oracle.c) with the
Umeyama step replaced by plane_update below; the correspondence search is the oracle's own
(oracle.radius_nn), so its semantics -- d2 < (double)(float)(d*d) strictly, lowest index on
ties -- are literally the oracle's.

Everything is f64 with every operation rounded on its own (numpy and Python floats do not
fuse; the library is built with -ffp-contract=off).  Element-wise numpy expressions below
are the scalar expressions of the kernel applied per correspondence.

The exact sums.  Per correspondence (s the moved source point, t its target, n the target's
normal): e = s - t, r = (e0 n0 + e1 n1) + e2 n2, c = s x n, J = (c, n), w = weight(r).  The
normal equations take 21 sums A_ab += q((w J_a) J_b), a <= b, and 6 sums g_a += q((w J_a) r),
where q(x) = trunc(x 2^k) 2^-k.  quantum_exponent() chooses k so that the 27 sums are exact
in f64 in any order.  Proof (u = 2^-53):
  * An inlier lies within sqrt(thr) <= d (1 + 2^-23) of its target, so |s|_inf <= bt + 2d
    =: Bs with room to spare, bt = max_j |t_j|_inf over all targets.
  * With N = max |n_j|_inf over the normals whose three components are finite (the others
    contribute nothing): |c_a| = |s_b n_c - s_c n_b| <= 2 Bs N, |n_a| <= N, and by
    Cauchy-Schwarz |r| <= |e|_2 |n|_2 < sqrt(3) d N (1 + 2^-23) < 2 d N <= Bs N.  So every
    |J_a| and |r| is at most Jm = N max(2 Bs, 1), up to the roundings of the three or four
    operations that computed it: a factor below 1 + 8u, Jm's own rounding included.
  * w <= W, the kernel's supremum weight (1, or 1/k for GM, whose computed weight
    k / ((k + r^2)(k + r^2)) can exceed the computed 1/k by a few u at most).
  * A term fl(fl(w J_a) X) is therefore below W Jm^2 (1 + 32u) in magnitude.  With
    W < 2^eW and Jm < 2^eJ from frexp, it is below 2^e_max, e_max = eW + 2 eJ + 1: the
    + 1 pays for the roundings.
  * n <= 2^e_n terms, k = 52 - e_n - e_max: x 2^k is exact (a power of two; the clamp of k
    to +-200 keeps it from overflowing, and where it underflows the truncation is 0 either
    way), trunc gives an integer below 2^(e_max + k), and any partial sum of at most n of
    them is an integer below 2^(e_n + e_max + k) = 2^52.  Integers below 2^53 add exactly
    in f64, so the sums do not depend on the order, and scaling by 2^-k is exact.
The clamp at -200 would break the bound for coordinates beyond 2^100; such inputs are
outside the contract.

The solve is LDL^T without pivoting in the loop order of ldlt_solve; a pivot that is not
> 0 or not finite, or a non-finite solution, makes the update the identity.
"""
import math

import numpy as np

import oracle

KERNEL_IDS = {"l2": 0, "huber": 1, "cauchy": 2, "gm": 3, "tukey": 4}

# ---------------------------------------------------------------------------
# deterministic sine / cosine: + - * / and trunc only
# ---------------------------------------------------------------------------

TWO_OVER_PI = 6.36619772367581382433e-01
PIO2_HI = 1.57079632673412561417e+00   # the first 33 bits of pi/2: j * PIO2_HI is exact for j < 2^20
PIO2_LO = 6.07710050650619224932e-11   # pi/2 - PIO2_HI, rounded


def _cos_poly(x):
    """|x| <= pi/4 (and a little past it): the nested Taylor form to x^20, as det_cos_poly
    of oracle/fpfh_oracle.c."""
    x2 = x * x
    s = 1.0
    for k in range(10, 0, -1):
        s = 1.0 - x2 / float((2 * k - 1) * (2 * k)) * s
    return s


def _sin_poly(x):
    x2 = x * x
    s = 1.0
    for k in range(10, 0, -1):
        s = 1.0 - x2 / float((2 * k) * (2 * k + 1)) * s
    return x * s


def det_sincos(x):
    """(sin x, cos x) for every finite x (NaN, NaN otherwise).  a = |x|; j = trunc(a * 2/pi
    + 0.5) quarter turns are taken off in two steps, y = (a - j PIO2_HI) - j PIO2_LO, which
    leaves |y| <= pi/4 (up to the reduction's rounding); the quadrant j mod 4 = j - 4
    trunc(j / 4) picks the polynomial and the signs; sin is odd in x."""
    if not math.isfinite(x):
        return math.nan, math.nan
    a = abs(x)
    j = float(math.trunc(a * TWO_OVER_PI + 0.5))
    y = (a - j * PIO2_HI) - j * PIO2_LO
    q = j - 4.0 * float(math.trunc(j / 4.0))
    sp, cp = _sin_poly(y), _cos_poly(y)
    if q == 0.0:
        s, c = sp, cp
    elif q == 1.0:
        s, c = cp, -sp
    elif q == 2.0:
        s, c = -sp, -cp
    else:
        s, c = -cp, sp
    if x < 0.0:
        s = -s
    return s, c


# ---------------------------------------------------------------------------
# robust kernels
# ---------------------------------------------------------------------------


def weight(kernel, k, r):
    """The kernel's weight of the residuals r (array), per element as the scalar code."""
    r = np.asarray(r, np.float64)
    a = np.abs(r)
    with np.errstate(all="ignore"):
        if kernel == "l2":
            return np.ones_like(r)
        if kernel == "huber":
            return np.where(a <= k, 1.0, k / a)
        if kernel == "cauchy":
            return 1.0 / (1.0 + (r / k) * (r / k))
        if kernel == "gm":
            return k / ((k + r * r) * (k + r * r))
        if kernel == "tukey":
            t = 1.0 - (r / k) * (r / k)
            return np.where(a <= k, t * t, 0.0)
    raise KeyError(kernel)


def weight_sup(kernel, k):
    return 1.0 / k if kernel == "gm" else 1.0


# ---------------------------------------------------------------------------
# the quantum and the 27 sums
# ---------------------------------------------------------------------------


def quantum_exponent(tgt, nrm, n, d, W):
    """k of the quantum 2^-k (see the module docstring).  tgt, nrm: (m, 3) f64."""
    bt = 0.0
    for v in np.abs(tgt).reshape(-1):
        if v > bt:
            bt = float(v)
    N = 0.0
    fin = np.isfinite(nrm).all(axis=1)
    for v in np.abs(nrm[fin]).reshape(-1):
        if v > N:
            N = float(v)
    Bs = bt + 2.0 * d
    two = 2.0 * Bs
    Jm = N * (two if two > 1.0 else 1.0)
    eJ = math.frexp(Jm)[1]
    eW = math.frexp(W)[1]
    emax = eW + 2 * eJ + 1
    en = 0
    while (1 << en) < max(n, 1):
        en += 1
    return max(-200, min(200, 52 - en - emax))


PAIRS = [(a, b) for a in range(6) for b in range(a, 6)]   # the 21 sums' order


def plane_terms(P, tgt, nrm, cj, kernel, kk):
    """The unquantised terms of the contributing correspondences: (K, 27) f64 -- 21 of A
    in PAIRS' order, then 6 of g -- with J (K, 6), r (K,), w (K,)."""
    i = np.nonzero(cj >= 0)[0]
    s, t, n = P[i], tgt[cj[i]], nrm[cj[i]]
    with np.errstate(all="ignore"):
        e = s - t
        r = (e[:, 0] * n[:, 0] + e[:, 1] * n[:, 1]) + e[:, 2] * n[:, 2]
        c0 = s[:, 1] * n[:, 2] - s[:, 2] * n[:, 1]
        c1 = s[:, 2] * n[:, 0] - s[:, 0] * n[:, 2]
        c2 = s[:, 0] * n[:, 1] - s[:, 1] * n[:, 0]
        J = np.stack([c0, c1, c2, n[:, 0], n[:, 1], n[:, 2]], axis=1)
        w = weight(kernel, kk, r)
        keep = np.isfinite(n).all(axis=1) & np.isfinite(w)
        J, r, w = J[keep], r[keep], w[keep]
        wJ = w[:, None] * J
        cols = [wJ[:, a] * J[:, b] for a, b in PAIRS] + [wJ[:, a] * r for a in range(6)]
    return np.stack(cols, axis=1).reshape(-1, 27), J, r, w


def quantise(terms, k):
    """trunc(x 2^k) per term: the terms in quanta (integer-valued f64)."""
    return np.trunc(terms * math.ldexp(1.0, k))


def plane_sums(P, tgt, nrm, cj, kernel, kk, k):
    """(A21, g6): the 27 exact sums.  0.0 + ...: a sum of nothing but -0.0 is +0.0, as an
    accumulator that starts at +0.0 leaves it."""
    q = quantise(plane_terms(P, tgt, nrm, cj, kernel, kk)[0], k)
    tot = (0.0 + q.sum(axis=0)) * math.ldexp(1.0, -k)
    return tot[:21], tot[21:]


def ldlt_solve(A21, g6):
    """x of A x = -g by LDL^T without pivoting, or None.  The loop order is the contract."""
    A = [[0.0] * 6 for _ in range(6)]
    for q, (a, b) in enumerate(PAIRS):
        A[a][b] = A[b][a] = float(A21[q])
    L = [[0.0] * 6 for _ in range(6)]
    D = [0.0] * 6
    for j in range(6):
        dj = A[j][j]
        for k in range(j):
            dj = dj - (L[j][k] * D[k]) * L[j][k]
        if not (dj > 0.0) or not math.isfinite(dj):
            return None
        D[j] = dj
        for i in range(j + 1, 6):
            v = A[i][j]
            for k in range(j):
                v = v - (L[i][k] * D[k]) * L[j][k]
            L[i][j] = v / dj
    y = [0.0] * 6
    for i in range(6):
        v = -float(g6[i])
        for k in range(i):
            v = v - L[i][k] * y[k]
        y[i] = v
    x = [0.0] * 6
    for i in range(5, -1, -1):
        v = y[i] / D[i]
        for k in range(i + 1, 6):
            v = v - L[k][i] * x[k]
        x[i] = v
    if not all(math.isfinite(v) for v in x):
        return None
    return x


IDENTITY12 = [1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0]


def update_from_x(x):
    """U = [Rz(gamma) Ry(beta) Rx(alpha) | (tx, ty, tz)], row-major 3 x 4, the rotation's
    entries in this written form."""
    if x is None:
        return list(IDENTITY12)
    sa, ca = det_sincos(x[0])
    sb, cb = det_sincos(x[1])
    sg, cg = det_sincos(x[2])
    return [cg * cb, (cg * sb) * sa - sg * ca, (cg * sb) * ca + sg * sa, x[3],
            sg * cb, (sg * sb) * sa + cg * ca, (sg * sb) * ca - cg * sa, x[4],
            -sb, cb * sa, cb * ca, x[5]]


def plane_update(P, tgt, nrm, cj, kernel, kk, k):
    A21, g6 = plane_sums(P, tgt, nrm, cj, kernel, kk, k)
    return update_from_x(ldlt_solve(A21, g6))


# ---------------------------------------------------------------------------
# the loop (icp_core of oracle/pcr_oracle.c)
# ---------------------------------------------------------------------------


def _xform(U, P):
    x, y, z = P[:, 0].copy(), P[:, 1].copy(), P[:, 2].copy()
    return np.stack([((U[4 * r] * x + U[4 * r + 1] * y) + U[4 * r + 2] * z) + U[4 * r + 3]
                     for r in range(3)], axis=1)


def _evaluate(tgt, P, d, thr):
    cj, d2 = oracle.radius_nn(tgt, P, d)
    hit = cj >= 0
    cnt = int(hit.sum())
    if cnt == 0:
        return cj, 0, 0.0, 0.0
    scale = 1099511627776.0 / thr
    acc = sum(int(v) for v in d2[hit] * scale)
    return cj, cnt, float(cnt) / float(len(P)), math.sqrt((float(acc) / scale) / float(cnt))


def icp_plane(src, tgt, tgt_normals, d, init=None, kernel="l2", k=1.0, max_iteration=30,
              relative_fitness=1e-6, relative_rmse=1e-6, trace=None):
    """dict(T (4,4), fitness, inlier_rmse, iters, n_corr, corr_tgt (n,)).  trace (a list):
    gets one (P, cj, quantum exponent) per update computed."""
    src = np.ascontiguousarray(src, np.float32).reshape(-1, 3)
    tgt = np.ascontiguousarray(tgt, np.float32).reshape(-1, 3)
    nrm = np.ascontiguousarray(tgt_normals, np.float32).reshape(-1, 3).astype(np.float64)
    init = np.eye(4) if init is None else np.asarray(init, np.float64).reshape(4, 4)
    n, m = len(src), len(tgt)
    T = [float(v) for v in init.reshape(16)]
    out = dict(T=np.array(T).reshape(4, 4), fitness=0.0, inlier_rmse=0.0, iters=0, n_corr=0,
               corr_tgt=np.full(n, -1, np.int32))
    if not (d > 0.0) or n <= 0 or m <= 0:
        return out
    P = src.astype(np.float64)
    Tg = tgt.astype(np.float64)
    thr = float(np.float32(d * d))
    if not np.array_equal(init, np.eye(4)):
        P = _xform(T[:12], P)
    kq = quantum_exponent(Tg, nrm, n, d, weight_sup(kernel, k))
    cj, cnt, fit, rmse = _evaluate(Tg, P, d, thr)
    it = 0
    while it < max_iteration:
        if cnt == 0:
            break
        if trace is not None:
            trace.append((P.copy(), cj.copy(), kq))
        U = plane_update(P, Tg, nrm, cj, kernel, k, kq)
        U16 = U + [0.0, 0.0, 0.0, 1.0]
        T = [((U16[4 * a] * T[b] + U16[4 * a + 1] * T[4 + b]) + U16[4 * a + 2] * T[8 + b])
             + U16[4 * a + 3] * T[12 + b] for a in range(4) for b in range(4)]
        P = _xform(U, P)
        pf, pr = fit, rmse
        cj, cnt, fit, rmse = _evaluate(Tg, P, d, thr)
        it += 1
        if abs(pf - fit) < relative_fitness and abs(pr - rmse) < relative_rmse:
            break
    return dict(T=np.array(T).reshape(4, 4), fitness=fit, inlier_rmse=rmse, iters=it, n_corr=cnt,
                corr_tgt=cj.astype(np.int32))
