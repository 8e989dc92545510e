"""Independent references for the f1 kernels (hybrid search, normals, SPFH/FPFH):
plain numpy in f64, built from the published algorithms, sharing no code with
oracle/fpfh_oracle.c or csrc/fpfh.hip."""
import math

import numpy as np


def brute_hybrid(p, r, K):
    """KDTreeFlann::SearchHybrid(p[i], r, K) for every point by brute force:
    (idx (n,K) int32 -1 padded, d2 (n,K) f64 0 padded, cnt (n,), full_cnt (n,)).
    In radius means d2 < (double)(float)(r*r) strictly, d2 = ((dx^2 + dy^2) + dz^2) on
    the f64 of the f32 points; the order is (d2, index); full_cnt is the uncut count."""
    P = np.ascontiguousarray(p, np.float32).reshape(-1, 3).astype(np.float64)
    n = len(P)
    thr = float(np.float32(r * r))
    idx = np.full((n, K), -1, np.int32)
    d2 = np.zeros((n, K), np.float64)
    cnt = np.zeros(n, np.int32)
    full = np.zeros(n, np.int32)
    for i0 in range(0, n, 512):
        Q = P[i0:i0 + 512, None, :]
        with np.errstate(invalid="ignore", over="ignore"):   # NaN / inf points see nothing
            dx, dy, dz = Q[..., 0] - P[None, :, 0], Q[..., 1] - P[None, :, 1], Q[..., 2] - P[None, :, 2]
            D = (dx * dx + dy * dy) + dz * dz
            inr = D < thr
        for a in range(len(D)):
            j = np.nonzero(inr[a])[0]
            o = np.lexsort((j, D[a, j]))[:K]
            i = i0 + a
            full[i] = len(j)
            cnt[i] = len(o)
            idx[i, :len(o)] = j[o]
            d2[i, :len(o)] = D[a, j[o]]
    return idx, d2, cnt, full


def eigh_normals(p, idx, cnt):
    """The eigenvector of the smallest eigenvalue of each list's centred covariance
    (np.linalg.eigh): (v0 (n,3), ok (n,)).  ok is false where the list has fewer than
    3 points or the two smallest eigenvalues are too close for v0 to be unique
    (w1 - w0 < 1e-6 * max(w2, 1e-300))."""
    P = np.ascontiguousarray(p, np.float32).reshape(-1, 3).astype(np.float64)
    n = len(P)
    C = np.zeros((n, 3, 3))
    for i in range(n):
        k = int(cnt[i])
        if k >= 3:
            q = P[idx[i, :k]]
            q = q - q.mean(0)
            C[i] = q.T @ q / k
    w, V = np.linalg.eigh(C)
    ok = (np.asarray(cnt) >= 3) & ~(w[:, 1] - w[:, 0] < 1e-6 * np.maximum(w[:, 2], 1e-300))
    return V[:, :, 0].copy(), ok


def numpy_fpfh(p, nm, idx, d2, cnt):
    """Second, independent implementation (libm math) of Feature.cpp's SPFH/FPFH."""
    n = len(p)
    P = p.astype(np.float64)
    sp = np.zeros((n, 33))
    for i in range(n):
        k = cnt[i]
        if k <= 1:
            continue
        for j in idx[i, 1:k]:
            dp = P[j] - P[i]
            f3 = math.sqrt(dp @ dp)
            f = [0.0, 0.0, 0.0]
            if f3 != 0.0:
                n1, n2 = nm[i], nm[j]
                a1, a2 = (n1 @ dp) / f3, (n2 @ dp) / f3
                if math.acos(abs(a1)) > math.acos(abs(a2)):
                    n1, n2, dp, f2 = n2, n1, -dp, -a2
                else:
                    f2 = a1
                v = np.cross(dp, n1)
                vn = math.sqrt(v @ v)
                if vn != 0.0:
                    v = v / vn
                    w = np.cross(n1, v)
                    f = [math.atan2(w @ n2, n1 @ n2), v @ n2, f2]
            h = [int(math.floor(11 * (f[0] + math.pi) / (2 * math.pi))),
                 int(math.floor(11 * (f[1] + 1.0) * 0.5)), int(math.floor(11 * (f[2] + 1.0) * 0.5))]
            for g in range(3):
                sp[i, 11 * g + min(max(h[g], 0), 10)] += 100.0 / (k - 1)
    fp = np.zeros((n, 33))
    for i in range(n):
        k = cnt[i]
        if k <= 1:
            continue
        acc = np.zeros(33)
        for j, dd in zip(idx[i, 1:k], d2[i, 1:k]):
            if dd != 0.0:
                acc += sp[j] / dd
        s = acc.reshape(3, 11).sum(1)
        s = np.where(s != 0, 100.0 / np.where(s != 0, s, 1), 0.0)
        fp[i] = acc * np.repeat(s, 11) + sp[i]
    return sp, fp
