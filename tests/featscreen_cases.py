"""Inputs and a numpy model for the tests of the 1-term feature screen's bias and
certificates (csrc/featnn_pack.hip, featnn_row.hip: feat_sample / feat_pack5 / feat_colterms /
row_tail).  No GPU here: test_featscreen_model_cpu.py checks on any machine that
the generated cases are adversarial, the *_gpu.py files run them.

The model restates, in numpy, only what the kernels define as arithmetic:
  split5_params, pair_scale5, the sample / repair choice of the pair's scale s
  (a power of two), f16(x s), |x s - f16(x s)|, and row_tail's kCT bound `bnd`.
"""
import numpy as np

U = 2.0 ** -24
K_SAMPLE_ROWS = 64
K_SPEC_MARGIN = 1


def mut_scratch(P, Nmax, Mmax):
    """Named views of the scratch of the last pcr_feature_correspondences call at
    D <= 64, read through pcr_featmut_debug_copy (needs the GPU).  The one copy of
    feature_corres_v5's layout (csrc/featnn.hip) on the test side: each array at
    the next multiple of its element's alignment, in the order of its take()s --
      v12 [P][Nmax] f64, e12 [P][Nmax] f32, wq [P][Mmax][4] f32 (16-byte aligned),
      used, pos [P][Mmax + 1] i32, jlist, nn21x [P][Mmax] i32, flag [P][Nmax + 1]
      i32, nj [P] i32.
    used / pos / flag keep their per-pair extra element."""
    import torch
    from pointcloudregistration_amd import _lib
    fields = (("v12", np.float64, (P, Nmax), 8), ("e12", np.float32, (P, Nmax), 4),
              ("wq", np.float32, (P, Mmax, 4), 16), ("used", np.int32, (P, Mmax + 1), 4),
              ("pos", np.int32, (P, Mmax + 1), 4), ("jlist", np.int32, (P, Mmax), 4),
              ("nn21x", np.int32, (P, Mmax), 4), ("flag", np.int32, (P, Nmax + 1), 4), ("nj", np.int32, (P,), 4))
    at, end = {}, 0
    for name, dt, shape, align in fields:
        at[name] = (end + align - 1) // align * align
        end = at[name] + int(np.prod(shape)) * np.dtype(dt).itemsize
    buf = torch.empty(end, dtype=torch.uint8, device="cuda")
    _lib.call("pcr_featmut_debug_copy", buf.data_ptr(), buf.numel(), _lib.stream_handle())
    torch.cuda.synchronize()
    raw = buf.cpu().numpy()
    return {name: raw[at[name]:at[name] + int(np.prod(shape)) * np.dtype(dt).itemsize].view(dt).reshape(shape)
            for name, dt, shape, align in fields}


def split5_params(D):
    L = 0
    while (1 << L) < D:
        L += 1
    T = min((30 - L) // 2, 12)
    return T, 2 * T + L - 15


def pair_scale5(m, T):
    """featnn_v5.h pair_scale5: 2^e with max * 2^e in [2^(T-1), 2^T)."""
    bits = int(np.float32(m).view(np.uint32))
    E = (bits >> 23) & 0xff
    if E == 0 or E == 255:
        return 1.0
    return 2.0 ** min(max(T + 126 - E, -126), 127)


def _fmax_abs(x):
    """fmaxf chain over |x| from 0: NaN operands are ignored, inf is kept."""
    a = np.abs(x[~np.isnan(x)])
    return np.float32(a.max()) if a.size else np.float32(0.0)


def pair_scale(F, G):
    """-> (s, flagged): the scale the packs end up using for the pair (feat_sample's
    speculative one unless a row leaves the split's range, then feat_maxabs')."""
    T, _ = split5_params(F.shape[1])
    smax = max(_fmax_abs(F[:K_SAMPLE_ROWS]), _fmax_abs(G[:K_SAMPLE_ROWS]))
    s0 = pair_scale5(smax, T - K_SPEC_MARGIN)
    with np.errstate(all="ignore"):
        ok = all(bool(np.all(np.abs(X * np.float32(s0)) < 2.0 ** T)) for X in (F, G))
    if ok:
        return s0, False
    return pair_scale5(max(_fmax_abs(F), _fmax_abs(G)), T), True


def scaled_terms(X, s):
    """per row of the cloud (f64): |x s|^2, |f16(x s)|^2, |x s - f16(x s)| (the
    pack's rex, rounded as split_err_norm), |x s| as the pack's f32 norm."""
    with np.errstate(all="ignore"):
        xs = X.astype(np.float32) * np.float32(s)
        h = xs.astype(np.float16).astype(np.float64)
        xd = xs.astype(np.float64)
        n2 = (xd * xd).sum(1)
        h2 = (h * h).sum(1)
        ex = np.sqrt(((xd - h) ** 2).sum(1)) * (1.0 + 1e-6)
        return n2, h2, ex.astype(np.float32).astype(np.float64), np.sqrt(n2).astype(np.float32).astype(np.float64)


def bias_upper(M):
    """A power of two at or above every bias rule in play for max norm M (the
    smallest power of two above M^2 (1 + 2^-18) + 1, and twice that): the bounds
    grow with B, so a precondition evaluated at this B holds at the kernel's."""
    return 4.0 * 2.0 ** np.ceil(np.log2(M * M * (1 + 2.0 ** -18) + 1.0))


def bnd_ct(qn, rex, Gm, cemax, B, D):
    """row_tail's kCT `bnd` (= 2 x the per-value error bound) of a row with scaled
    norm qn and split error rex against columns of max norm Gm / max split error
    cemax, bias B; and `ebias`.  NX = S = ceil(D / 16) executed k-chunks."""
    S = (D + 15) // 16
    sub = 2.0 ** -14 * np.sqrt(float(D))
    ex, E = rex + sub, cemax + sub
    err = (2.0 * (16 * S + 2) * U * ((B + Gm * Gm) + 2.0 * (qn + ex) * (Gm + E))
           + 2.0 * (ex * Gm + (qn + ex) * E) + U * (2.0 * B + Gm * Gm) * (1.0 + 2.0 ** -20) + 4.0)
    return 2.0 * err, U * (2.0 * B + qn * qn) * (1.0 + 2.0 ** -20)


def exact_dist(X, Y):
    """[N][M] f64 squared distances of the f32 rows (differences formed in f64,
    exact; summed in f64)."""
    X = np.asarray(X, np.float64)
    Y = np.asarray(Y, np.float64)
    out = np.empty((len(X), len(Y)))
    step = max(1, (1 << 22) // max(1, len(Y) * X.shape[1]))
    with np.errstate(all="ignore"):
        for i in range(0, len(X), step):
            d = X[i:i + step, None, :] - Y[None, :, :]
            out[i:i + step] = np.einsum("ijk,ijk->ij", d, d)
    return out


# ---------------------------------------------------------------------------
# A. boundary rows: every |element| = a = 2^j (1 - 2^-t), so D a^2 s^2 sits just
# below a power of two while f16(a s) rounds UP to the power of two itself
# ---------------------------------------------------------------------------
def boundary_pair(seed, D, t, j=0, K=48, N=520, M=480, where="sample", swap=False, twins=True):
    """-> dict(F, G, rows, twin, ...): K boundary rows in F (`where`: inside the
    first 64 rows, or only after row 64 behind small filler, which flags the pair
    for the repair pack), an exact copy of each in G at a permuted index (never
    index 0), Gaussian filler with norms <= 0.3 of the boundary norm.  D = 24
    keeps 16 non-zero elements per boundary row (D a^2 stays 2^4 a^2).  swap:
    the clouds exchanged (boundary rows in G, the twins in F)."""
    rng = np.random.default_rng(seed)
    nz = 16 if D == 24 else D
    a = np.float32(2.0 ** j * (1.0 - 2.0 ** -t))
    bn = float(a) * np.sqrt(nz)

    def filler(n):
        x = rng.standard_normal((n, D)) * (0.15 * float(a))
        x = np.clip(x, -0.9 * float(a), 0.9 * float(a))
        nr = np.sqrt((x * x).sum(1))
        x *= np.minimum(1.0, 0.29 * bn / nr)[:, None]
        return x.astype(np.float32)

    F, G = filler(N), filler(M)
    b = np.zeros((K, D), np.float32)
    b[:, :nz] = a * rng.choice(np.float32([-1.0, 1.0]), (K, nz))
    assert len(np.unique(b, axis=0)) == K
    if where == "sample":
        rows = np.sort(rng.permutation(np.arange(1, K_SAMPLE_ROWS))[:K])
        twin = rng.permutation(np.arange(1, M))[:K]
    else:
        F[:K_SAMPLE_ROWS + 16] *= np.float32(2.0 ** -6)
        G[:K_SAMPLE_ROWS + 16] *= np.float32(2.0 ** -6)
        rows = np.sort(rng.permutation(np.arange(K_SAMPLE_ROWS + 16, N))[:K])
        twin = rng.permutation(np.arange(K_SAMPLE_ROWS + 16, M))[:K]
    F[rows] = b
    if twins:
        G[twin] = b
    c = dict(F=F, G=G, rows=rows, twin=twin if twins else None, where=where, swap=swap, D=D, t=t)
    if swap:
        c["F"], c["G"] = G, F
    return c


def boundary_sides(c):
    """-> (X, Y, rows, twin): the cloud holding the boundary rows, the other one."""
    return (c["G"], c["F"], c["rows"], c["twin"]) if c["swap"] else (c["F"], c["G"], c["rows"], c["twin"])


def check_boundary_pair(c):
    """The case is adversarial whatever rule picks B: for each boundary row the
    screen's value against its twin, ct - 2 |f16(x s)|^2 with ct ~ |x s|^2 + B,
    falls below B - |x s|^2 by 2 (|f16(x s)|^2 - |x s|^2), more than the whole
    distance from |x s|^2 to the next power of two; and the row's exact runner-up
    gap is > 4 bnd, so a screen that loses the twin certifies the runner-up."""
    X, Y, rows, twin = boundary_sides(c)
    D = X.shape[1]
    s, flagged = pair_scale(c["F"], c["G"])
    assert flagged == (c["where"] != "sample"), (flagged, c["where"])
    n2x, h2x, exx, qx = scaled_terms(X, s)
    n2y, _, exy, qy = scaled_terms(Y, s)
    # the boundary rows carry both clouds' maximum norm
    assert n2x[rows].min() == n2x.max() and n2y.max() <= n2x.max()
    other = np.ones(len(X), bool)
    other[rows] = False
    assert n2x[other].max() <= 0.3 ** 2 * n2x.max()
    p2 = 2.0 ** np.ceil(np.log2(n2x[rows]))
    assert np.all(p2 > n2x[rows])
    assert np.all(2.0 * (h2x[rows] - n2x[rows]) > p2 - n2x[rows])
    if twin is None:
        return
    assert np.array_equal(X[rows], Y[twin]) and twin.min() > 0
    d = exact_dist(X[rows], Y) * s * s
    srt = np.sort(d, axis=1)
    assert np.array_equal(d.argmin(1), twin) and np.all(srt[:, 0] == 0.0)
    assert np.all(srt[:, 1] > 0.0)  # the twin is the row's only zero: no tie
    B = bias_upper(max(qx.max(), qy.max()))
    bnd, _ = bnd_ct(qx[rows], exx[rows], qy.max(), exy.max(), B, D)
    assert np.all(srt[:, 1] - srt[:, 0] > 4.0 * bnd), ((srt[:, 1] - srt[:, 0]).min(), bnd.max())
    # and the column direction (the twin as a pass-2 row against X's rows)
    dT = exact_dist(Y[twin], X) * s * s
    sT = np.sort(dT, axis=1)
    bndT, _ = bnd_ct(qy[twin], exy[twin], qx.max(), exx.max(), B, D)
    assert np.array_equal(dT.argmin(1), rows) and np.all(sT[:, 1] - sT[:, 0] > 4.0 * bndT)


def _bias_cases():
    c = {}
    ts = [12, 13, 14, 16]
    k = 0
    # (D, where, swap): sample = the boundary rows set feat_sample's speculative
    # scale; tail = the pair is flagged and takes the repair pack's full-max scale
    for D in (32, 16, 24):
        for where in ("sample", "tail"):
            for swap in (False, True):
                t = ts[k % 4]
                c[f"d{D}_{where}_{'g' if swap else 'f'}_t{t}"] = boundary_pair(900 + k, D, t, where=where, swap=swap)
                k += 1
    return c


BIAS_CASES = _bias_cases()


def bias_batch():
    """P = 5, per-pair B: boundary pairs at x 2^-9 and x 2^7, two ordinary random
    pairs, a pair whose boundary rows sit in G only (no twins)."""
    rng = np.random.default_rng(77)
    N, M, D = 520, 480, 32
    ps = [boundary_pair(31, D, 13, j=-9, N=N, M=M),
          dict(F=rng.standard_normal((N, D)).astype(np.float32), G=rng.standard_normal((M, D)).astype(np.float32)),
          boundary_pair(32, D, 12, j=7, N=N, M=M, where="tail"),
          dict(F=(rng.standard_normal((N, D)) * 30).astype(np.float32),
               G=(rng.standard_normal((M, D)) * 30).astype(np.float32)),
          boundary_pair(33, D, 14, N=M, M=N, swap=True, twins=False)]
    return ps, np.stack([p["F"] for p in ps]), np.stack([p["G"] for p in ps])


# ---------------------------------------------------------------------------
# B. a non-finite value in ONE cloud, whose finite rows are ~8x the other's
# ---------------------------------------------------------------------------
def onesided_pair(seed, bad, bad_row, side, full_twins, N=600, M=500, D=32):
    """The cloud `side` ('f' / 'g') holds one row with a `bad` (nan / inf) element
    at bad_row and finite rows of ~8x the other cloud's norm; the other cloud
    holds exact copies of 60 of them scaled by 1/8 (aligned: each is its big
    row's nearest, with a dot product far above the small cloud's |y|^2) and,
    with full_twins, 20 exact full-scale twins (its max norm equals the big
    cloud's)."""
    rng = np.random.default_rng(seed)
    big = (rng.standard_normal((N, D)) * 8.0).astype(np.float32)
    small = rng.standard_normal((M, D)).astype(np.float32)
    src = rng.permutation(np.arange(1, N))[:80]
    src = src[src != bad_row]
    top = int(np.argmax((big.astype(np.float64) ** 2).sum(1) * (np.arange(N) != bad_row)))
    src = np.concatenate([src[src != top][:60], [top], src[src != top][60:]])  # the max-norm row: a full twin
    dst = rng.permutation(np.arange(1, M))[:len(src)]
    small[dst[:60]] = big[src[:60]] * np.float32(0.125)
    if full_twins:
        small[dst[60:]] = big[src[60:]]
    big[bad_row, 5] = bad
    c = dict(F=big, G=small) if side == "f" else dict(F=small, G=big)
    c["full_twins"] = full_twins
    return c


def _onesided_cases():
    c = {}
    k = 0
    for side in ("f", "g"):
        # after row 64: the packs flag the pair (a non-finite element is outside
        # the split's range) and the repair takes the finite full max; inside the
        # sample: fmaxf drops the NaN from the sample max, the pack flags it again
        for bad_row, tag in ((300, "tail"), (10, "sample")):
            for full in (False, True):
                c[f"nan_{side}_{tag}{'_twins' if full else ''}"] = onesided_pair(40 + k, np.nan, bad_row, side, full)
                k += 1
        # inf: fmaxf keeps it, the cloud's max norm is +inf (finite-max test fails:
        # the pair's B is 2^60) and the pair's scale is 1
        c[f"inf_{side}_tail"] = onesided_pair(60 + k, np.inf, 300, side, False)
        c[f"inf_{side}_sample"] = onesided_pair(61 + k, -np.inf, 10, side, False)
        k += 2
    return c


ONESIDED_CASES = _onesided_cases()


def check_onesided_pair(c):
    """Without full-scale twins a bias sized from the finite cloud alone is below
    the big rows' |x s|^2: every aligned (1/8 copy) column's exact value
    |y|^2 + B - 2 x.y is negative for B up to 2x that cloud's own power of two.
    With them the finite cloud's max norm equals the big cloud's."""
    F, G = c["F"], c["G"]
    big, small = (F, G) if not np.isfinite(F).all() else (G, F)
    assert np.isfinite(small).all() and not np.isfinite(big).all()
    s, flagged = pair_scale(F, G)
    assert flagged
    fin = np.isfinite(big).all(1)
    n2b, _, _, _ = scaled_terms(big[fin], s)
    n2s, _, _, qs = scaled_terms(small, s)
    d = exact_dist(big[fin], small)
    j = d.argmin(1)
    al = np.array([np.array_equal(small[j[i]], big[fin][i] * np.float32(0.125)) for i in range(len(j))])
    assert al.sum() >= 50
    if c["full_twins"]:
        assert n2s.max() == n2b.max()
        return
    Bs = 2.0 * 2.0 ** np.ceil(np.log2(n2s.max()))
    dot = (big[fin][al].astype(np.float64) * small[j[al]].astype(np.float64)).sum(1) * s * s
    assert np.all(n2s[j[al]] + Bs - 2.0 * dot < 0.0)
