"""f64 restatement of the landmark term of the NDP level loss
(registration.py:213-227; include/pcr_api.h: pcr_ndp_ldmk_loss and the landmark
block of pcr_ndp_train), its gradient, the composed level loss, their derived
rounding bounds and the case lists of tests/test_ndp_ldmk_gpu.py.  numpy only;
the Chamfer and BCE parts are ndp_loop_ref.level_loss.  tests/
test_ndp_ldmk_ref_cpu.py pins the restatement to torch autograd in f64 and
checks every bound against torch in f32.

    loss_ldmk = mean_k sum_c (x[k][c] - t[k][c])^2                      (L landmarks)
    loss      = loss_ldmk + f32(w_cd) (sum(d1')/K + sum(d2')/M)          (mode A)
                [+ f32(w_reg) mean(-max(log(1 - s), -100)) over the P warped points]
    loss      = loss_ldmk [+ the same BCE term over P = L]               (mode B)
    dloss_ldmk/dx[k][c] = f32(2 / L) (x[k][c] - t[k][c])                 (f32: one
        subtraction, one product -- torch's f32 autograd bit for bit, it computes
        (1/L) (2 (x - t)) and the doubling is exact)

Bounds, in units u = 2^-24 as in ndp_loop_ref (nothing measured):
  * a landmark term sum_c (x - t)^2: 3 differences, 3 squares, 2 adds = 8
    roundings of a non-negative sum, 8 u of the term (0 when the differences and
    squares are exact: `terms_exact`);
  * the sum over the landmarks in pcr_ndp_ldmk_loss's order (the 32-block
    reduction of pcr_ndp_chamfer_loss): ndp_loop_ref.sum_roundings(L, "blocks") u
    of the sum (0 when ndp_loop_ref.sum_is_exact);
  * the Chamfer and BCE parts: ndp_loop_ref.loss_bound of them (w_cd <= 1 in
    every case, so the weighted Chamfer part's error is no larger; asserted);
  * composing: the division by L, f32(w_cd), its product and the two sums that
    join the parts: 5 u of the loss's magnitude (all parts are non-negative).
"""
import numpy as np

import ndp_loop_ref as loop

U, TINY, F32 = loop.U, loop.TINY, np.float32


def ldmk_terms(x, t):
    """sum_c (x - t)^2 per landmark, f64 on the f32 inputs."""
    e = np.asarray(x, F32).astype(np.float64) - np.asarray(t, F32).astype(np.float64)
    return (e * e).sum(-1).reshape(-1)


def ldmk_loss(x, t):
    terms = ldmk_terms(x, t)
    return float(terms.sum() / terms.size)


def ldmk_grad64(x, t):
    """d loss_ldmk / dx in f64: 2 / L (x - t)."""
    x, t = np.asarray(x, F32).astype(np.float64), np.asarray(t, F32).astype(np.float64)
    return 2.0 / x.shape[0] * (x - t)


def ldmk_grad32(x, t):
    """The stated f32 formula: f32(2 / L) * (x - t), one subtraction and one product."""
    x, t = np.asarray(x, F32), np.asarray(t, F32)
    return (F32(2.0 / x.shape[0]) * (x - t)).astype(F32)


def compose_g(x_out, tgt_ldmk, gsub, cd_scale):
    """dL/dx' (P, 3) f32 as the landmark block of pcr_ndp_train_backward defines it:
    rows < L the landmark gradient from x_out, rows >= L gsub f32(cd_scale) (zeros
    when gsub is None: no Chamfer part)."""
    x_out = np.asarray(x_out, F32)
    L = np.asarray(tgt_ldmk).shape[0]
    g = np.zeros_like(x_out)
    g[:L] = ldmk_grad32(x_out[:L], tgt_ldmk)
    if gsub is not None:
        g[L:] = (np.asarray(gsub, F32) * F32(cd_scale)).astype(F32)
    return g


def terms_exact(x, t):
    """True when no difference and no square rounds in f32."""
    x, t = np.asarray(x, F32), np.asarray(t, F32)
    e64 = x.astype(np.float64) - t.astype(np.float64)
    with np.errstate(all="ignore"):
        ok = np.array_equal(e64.astype(F32).astype(np.float64), e64)
        sq = e64 * e64
        return bool(ok and np.array_equal(sq.astype(F32).astype(np.float64), sq))


def level_loss(x, t, d1, d2, s, w_cd, w_reg=loop.W_REG, trunc=loop.TRUNC):
    """The composed loss.  d1 = d2 = None is mode B.  Returns a dict: loss, ldmk
    (the landmark part), terms, rest (ndp_loop_ref.level_loss of the other parts,
    None when there are none), cd (c1 + c2 or 0), w_cd (the f32 value)."""
    terms = ldmk_terms(x, t)
    with np.errstate(all="ignore"):
        out = dict(terms=terms, ldmk=float(terms.sum() / terms.size), w_cd=float(F32(w_cd)), cd=0.0, rest=None,
                   mode="B" if d1 is None else "A")
    loss = out["ldmk"]
    if d1 is not None:
        out["rest"] = loop.level_loss(d1, d2, s, w_reg, trunc)
        out["cd"] = out["rest"]["c1"] + out["rest"]["c2"]
        loss = loss + out["w_cd"] * out["cd"]
        if s is not None:
            loss = loss + out["rest"]["w"] * out["rest"]["bce"]
    elif s is not None:
        # only the BCE part of level_loss is used: one exact zero distance per side
        out["rest"] = loop.level_loss(np.zeros(1, F32), np.zeros(1, F32), s, w_reg, trunc)
        loss = loss + out["rest"]["w"] * out["rest"]["bce"]
    out["loss"] = float(loss)
    return out


def ldmk_bound(x, t):
    """|f32 landmark mean - ldmk_loss| without the final division: see the module
    docstring (8 u per term, sum_roundings u of the sum, each 0 when exact)."""
    terms = ldmk_terms(x, t)
    mean = np.abs(terms).sum() / terms.size
    r = 0 if terms_exact(x, t) else 8
    if not (r == 0 and loop.sum_is_exact(terms)):
        r += loop.sum_roundings(terms.size, "blocks")
    return r * U * mean


def loss_bound(ref, x, t):
    """|pcr_ndp_ldmk_loss - level_loss| for a finite loss."""
    assert ref["w_cd"] <= 1.0
    b = ldmk_bound(x, t)
    mag = ref["ldmk"]
    if ref["rest"] is not None:
        b += loop.loss_bound(ref["rest"], "blocks")
        mag += ref["w_cd"] * ref["cd"]
        if ref["rest"]["bce"] is not None:
            mag += ref["rest"]["w"] * abs(ref["rest"]["bce"])
    return b + 5.0 * U * mag + TINY


def guard_ratio(ref, x, t):
    """Smallest landmark term / L / the bound: how far above the bound the loss
    moves when one landmark is dropped or counted twice."""
    return float(ref["terms"].min() / ref["terms"].size / loss_bound(ref, x, t))


# --------------------------------------------------------------------------
# cases
# --------------------------------------------------------------------------

LDMK_SIZES = (1, 31, 32, 33, 255, 256, 257, 1025)
HOLD = 33                                   # K = M = P - L in mode A
W_CDS = (1.0, 0.5, 0.3)
REGIMES = ("draws", "nan", "trunc", "alltrunc")
# (L, N) of the backward cases: the landmark / sample boundary inside, at the edge
# of and just past a 32-point tile and the 128-point weight-gradient chunk
BWD_SHAPES = ((1, 1), (1, 40), (31, 1), (32, 32), (33, 31), (100, 60), (3, 0), (33, 0), (130, 0))
GUARD_MIN = 100.0


def make_ldmk(L, seed=0, nan=False):
    """(x, t) (L, 3) f32.  x on a grid of 1/2 in [-8, 8], t = x + e with |e| on a
    grid of 1/2 in [8, 16] and a drawn sign: differences and squares are exact,
    every term lies in [192, 768] on a grid of 1/4 and 1025 of them sum below
    2^24 / 4 (sum_is_exact), so the landmark part's bound is the composition's
    alone and one term in 1025 (>= 192 / 1025 of the mean) stays 100 x above it
    next to Chamfer parts of ndp_loop_ref.make_loss_case's scale."""
    rng = np.random.default_rng([20251021, L, seed])
    x = (rng.integers(-16, 17, (L, 3)) * 0.5).astype(F32)
    e = (rng.integers(16, 33, (L, 3)) * 0.5) * rng.choice([-1.0, 1.0], (L, 3))
    t = (x + e).astype(F32)
    if nan:
        t[L // 2, 1] = np.nan
    return x, t


def make_case(L, mode, regime):
    """(x, t, d1, d2, s): mode "A" with K = M = HOLD distances of make_loss_case's
    regime and s over P = L + HOLD, mode "B" with no distances and s over P = L.
    "alltrunc" carries no s: its loss is the landmark part alone."""
    x, t = make_ldmk(L, nan=regime == "nan")
    lreg = regime if regime in ("trunc", "alltrunc") else "draws"
    P = L + HOLD if mode == "A" else L
    d1, d2, s = loop.make_loss_case(HOLD, HOLD, P, lreg)
    if regime == "alltrunc":
        s = None
    if mode == "B":
        d1 = d2 = None
    return x, t, d1, d2, s
