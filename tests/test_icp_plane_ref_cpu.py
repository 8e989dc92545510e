"""CPU: the contract of point-to-plane ICP (tests/icp_plane_ref.py) checked on its own --
the 27 sums are exact, the estimator agrees with an independent least-squares solve, the
deterministic sine / cosine are accurate, the weights have their closed forms, degenerate
normal equations give the identity update, and the loop recovers a known motion."""
import math

import numpy as np
import pytest

import icp_plane_cases as pc
import icp_plane_ref as ref
import registration_cases as rc
from pointcloudregistration_amd import synth

U = 2.0 ** -53


def _states(name):
    """(case, P, cj, k) of every update the reference computes for copies 0 and 1."""
    c = pc.big_target_case() if name == "big_target" else pc.case(name)
    out = []
    for k in (0, 1):
        tr = []
        ref.icp_plane(c.src, c.tgt, c.nrm, c.d, init=rc.jitter_init(c.init, k), kernel=c.kernel, k=c.k,
                      trace=tr)
        out += [(c,) + s for s in tr]
    return out


@pytest.mark.parametrize("name", pc.CASES + ("big_target",))
def test_sums_are_exact_in_integers(name):
    """Every GPU case, every iteration: the terms in quanta are integers; the sum of their
    magnitudes stays below 2^52, so no partial sum in any order reaches it; the integer
    sums equal the f64 sums bit for bit, also in reversed and shuffled order."""
    rng = np.random.default_rng(3)
    for c, P, cj, k in _states(name):
        tgt, nrm = c.tgt.astype(np.float64), c.nrm.astype(np.float64)
        q = ref.quantise(ref.plane_terms(P, tgt, nrm, cj, c.kernel, c.k)[0], k)
        assert np.isfinite(q).all() and (q == np.trunc(q)).all()
        A, g = ref.plane_sums(P, tgt, nrm, cj, c.kernel, c.k, k)
        got = np.concatenate([A, g])
        for col in range(27):
            ints = [int(v) for v in q[:, col]]
            assert sum(abs(v) for v in ints) < 2 ** 52
            want = float(sum(ints)) * math.ldexp(1.0, -k)
            assert got[col] == want
        isk = math.ldexp(1.0, -k)
        for order in (np.arange(len(q))[::-1], rng.permutation(len(q))):
            tot = np.zeros(27)
            for row in q[order]:
                tot = tot + row
            assert (tot * isk).tobytes() == (got + 0.0).tobytes()


WELL_POSED = ("n63_m64", "n63_m777", "n65_m64", "n65_m777", "n1000_m64", "n1000_m777") + pc.KERNEL_CASES + \
    ("other_init", "nonunit", "nan_normal")


def _lstsq_gap(name):
    """max over the case's updates of (|x - x'|_2, its bound).  x' solves min |sqrt(w) (J x
    + r)| by numpy's SVD least squares on the unquantised rows.

    Bound.  Truncation moves each of the at most n terms of a sum by less than 2^-k, and
    the rounded products behind a term by 2u of its magnitude, so every entry of A and g
    moves by at most e = n 2^-k + 2u S, S the largest sum of term magnitudes: |dA|_2 <=
    |dA|_F <= 6 e, |dg|_2 <= sqrt(6) e.  First-order perturbation theory for A x = -g gives
    |dx| <= |A^-1| (|dA| |x| + |dg|) / (1 - |A^-1| |dA|); the factor 2 below covers the
    denominator (asserted).  Both solvers are backward stable: LDL^T of a positive definite
    6 x 6 matrix and the SVD solve each add at most c u cond(A) |x| with c of the order of
    the dimension squared; 100 u cond(A) |x| covers the two."""
    worst, room = 0.0, math.inf
    for c, P, cj, k in _states(name):
        tgt, nrm = c.tgt.astype(np.float64), c.nrm.astype(np.float64)
        terms, J, r, w = ref.plane_terms(P, tgt, nrm, cj, c.kernel, c.k)
        A21, g = ref.plane_sums(P, tgt, nrm, cj, c.kernel, c.k, k)
        x = ref.ldlt_solve(A21, g)
        assert x is not None
        x = np.array(x)
        sw = np.sqrt(w)
        xi = np.linalg.lstsq(sw[:, None] * J, -(sw * r), rcond=None)[0]
        A = np.zeros((6, 6))
        for q, (a, b) in enumerate(ref.PAIRS):
            A[a, b] = A[b, a] = A21[q]
        inv = np.linalg.norm(np.linalg.inv(A), 2)
        e = len(P) * math.ldexp(1.0, -k) + 2 * U * np.abs(terms).sum(axis=0).max()
        assert inv * 6 * e < 0.5
        bound = 2 * inv * (6 * e * np.linalg.norm(x) + math.sqrt(6) * e) + \
            100 * U * np.linalg.cond(A) * np.linalg.norm(x)
        gap = float(np.linalg.norm(x - xi))
        assert gap <= bound, (name, gap, bound)
        worst = max(worst, gap)
        room = min(room, bound / max(gap, 1e-300))
    return worst, room


def test_estimator_agrees_with_unquantised_least_squares():
    worst = max((_lstsq_gap(name) + (name,) for name in WELL_POSED), key=lambda v: v[0])
    print(f"worst |x - x'| = {worst[0]:.3e} ({worst[2]}), bound / gap >= {worst[1]:.1f}")


def _ulp(x):
    return math.ulp(x) if x else math.ulp(1.0) * 2.0 ** -52


ANGLES = [0.0, -0.0, 1e-300, 1e-9, -1e-9, 1e-3, 0.01, -0.02, 0.1, 0.5, -0.7] + \
    [s * (c + e) for c in (math.pi / 4, math.pi / 2, 3 * math.pi / 4, math.pi, 2 * math.pi)
     for e in (-1e-9, -2e-16, 0.0, 2e-16, 1e-9) for s in (1.0, -1.0)] + \
    [3.5, -4.0, 6.0, 10.0, -25.0, 50.0, 99.0, -100.0] + list(np.linspace(-100.0, 100.0, 4001))


def test_det_sincos_is_within_its_bound():
    """|x| <= 100.  The reduction y = (a - j PIO2_HI) - j PIO2_LO: the first difference is
    exact (j PIO2_HI is exact, and the operands are within a factor 2), the product j
    PIO2_LO and the second difference round by at most u |y| + u j 6.1e-11, and pi/2 -
    (PIO2_HI + PIO2_LO) is below 2^-86: y is off by less than 0.6 u.  The nested form
    evaluates s <- 1 - (x2 / c) s ten times with three roundings each; the last step's
    factor x2 / 2 <= 0.31 (sine: x2 / 6 <= 0.11) damps what the earlier ones left, so the
    polynomial is off by less than u (1 + 0.31 (3 + ...)) < 2.2 u, the sine's final product
    by another 0.71 u, and the Taylor remainder is below 1e-23.  With math.sin / math.cos
    themselves within u: 0.6 + 2.2 + 0.71 + 1 < 5 u absolute."""
    worst_abs = worst_ulp = 0.0
    for x in ANGLES:
        s, c = ref.det_sincos(float(x))
        for got, want in ((s, math.sin(x)), (c, math.cos(x))):
            worst_abs = max(worst_abs, abs(got - want))
            if abs(want) > 1e-3:
                worst_ulp = max(worst_ulp, abs(got - want) / math.ulp(want))
        assert abs(s - math.sin(x)) <= 5 * U and abs(c - math.cos(x)) <= 5 * U, x
        assert abs(s * s + c * c - 1.0) <= 8 * U
    print(f"worst |error| = {worst_abs:.3e} = {worst_abs / U:.2f} u; worst {worst_ulp:.2f} ulp of the value")
    assert ref.det_sincos(0.0) == (0.0, 1.0)
    assert all(math.isnan(v) for x in (math.inf, -math.inf, math.nan) for v in ref.det_sincos(x))
    for x in (1e6, -3e9, 1e300):       # defined for every finite argument, if not accurate
        s, c = ref.det_sincos(x)
        assert not math.isnan(s) and not math.isnan(c)


def test_det_sincos_large_arguments_follow_the_reduction():
    """|x| > pi: the quadrant logic against libm on arguments the reduction handles to
    a few u times the quarter turns taken off (j u pi/2 from a's own spacing)."""
    for x in (3.2, -3.2, 4.8, 7.9, -11.0, 1000.0, -12345.678):
        s, c = ref.det_sincos(x)
        tol = 5 * U + abs(x) * 2 * U
        assert abs(s - math.sin(x)) <= tol and abs(c - math.cos(x)) <= tol


def test_weights_closed_forms():
    w = lambda kn, k, r: float(ref.weight(kn, k, np.array([r]))[0])   # noqa: E731
    for r in (-3.0, 0.0, 0.25, 1e9):
        assert w("l2", 1.0, r) == 1.0
    assert w("huber", 0.5, 0.25) == 1.0 and w("huber", 0.5, -2.0) == 0.25
    assert w("huber", 0.5, 0.5) == 1.0                                   # a == k: the first branch
    assert w("huber", 0.5, np.nextafter(0.5, 1.0)) == 0.5 / np.nextafter(0.5, 1.0)   # continuous at k
    assert 1.0 - w("huber", 0.5, np.nextafter(0.5, 1.0)) <= 4 * U
    assert w("cauchy", 2.0, 0.0) == 1.0 and w("cauchy", 2.0, 2.0) == 0.5 and w("cauchy", 2.0, -6.0) == 0.1
    assert w("gm", 0.5, 0.0) == 2.0 and w("gm", 1.0, 1.0) == 0.25 and w("gm", 4.0, -2.0) == 0.0625
    assert w("tukey", 2.0, 0.0) == 1.0 and w("tukey", 2.0, 1.0) == 0.5625
    assert w("tukey", 2.0, 2.0) == 0.0                                   # (1 - 1)^2
    for r in (np.nextafter(2.0, 3.0), -2.5, 1e30, -math.inf):
        assert w("tukey", 2.0, r) == 0.0                                 # exactly 0 beyond k
    for kn, k in (("huber", 0.3), ("cauchy", 0.3), ("gm", 0.3), ("tukey", 0.3), ("l2", 1.0)):
        rs = np.linspace(0.0, 2.0, 2001)
        ws = ref.weight(kn, k, rs)
        assert (ws >= 0.0).all() and ws.max() <= ref.weight_sup(kn, k) * (1 + 4 * U)
        assert np.array_equal(ws, ref.weight(kn, k, -rs))                # even in r


def test_planar_target_gives_identity_and_the_loop_leaves():
    c = pc.case("planar")
    tr = []
    r = ref.icp_plane(c.src, c.tgt, c.nrm, c.d, kernel=c.kernel, k=c.k, trace=tr)
    P, cj, k = tr[0]
    A, g = ref.plane_sums(P, c.tgt.astype(np.float64), c.nrm.astype(np.float64), cj, c.kernel, c.k, k)
    M = np.zeros((6, 6))
    for q, (a, b) in enumerate(ref.PAIRS):
        M[a, b] = M[b, a] = A[q]
    assert np.linalg.matrix_rank(M) == 3
    assert ref.ldlt_solve(A, g) is None
    assert ref.plane_update(P, c.tgt.astype(np.float64), c.nrm.astype(np.float64), cj, c.kernel, c.k, k) \
        == ref.IDENTITY12
    assert r["iters"] == 1 and len(tr) == 1 and np.array_equal(r["T"], np.eye(4)) and r["n_corr"] == 65


@pytest.mark.parametrize("name", ["n1_m64", "n5_m64", "n5_m777"])
def test_fewer_than_six_correspondences_give_identity(name):
    c = pc.case(name)
    r = ref.icp_plane(c.src, c.tgt, c.nrm, c.d, kernel=c.kernel, k=c.k)
    assert 0 < r["n_corr"] < 6 and r["iters"] == 1 and np.array_equal(r["T"], np.eye(4))


def test_nan_normal_rows_are_skipped_but_counted():
    c = pc.case("nan_normal")
    tr = []
    r = ref.icp_plane(c.src, c.tgt, c.nrm, c.d, kernel=c.kernel, k=c.k, max_iteration=1, trace=tr)
    P, cj, k = tr[0]
    bad = ~np.isfinite(c.nrm).all(axis=1)
    assert bad.sum() == 2
    hit = cj >= 0
    skipped = int(bad[cj[hit]].sum())
    terms = ref.plane_terms(P, c.tgt.astype(np.float64), c.nrm.astype(np.float64), cj, c.kernel, c.k)[0]
    assert skipped >= 1 and len(terms) == hit.sum() - skipped and np.isfinite(terms).all()
    assert r["n_corr"] == 65 and r["fitness"] == 1.0 and np.isfinite(r["T"]).all()
    assert not np.array_equal(r["T"], np.eye(4))


def _known_answer():
    rng = np.random.default_rng(11)
    tgt, nrm = pc.ellipsoid(rng, 3000)
    src, _ = pc.ellipsoid(rng, 800)
    T = rc._rigid(0.03, -0.02, 0.025, [0.015, -0.02, 0.01])
    src = (src - T[:3, 3]) @ T[:3, :3]            # T takes it back onto the ellipsoid
    return rc._f32(src), rc._f32(tgt), rc._f32(nrm), T


# (RRE in degrees, RTE) of the reference's result, measured from the reference on the CPU
# (3 iterations each; before: 2.5 degrees, 0.027)
KNOWN = {"l2": (0.0181, 4.21e-5), "tukey": (0.0181, 4.19e-5)}


@pytest.mark.parametrize("kernel,k", [("l2", 1.0), ("tukey", 0.05)])
def test_known_motion_is_recovered(kernel, k):
    """Both clouds sampled separately on an ellipsoid with analytic normals, the source
    offset by a rigid motion (|t| = 0.027, 2.5 degrees) well inside d = 0.1."""
    src, tgt, nrm, T = _known_answer()
    r = ref.icp_plane(src, tgt, nrm, 0.1, kernel=kernel, k=k)
    rre, rte = synth.rre_rte(r["T"][:3, :3], r["T"][:3, 3], T[:3, :3], T[:3, 3])
    print(f"{kernel}: iters {r['iters']} fitness {r['fitness']:.3f} RRE {float(rre):.4f} deg RTE {float(rte):.2e}")
    want_rre, want_rte = KNOWN[kernel]
    # margin: a factor 2 over the measured error, which is set by the targets' spacing
    # (the nearest target is off the source's foot point), not by the arithmetic
    assert float(rre) <= 2 * want_rre and float(rte) <= 2 * want_rte
    assert r["fitness"] == 1.0


