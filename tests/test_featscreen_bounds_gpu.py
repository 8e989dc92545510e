"""GPU: the feature screen's certificates against exact distances.

row_tail (csrc/featnn_row.hip) stores for every pass-1 row its screened value and an
error bound, v12 / e12, and for every pass-2 column wq = (w1 + bias, w2 + bias,
e2, bias); featmut_resolve decides mutuality from these numbers alone.  Here
they are read back (featscreen_cases.mut_scratch: feature_corres_v5's scratch
through pcr_featmut_debug_copy) and each CLAIM is checked: |value - s^2 D_exact| <= its bound, with
D_exact in f64 from the f32 inputs and s the pair's power-of-two scale (x s is
exact), recovered from the values themselves.  The only slack is the f64
rounding of the reference, 1e-12 s^2 (|x|^2 + |y|^2) (D 2^-52 relative with a
wide margin): it is no tolerance for the kernel.  A bound that is not finite
claims nothing (the resolve rescans) and is skipped; rows / columns with a
non-finite element have no exact distance and are skipped.

`subnormal` (test_featcorres_gpu.CASES) is left out here only: its scale
saturates at 2^127 and the descriptors stay subnormal after scaling, so the
recovery of s^2 from value / distance is ill-posed."""
import numpy as np
import pytest

import featscreen_cases as fc
from pointcloudregistration_amd import registration as reg
from test_featcorres_gpu import CASES, USED_RESCAN, USED_SCREENED

pytestmark = pytest.mark.gpu

PATHS = {"row9": {}, "row8": {"PCR_FEAT_ROW9": "0"}}
_DIST = {}


def _np(t):
    return t.detach().cpu().numpy()


def _all_cases():
    c = {k: (CASES[k][0][None], CASES[k][1][None]) for k in
         ("synthetic_4096", "dynamic_range", "offset", "near_twins", "tail_above_sample", "tail_below_sample", "d1")}
    for k in fc.BIAS_CASES:
        c["bias_" + k] = (fc.BIAS_CASES[k]["F"][None], fc.BIAS_CASES[k]["G"][None])
    _, F, G = fc.bias_batch()
    c["bias_batch"] = (F, G)
    for k in fc.ONESIDED_CASES:
        c["onesided_" + k] = (fc.ONESIDED_CASES[k]["F"][None], fc.ONESIDED_CASES[k]["G"][None])
    return c


ALL = _all_cases()


def _exact(name, p):
    """the pair's exact distances and squared norms, computed once"""
    if (name, p) not in _DIST:
        F, G = ALL[name][0][p], ALL[name][1][p]
        _DIST[(name, p)] = (fc.exact_dist(F, G), (F.astype(np.float64) ** 2).sum(1),
                            (G.astype(np.float64) ** 2).sum(1))
    return _DIST[(name, p)]


def _scale2(v12, dsel):
    """s^2 = 2^(2 round(0.5 log2(v12 / D))) at the row with the largest exact
    distance; the same exponent must come out of at least 5 other rows."""
    with np.errstate(all="ignore"):
        ok = np.isfinite(dsel) & (dsel > 0) & np.isfinite(v12) & (v12 > 0)
        ex = np.round(0.5 * np.log2(v12 / dsel))
    assert ok.sum() >= 6, ok.sum()
    top = np.flatnonzero(ok)[np.argmax(dsel[ok])]
    same = int((ex[ok] == ex[top]).sum()) - 1
    assert same >= 5, (ex[top], same)
    return 2.0 ** (2.0 * ex[top])


def _holds(err, bound):
    """the claim |err| <= bound; a non-finite bound claims nothing"""
    with np.errstate(all="ignore"):
        return (err <= bound) | ~np.isfinite(bound)


def _check_pair(name, p, nn, v12, e12, wq, used):
    D, nx, ny = _exact(name, p)
    n, m = D.shape
    rows = np.arange(n)
    dsel = D[rows, nn]
    s2 = _scale2(v12, dsel)
    fin = np.isfinite(dsel)
    slack = 1e-12 * s2 * (nx + ny[nn])
    # pass 1: every row (rescanned ones carry e12 = 0: the slack alone)
    with np.errstate(all="ignore"):
        err = np.abs(v12 - s2 * dsel)
    ok = _holds(err, e12.astype(np.float64) + slack) | ~fin
    bad = np.flatnonzero(~ok)
    assert bad.size == 0, ("pass 1", p, bad[:6], v12[bad[:6]], s2 * dsel[bad[:6]], e12[bad[:6]])
    # pass 2: every screened column's top-2 values over the rows
    Dc = np.where(np.isnan(D), np.inf, D)
    o = np.argsort(Dc, axis=0, kind="stable")[:2]
    scr = np.flatnonzero((used == USED_SCREENED) | (used == USED_RESCAN))
    scr = scr[np.isfinite(ny[scr])]
    w = wq[scr].astype(np.float64)
    bias, e2 = w[:, 3], w[:, 2]
    for k in range(min(2, n)):
        i = o[k, scr]
        ex = s2 * Dc[i, scr]
        with np.errstate(all="ignore"):
            err = np.abs((w[:, k] - bias) - ex)
        ok = _holds(err, e2 + 1e-12 * s2 * (nx[i] + ny[scr])) | ~np.isfinite(ex)
        bad = np.flatnonzero(~ok)
        assert bad.size == 0, ("pass 2 w%d" % (k + 1), p, scr[bad[:6]], (w[:, k] - bias)[bad[:6]], ex[bad[:6]],
                               e2[bad[:6]])
    return s2, D


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("name", list(ALL))
def test_certificates_hold(monkeypatch, name, path):
    """Every stored (value, bound) of both passes covers the exact distance, on
    the shipped featnn_row9 path and on the featnn_row8 1-term passes (the same
    row_tail with the fixed bias and bound1)."""
    for k, v in PATHS[path].items():
        monkeypatch.setenv(k, v)
    F, G = ALL[name]
    P, N, M = F.shape[0], F.shape[1], G.shape[1]
    co, nc, nn12 = reg.feature_correspondences(F, G)
    sc = fc.mut_scratch(P, N, M)
    v12, e12, wq, used = sc["v12"], sc["e12"], sc["wq"], sc["used"][:, :M]
    nn12 = _np(nn12)
    for p in range(P):
        s2, D = _check_pair(name, p, nn12[p], v12[p], e12[p], wq[p], used[p])
        if name == "synthetic_4096":
            # not vacuous: on ordinary data (test_featscreen_model_cpu.py shows the
            # input allows it) the bound is below half the exact top-2 gap for more
            # than half of the rows, so the certificate can decide them
            d = np.partition(D, 1, axis=1)[:, :2]
            assert (e12[p] < 0.5 * (d[:, 1] - d[:, 0]) * s2).mean() > 0.5
