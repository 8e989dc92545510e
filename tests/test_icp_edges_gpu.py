"""ICP (csrc/icp.hip) against the oracle's icp_core, bit for bit, where there is little
or nothing to estimate from (tests/registration_cases.py): no correspondence at the
start (iters 0, T == init, with the exact identity and with another init), one or two
correspondences (rank-deficient Horn input), n = 1, m = 1, max_iteration 0 and 1, a
point exactly at distance d, a radius whose float square differs from its f64 square,
duplicate targets, collinear clouds and all points identical -- as two pairs on 2 and
on 8 cooperating workgroups each (most lanes own no point), as 300 copies with jittered
inits (one workgroup per pair, then the tail launch), and in one ragged batch that also
holds pairs without sources and without targets.

Compared: T as raw f64 bits, fitness, rmse, (iters, n_corr), the number of corr_tgt
entries set and the padding of corr_tgt."""
import os

import numpy as np
import pytest

import registration_cases as rc
from pointcloudregistration_amd import registration as reg

pytestmark = pytest.mark.gpu

KEYS = ("PCR_COOP_G", "PCR_ICP_TAIL")


@pytest.fixture()
def icp_env():
    old = {k: os.environ.get(k) for k in KEYS}

    def set_env(g=None):
        os.environ.pop("PCR_ICP_TAIL", None)
        if g is None:
            os.environ.pop("PCR_COOP_G", None)
        else:
            os.environ["PCR_COOP_G"] = str(g)
    yield set_env
    for k, v in old.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v


def _np(t):
    return t.detach().cpu().numpy()


def _mismatch(res, p, o, init, n):
    """Names of the fields of pair p that differ from the oracle result o."""
    T, ct = _np(res.transformation)[p], _np(res.corr_tgt)[p]
    bad = []
    if T.tobytes() != np.ascontiguousarray(o["T"]).tobytes():
        bad.append("T")
    if _np(res.fitness)[p].tobytes() != np.float64(o["fitness"]).tobytes():
        bad.append("fitness")
    if _np(res.inlier_rmse)[p].tobytes() != np.float64(o["inlier_rmse"]).tobytes():
        bad.append("rmse")
    st = tuple(int(v) for v in _np(res.stats)[p])
    if st != (o["iters"], o["n_corr"]):
        bad.append(f"stats {st} != {(o['iters'], o['n_corr'])}")
    if int((ct[:n] >= 0).sum()) != o["n_corr"] or not (ct[n:] == -1).all():
        bad.append("corr_tgt")
    if o["n_corr"] == 0 and o["iters"] == 0:   # nothing to estimate from: T is init, untouched
        if T.tobytes() != np.ascontiguousarray(init, np.float64).tobytes() or not (ct == -1).all():
            bad.append("T != init")
    return bad


def _copies(name, ks):
    c = rc.icase(name)
    P = len(ks)
    src = np.broadcast_to(c.src, (P,) + c.src.shape).copy()
    tgt = np.broadcast_to(c.tgt, (P,) + c.tgt.shape).copy()
    init = np.stack([rc.jitter_init(c.init, k) for k in ks])
    return c, src, tgt, init


@pytest.mark.parametrize("G", [2, 8])
@pytest.mark.parametrize("name", rc.ICP_CASES)
def test_icp_case_cooperative_bitexact_vs_oracle(oracle, icp_env, name, G):
    """The case and a copy with a jittered init as P = 2 on G workgroups per pair: the
    count == 0 exit and the stop rule are taken from the pair-wide totals, so all G
    leave the loop together."""
    c, src, tgt, init = _copies(name, (0, 1))
    icp_env(G)
    bad = {}
    for it in rc.ICP_ITERS:
        res = reg.icp_batch(src, tgt, init, reg.IcpParams(c.d, max_iteration=it))
        for p in range(2):
            m = _mismatch(res, p, rc.oracle_icp(oracle, name, it, p), init[p], len(c.src))
            if m:
                bad[(it, p)] = m
    assert bad == {}


@pytest.mark.parametrize("name", rc.ICP_CASES)
def test_icp_case_300_copies_bitexact_vs_oracle(oracle, icp_env, name):
    """300 copies with per-pair init jitter: one workgroup per pair, the last pairs
    still iterating handed to the cooperative tail launch."""
    P = 300
    c, src, tgt, init = _copies(name, range(P))
    icp_env(None)
    bad = {}
    for it in rc.ICP_ITERS:
        res = reg.icp_batch(src, tgt, init, reg.IcpParams(c.d, max_iteration=it))
        for p in range(P):
            m = _mismatch(res, p, rc.oracle_icp(oracle, name, it, p), init[p], len(c.src))
            if m:
                bad[(it, p)] = m
    assert bad == {}


@pytest.mark.parametrize("G", [None, 1, 8])
def test_icp_ragged_batch_bitexact_vs_oracle(oracle, icp_env, G):
    """Every case of radius ICP_D and its jittered copy in one padded batch with a pair
    without sources and one without targets (both: T = init, iters 0, no barrier met).
    Padding holds points that would change the result if the kernel looked at them:
    targets on a source point, sources far away."""
    names = [n for n in rc.ICP_CASES if rc.icase(n).d == rc.ICP_D]
    rows = [(n, k) for n in names for k in (0, 1)] + [("ordinary", "n0"), ("ordinary", "m0")]
    N = max(len(rc.icase(n).src) for n, _ in rows)
    M = max(len(rc.icase(n).tgt) for n, _ in rows)
    P = len(rows)
    src = np.full((P, N, 3), 50.0, np.float32)
    tgt = np.zeros((P, M, 3), np.float32)
    init = np.zeros((P, 4, 4))
    ns, nt = np.zeros(P, np.int32), np.zeros(P, np.int32)
    for p, (n, k) in enumerate(rows):
        c = rc.icase(n)
        tgt[p] = c.src[0]
        if k != "n0":
            src[p, :len(c.src)] = c.src
            ns[p] = len(c.src)
        if k != "m0":
            tgt[p, :len(c.tgt)] = c.tgt
            nt[p] = len(c.tgt)
        init[p] = rc.NON_IDENTITY if isinstance(k, str) else rc.jitter_init(c.init, k)
    icp_env(G)
    bad = {}
    for it in rc.ICP_ITERS:
        res = reg.icp_batch(src, tgt, init, reg.IcpParams(rc.ICP_D, max_iteration=it), n_src=ns, n_tgt=nt)
        for p, (n, k) in enumerate(rows):
            if isinstance(k, str):
                o = dict(T=init[p], fitness=0.0, inlier_rmse=0.0, iters=0, n_corr=0)
            else:
                o = rc.oracle_icp(oracle, n, it, k)
            m = _mismatch(res, p, o, init[p], int(ns[p]))
            if m:
                bad[(it, n, k)] = m
    assert bad == {}
