"""CPU: the f64 restatement of the CPD contract (tests/cpd_ref.py) is sound --
its dense and matrix-free E-steps agree, it recovers known rigid and affine maps,
its stop rule and its den == 0 rule behave as written -- and the entries are
declared, bound and exported and refuse bad arguments before any device work.
That is what lets tests/test_cpd_gpu.py stand on the restatement."""
import ctypes
import os

import numpy as np
import pytest

import cpd_ref as cr
from pointcloudregistration_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("pcr_cpd_scratch_bytes", "pcr_cpd_estep", "pcr_cpd_register")
EULER = cr.rot_z(0.4) @ np.array([[1, 0, 0], [0, np.cos(.3), -np.sin(.3)], [0, np.sin(.3), np.cos(.3)]])
SHIFT = np.array([0.1, -0.2, 0.05])


@pytest.mark.parametrize("M,N", [(1, 1), (1, 9), (9, 1), (33, 47)])
@pytest.mark.parametrize("sigma2", [1e-1, 1e-3])
@pytest.mark.parametrize("w", [0.0, 0.1])
def test_dense_and_matrix_free_agree(M, N, sigma2, w):
    rng = np.random.default_rng(M * 100 + N)
    ys, X = rng.random((M, 3), dtype=np.float32), rng.random((N, 3), dtype=np.float32)
    X[-1] += 9.0 if N > 1 else 0.0     # a column every term of which is flushed
    a, b = cr.estep(ys, X, sigma2, w), cr.estep_matrix_free(ys, X, sigma2, w)
    for u, v in zip(a, b):
        assert cr.rel_err(v, u) < 1e-12


def test_den_zero_rule():
    """A target no source reaches: den is FLT_EPSILON there, so Pt1 is 1 with
    w = 0 and eps / (eps + c) otherwise, and the column adds nothing to P1, PX."""
    rng = np.random.default_rng(1)
    ys, X = rng.random((20, 3), dtype=np.float32), rng.random((30, 3), dtype=np.float32)
    X[7] += 5.0
    s2 = 1e-2
    assert cr.column_max_args(ys, X, s2)[7] < -120
    keep = np.arange(30) != 7
    for w in (0.0, 0.1):
        pt1, p1, px, n_p = cr.estep(ys, X, s2, w)
        c = cr.const_c(s2, w, 20, 30)
        assert pt1[7] == cr.FLT_EPSILON / (cr.FLT_EPSILON + c)
        assert w > 0 or pt1[7] == 1.0
        # the other columns are those of the 29-target problem with the same c
        k = np.exp(-cr.sqdist_f32(ys, X[keep]).astype(np.float64) / (2 * s2))
        r = k.sum(0) + c
        assert np.allclose(p1, (k / r).sum(1), rtol=1e-13, atol=0)
        assert np.allclose(pt1[keep], k.sum(0) / r, rtol=1e-13, atol=0)
        assert n_p == pytest.approx(p1.sum(), rel=1e-15)


def test_f32_program_is_close_to_f64():
    """probreg's dense f32 formulation, the GPU tests' yardstick for tolerances,
    is itself within 1e-5 of the f64 contract and farther from it at small sigma2."""
    rng = np.random.default_rng(2)
    ys = rng.random((257, 3), dtype=np.float32)
    X = (ys[rng.integers(0, 257, 200)] + rng.normal(0, 0.01, (200, 3))).astype(np.float32)
    errs = []
    for s2 in (1e-1, 1e-3):
        a, b = cr.estep(ys, X, s2, 0.1), cr.estep_f32(ys, X, s2, 0.1)
        errs.append(max(cr.rel_err(v, u) for u, v in zip(a[:3], b[:3])))
    assert errs[0] < errs[1] < 1e-5


def subset_pair(seed=0):
    """X (130 points) and a 65-point subset of it: the targets of a noiseless pair."""
    rng = np.random.default_rng(seed)
    X = rng.random((130, 3))
    return X, X[rng.permutation(130)[:65]]


@pytest.mark.parametrize("kind,s", [(cr.RIGID, 1.0), (cr.RIGID_SCALE, 1.2)])
def test_recovers_rotation_scale_translation(kind, s):
    """x = s R y + t on a noiseless pair whose targets are a subset of the moved
    sources (every target has its source, so sigma2 falls to its floor)."""
    X, Xs = subset_pair()
    Y = ((X - SHIFT) @ EULER) / s
    r = cr.register(Y, Xs, kind, w=0.0, maxiter=50, tol=0)
    assert r["status"] == 0 and r["iters"] == 50
    # Y is rounded to f32 by the contract: 2^-24 relative on coordinates of size 1
    assert np.abs(r["T"][:3, :3] - s * EULER).max() < 1e-6
    assert np.abs(r["T"][:3, 3] - SHIFT).max() < 1e-6
    assert abs(r["scale"] - s) < 1e-6
    assert r["sigma2"] == cr.FLT_EPSILON
    assert np.array_equal(r["T"][3], [0, 0, 0, 1])


def test_recovers_affine_map():
    X, Xs = subset_pair(1)
    B = EULER @ np.diag([1.1, 0.9, 1.05]) + 0.05 * np.random.default_rng(5).normal(size=(3, 3))
    Y = (X - SHIFT) @ np.linalg.inv(B).T
    r = cr.register(Y, Xs, cr.AFFINE, w=0.0, maxiter=50, tol=0)
    assert np.abs(r["T"][:3, :3] - B).max() < 1e-6
    assert np.abs(r["T"][:3, 3] - SHIFT).max() < 1e-6
    assert r["scale"] == 1.0


def test_rotation_is_proper_under_reflection():
    A = np.diag([3.0, 2.0, -1.0])
    R = cr.rotation_of(A)
    assert np.linalg.det(R) == pytest.approx(1.0) and np.allclose(R, np.eye(3))


def test_stop_rule():
    y, x = cr.stop_rule_pair()
    full = cr.register(y, x, cr.RIGID, w=0.1, maxiter=40, tol=0)
    assert full["iters"] == 40 and len(full["qs"]) == 40       # tol <= 0 never stops
    dq = np.abs(np.diff(full["qs"]))
    for tol in (0.1, 1.0):
        r = cr.register(y, x, cr.RIGID, w=0.1, maxiter=40, tol=tol)
        first = int(np.argmax(dq < tol)) + 1                    # 0-based iteration i >= 1
        assert (dq < tol).any() and r["iters"] == first + 1
        assert r["qs"] == full["qs"][:first + 1]
    # iteration 0 never stops, whatever tol
    assert cr.register(y, x, cr.RIGID, w=0.1, maxiter=40, tol=1e30)["iters"] == 2
    assert cr.register(y, x, cr.RIGID, maxiter=0)["iters"] == 0
    assert cr.register(y[:0], x, cr.RIGID)["status"] == 1


def test_stop_rule_pair_is_unambiguous():
    """On the stop-rule pair the f64 and the f32 program stop at the same
    iteration in all four combinations, with every |dq| well away from tol."""
    y, x = cr.stop_rule_pair()
    for w in (0.0, 0.1):
        for kind in (cr.RIGID, cr.RIGID_SCALE):
            a = cr.register(y, x, kind, w=w, maxiter=60, tol=0.1)
            b = cr.register(y, x, kind, w=w, maxiter=60, tol=0.1, estep_fn=cr.estep_f32)
            assert a["iters"] == b["iters"] < 60
            qd = np.abs(np.array(a["qs"]) - np.array(b["qs"])).max()
            margin = np.abs(np.abs(np.diff(a["qs"])) - 0.1).min()
            assert margin >= 8 * qd
            assert min(a["min_colmax"]) > -80


def test_nonrigid_restatement_reduces_the_residual():
    rng = np.random.default_rng(4)
    Y = rng.random((40, 3))
    X = Y + 0.05 * np.sin(3.0 * Y[:, [1, 2, 0]])
    r = cr.nonrigid(Y, X, maxiter=10, tol=0)
    moved = Y.astype(np.float32).astype(np.float64) + r["g"] @ r["w"]
    assert r["iters"] == 10
    assert np.abs(moved - X).max() < 0.3 * np.abs(Y - X).max()


def test_entries_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "pcr_api.h")).read()
    lib = _lib.load()
    for s in ENTRIES:
        assert s + "(" in hdr and s in _lib.exported_symbols() and hasattr(lib, s)
    assert len(_lib.SIGNATURES["pcr_cpd_estep"]) == 16
    assert len(_lib.SIGNATURES["pcr_cpd_register"]) == 20
    assert "not pinned against probreg" in hdr.lower()


def test_scratch_sizes():
    lib = _lib.load()
    f = lib.pcr_cpd_scratch_bytes
    assert f(-1, 4, 4) == -1 and b"out of range" in lib.pcr_last_error()
    assert f(0, 0, 0) >= 0
    # a batch that fills the chip unsplit: state, inv, Pt1, P1, PX, the five f64 row
    # moments and one f64 a target only -- 256 + 56 M + 16 N bytes a pair plus rounding,
    # nothing that grows with M N
    P, M, N = 256, 1024, 1024
    assert f(P, M, N) <= P * (256 + 56 * M + 16 * N) + 10 * 256
    assert f(512, 100000, 100000) <= 512 * (256 + 72 * 100000) + 10 * 256
    # a split sweep (P ceil(lanes / 256) < 512) keeps one f64 partial per lane and
    # 512-point chunk of the staged axis, 1 a target and 5 a source: a product of both
    # sizes over 512, as the header says -- 6 MiB here, about 0.9 GB at P = 1, 100000^2
    chunks = 8192 // 512
    assert f(1, 8192, 8192) <= 8 * chunks * 6 * 8192 + (256 + 72 * 8192) + 10 * 256
    assert f(1, 8192, 8192) >= 8 * chunks * 6 * 8192
    assert 0.9e9 < f(1, 100000, 100000) < 1.0e9


def test_bad_arguments_are_refused_before_device_work():
    lib = _lib.load()
    one = ctypes.c_void_p(256)
    assert lib.pcr_cpd_register(one, one, 1, 4, 4, None, None, 3, 0.0, 5, 0.0, None, one, one, one, one, one, one,
                                one, None) != 0
    assert b"kind=3" in lib.pcr_last_error()
    assert lib.pcr_cpd_register(one, one, 1, 4, 4, None, None, 0, 1.0, 5, 0.0, None, one, one, one, one, one, one,
                                one, None) != 0
    assert b"w=1" in lib.pcr_last_error()
    assert lib.pcr_cpd_estep(one, one, 1, 4, 4, None, None, None, one, 0.0, one, one, one, one, None, None) != 0
    assert b"null pointer" in lib.pcr_last_error()
    assert lib.pcr_cpd_estep(one, one, 1, 4, 4, None, None, None, one, 0.0, one, one, one, one,
                             ctypes.c_void_p(8), None) != 0
    assert b"aligned" in lib.pcr_last_error()


def test_python_names_and_cpu_tensors_raise():
    import torch
    from pointcloudregistration_amd import cpd
    for name in ("RigidCPD", "AffineCPD", "NonRigidCPD", "expectation_step", "register_batch", "CpdBatchResult"):
        assert hasattr(cpd, name) and name in cpd.__all__
    import pointcloudregistration_amd as pcr
    assert pcr.cpd is cpd and "cpd" in pcr.__all__
    cpu = torch.zeros(4, 3)
    with pytest.raises(ValueError, match="no CPU path"):
        cpd.RigidCPD(cpu)
    with pytest.raises(ValueError, match="no CPU path"):
        cpd.expectation_step(cpu, cpu, 0.1)
    with pytest.raises(ValueError, match="no CPU path"):
        cpd.register_batch(cpu[None], cpu[None])
    with pytest.raises(ValueError, match="no CPU path"):
        cpd.RigidCPD(np.zeros((4, 3), np.float32), use_cuda=False)
