"""CPU: pcr_icp_plane_batch's C ABI -- the ctypes mirror of pcr_icp_plane_params has gcc's
layout, the entry is declared, bound and exported, bad arguments are refused before any
device work -- and the façade's checks that raise before the GPU is touched."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from pointcloudregistration_amd import _lib
from pointcloudregistration_amd import registration as reg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -1


def test_plane_params_mirror_matches_c_layout(tmp_path):
    py = _lib.IcpPlaneParams
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "pcr_api.h"', "int main(void) {",
             'printf("sizeof %zu\\n", sizeof(pcr_icp_plane_params));']
    lines += [f'printf("{f[0]} %zu\\n", offsetof(pcr_icp_plane_params, {f[0]}));' for f in py._fields_]
    lines += ['printf("ids %d %d %d %d %d\\n", PCR_KERNEL_L2, PCR_KERNEL_HUBER, PCR_KERNEL_CAUCHY, '
              'PCR_KERNEL_GM, PCR_KERNEL_TUKEY);', "return 0; }"]
    src, exe = tmp_path / "abi.c", tmp_path / "abi"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True,
                   capture_output=True)
    out = dict(ln.split(None, 1) for ln in subprocess.run([str(exe)], check=True, capture_output=True,
                                                          text=True).stdout.splitlines())
    assert int(out["sizeof"]) == ctypes.sizeof(py) == 16
    for f in py._fields_:
        assert int(out[f[0]]) == getattr(py, f[0]).offset, f[0]
    ids = [int(v) for v in out["ids"].split()]
    assert ids == [c.kernel_id for c in (reg.L2Loss, reg.HuberLoss, reg.CauchyLoss, reg.GMLoss, reg.TukeyLoss)]


def test_entry_is_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "pcr_api.h")).read()
    lib = _lib.load()
    assert "pcr_icp_plane_batch(" in hdr and hasattr(lib, "pcr_icp_plane_batch")
    assert len(_lib.SIGNATURES["pcr_icp_plane_batch"]) == 16


def _call(lib, P=1, N=4, M=4, kernel=0, k=1.0, null=None, params=True, plane=True):
    one = ctypes.c_void_p(256)   # never dereferenced: every check below precedes device work
    ptr = {n: one for n in ("src", "tgt", "nrm", "init", "T", "fr", "st")}
    if null:
        ptr[null] = None
    ip = _lib.IcpParams(0.1, 1e-6, 1e-6, 30, 0)
    pp = _lib.IcpPlaneParams(kernel, 0, k)
    return lib.pcr_icp_plane_batch(ptr["src"], ptr["tgt"], ptr["nrm"], P, N, M, None, None, ptr["init"],
                                   ctypes.byref(ip) if params else None, ctypes.byref(pp) if plane else None,
                                   ptr["T"], ptr["fr"], ptr["st"], None, None)


def test_bad_arguments_are_refused_before_device_work():
    lib = _lib.load()
    assert _call(lib, P=0) == 0                      # nothing to do, even with ...
    assert _call(lib, P=0, null="src", params=False, plane=False) == 0   # ... nothing to read
    for null in ("src", "tgt", "nrm", "init", "T", "fr", "st"):
        assert _call(lib, null=null) == ERR_ARG, null
        assert b"icp_plane: null pointer" in lib.pcr_last_error()
    assert _call(lib, params=False) == ERR_ARG and b"null pointer" in lib.pcr_last_error()
    assert _call(lib, plane=False) == ERR_ARG and b"null pointer" in lib.pcr_last_error()
    for kw in (dict(P=-1), dict(N=-1), dict(M=-1)):
        assert _call(lib, **kw) == ERR_ARG, kw
        assert b"negative size" in lib.pcr_last_error()
    for kernel in (-1, 5, 99):
        assert _call(lib, kernel=kernel) == ERR_ARG
        assert b"unknown kernel" in lib.pcr_last_error()
    for kernel in (1, 2, 3, 4):
        for k in (0.0, -1.0, float("nan")):
            assert _call(lib, kernel=kernel, k=k) == ERR_ARG, (kernel, k)
            assert b"k must be > 0" in lib.pcr_last_error()


class _Cloud:
    def __init__(self, points, normals=None):
        self.points, self.normals = points, normals


def test_facade_refuses_before_the_gpu(monkeypatch):
    """Each check raises before a tensor is made: the device lookup is made to fail
    loudly, so reaching it would show as another error."""
    def no_device():
        raise AssertionError("the GPU was touched")
    monkeypatch.setattr(reg, "_device", no_device)
    pts = np.zeros((8, 3))
    nrm = np.tile([0.0, 0.0, 1.0], (8, 1))
    P2P = reg.TransformationEstimationPointToPlane
    with pytest.raises(NotImplementedError, match="L1Loss"):
        reg.registration_icp(_Cloud(pts), _Cloud(pts, nrm), 0.1, np.eye(4), P2P(reg.L1Loss()))
    with pytest.raises(ValueError, match="normals"):
        reg.registration_icp(_Cloud(pts), _Cloud(pts), 0.1, np.eye(4), P2P())
    with pytest.raises(ValueError, match="normals"):
        reg.registration_icp(_Cloud(pts), reg.PointCloud(pts), 0.1, np.eye(4), P2P(reg.TukeyLoss(0.1)))
    for loss in (reg.HuberLoss, reg.CauchyLoss, reg.GMLoss, reg.TukeyLoss):
        for k in (0.0, -2.0, float("nan")):
            with pytest.raises(ValueError, match="k must be > 0"):
                reg.registration_icp(_Cloud(pts), _Cloud(pts, nrm), 0.1, np.eye(4), P2P(loss(k)))
            with pytest.raises(ValueError, match="k must be > 0"):
                reg.icp_batch(pts, pts, np.eye(4), reg.IcpParams(0.1), estimation=P2P(loss(k)), tgt_normals=nrm)
    with pytest.raises(NotImplementedError, match="L1Loss"):
        reg.icp_batch(pts, pts, np.eye(4), reg.IcpParams(0.1), estimation=P2P(reg.L1Loss()), tgt_normals=nrm)
    with pytest.raises(ValueError, match="tgt_normals"):
        reg.icp_batch(pts, pts, np.eye(4), reg.IcpParams(0.1), estimation=P2P())
    with pytest.raises(NotImplementedError, match="with_scaling"):
        reg.TransformationEstimationPointToPoint(with_scaling=True)
    assert isinstance(P2P().kernel, reg.L2Loss)
