"""Coherent Point Drift on the GPU: rigid, rigid + scale, affine and non-rigid
(Myronenko & Song 2010), the second alignment method of the reference
(``DataPreparation/CPD.py:26-73`` runs ``probreg.cpd`` on cupy in f32).

probreg's E-step forms the dense ``(M, N)`` posterior three times per iteration;
only ``Pt1 (N)``, ``P1 (M)`` and ``PX (M, 3)`` are used.  Here two sweeps of
libpcr.so (``pcr_cpd_estep``; contract in ``include/pcr_api.h``) give those
vectors with no ``(M, N)`` array, and ``pcr_cpd_register`` runs the whole rigid
or affine loop on torch's current stream from a per-pair state record in device
memory: no result goes through the host, every pair of a batch stops on its
own, and the sequence can be captured in a ``torch.cuda.graph``.  The one host
read is the count of stopped pairs, after every eighth iteration when
``tol > 0`` and the stream is not capturing (it synchronises the stream, so
work queued on other streams behind it waits; ``tol <= 0`` or a capture has
none).  Non-rigid CPD uses
the same E-step; its Gram matrix, the ``(M, M)`` solve (``torch.linalg.solve``,
f64, on the device) and the stop test are torch plumbing here, with one host
read per iteration.

The call shape is probreg's, so ``CPD.py`` swaps one import::

    from pointcloudregistration_amd import cpd
    tf_param, sigma2, q = cpd.RigidCPD(source).registration(target)
    moved = tf_param.transform(source)

NOT pinned against probreg: probreg and cupy are not available to this project,
so the contract is CPD as published with probreg's conventions as far as they
are known (``tests/cpd_ref.py`` restates it in f64).

numpy inputs give numpy outputs, device tensors stay device tensors, CPU torch
tensors raise: like ``nndistance``, the module has no CPU path.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from . import _lib

__all__ = ["RigidCPD", "AffineCPD", "NonRigidCPD", "RigidTransformation", "AffineTransformation",
           "NonRigidTransformation", "CpdBatchResult", "expectation_step", "register_batch"]

KINDS = {"rigid": 0, "rigid_scale": 1, "affine": 2}


def _device():
    if not torch.cuda.is_available():
        raise _lib.PcrError("cpd needs a ROCm/HIP device: libpcr is a GPU (gfx950) library with no CPU path")
    return torch.device("cuda", torch.cuda.current_device())


def _cloud(name, a, dims):
    """f32 contiguous device tensor and whether the caller passed numpy."""
    if isinstance(a, np.ndarray):
        t, was_np = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(_device()), True
    elif isinstance(a, torch.Tensor):
        if not a.is_cuda:
            raise ValueError(f"{name} must be a numpy array or a CUDA (ROCm/HIP) tensor: this module has no "
                             "CPU path")
        t, was_np = a.detach().to(torch.float32).contiguous(), False
    else:
        raise TypeError(f"{name} must be a numpy array or a torch.Tensor, got {type(a).__name__}")
    if t.dim() not in dims or t.shape[-1] != 3:
        raise ValueError(f"{name} must be ({'P, ' if 3 in dims else ''}n, 3), got {tuple(t.shape)}")
    return t, was_np


def _counts(name, n, P, device):
    """Valid counts as an int32 device tensor; the kernels clamp them into [0, nmax]."""
    if n is None:
        return None
    t = torch.as_tensor(n, device=device).to(torch.int32).contiguous()
    if tuple(t.shape) != (P,):
        raise ValueError(f"{name} must have shape ({P},), got {tuple(t.shape)}")
    return t


def _scratch(P, M, N, device):
    n = _lib.load().pcr_cpd_scratch_bytes(P, M, N)
    if n < 0:
        raise _lib.PcrError("pcr_cpd_scratch_bytes: " + _lib.load().pcr_last_error().decode())
    return torch.empty(max(int(n), 1), dtype=torch.uint8, device=device)


def _f64_per_pair(name, v, P, device, shape=()):
    t = torch.as_tensor(v, dtype=torch.float64, device=device)
    if t.dim() == len(shape):
        t = t.expand((P,) + tuple(shape))
    if tuple(t.shape) != (P,) + tuple(shape):
        raise ValueError(f"{name} must be {tuple(shape)} or {(P,) + tuple(shape)}, got {tuple(t.shape)}")
    return t.contiguous()


def _estep(src, tgt, n_src, n_tgt, T, sigma2, w):
    """Batched E-step on device tensors: pt1 (P,N), p1 (P,M), px (P,M,3) f32, n_p (P) f64."""
    P, M, N = src.shape[0], src.shape[1], tgt.shape[1]
    dev = src.device
    pt1 = torch.zeros(P, N, dtype=torch.float32, device=dev)
    p1 = torch.zeros(P, M, dtype=torch.float32, device=dev)
    px = torch.zeros(P, M, 3, dtype=torch.float32, device=dev)
    n_p = torch.zeros(P, dtype=torch.float64, device=dev)
    scratch = _scratch(P, M, N, dev)
    with torch.cuda.device(dev):
        _lib.call("pcr_cpd_estep", _lib.ptr(src), _lib.ptr(tgt), P, M, N, _lib.ptr(n_src), _lib.ptr(n_tgt),
                  _lib.ptr(T), _lib.ptr(sigma2), float(w), _lib.ptr(pt1), _lib.ptr(p1), _lib.ptr(px),
                  _lib.ptr(n_p), _lib.ptr(scratch), _lib.stream_handle(dev))
    return pt1, p1, px, n_p


def expectation_step(t_source, target, sigma2, w=0.0, transform=None, n_src=None, n_tgt=None):
    """One CPD E-step without the ``(M, N)`` posterior.

    ``t_source (M, 3)`` (already transformed, or with ``transform`` a 4x4 f64
    applied in f64 inside the sweep) and ``target (N, 3)``, or batches
    ``(P, M, 3)`` / ``(P, N, 3)`` with optional valid counts ``n_src`` /
    ``n_tgt (P)``; ``sigma2`` a number or ``(P,)``.  Returns ``(pt1, p1, px,
    n_p)``: f32 ``(N,)``, ``(M,)``, ``(M, 3)`` and ``n_p`` f64 (a 0-d value, or
    with the leading ``P``).  Rows past a pair's counts are returned as 0."""
    src, np_in = _cloud("t_source", t_source, (2, 3))
    tgt, np_tgt = _cloud("target", target, (2, 3))
    if np_in != np_tgt or src.dim() != tgt.dim() or src.device != tgt.device:
        raise ValueError("t_source and target must be of one kind (numpy or device tensors), rank and device")
    single = src.dim() == 2
    if single:
        src, tgt = src[None], tgt[None]
    if src.shape[0] != tgt.shape[0]:
        raise ValueError(f"t_source {tuple(src.shape)} and target {tuple(tgt.shape)} must share the batch size")
    if not 0.0 <= float(w) < 1.0:
        raise ValueError(f"w={w} outside [0, 1)")
    P, dev = src.shape[0], src.device
    s2 = _f64_per_pair("sigma2", sigma2, P, dev)
    T = None if transform is None else _f64_per_pair("transform", transform, P, dev, (4, 4))
    out = _estep(src, tgt, _counts("n_src", n_src, P, dev), _counts("n_tgt", n_tgt, P, dev),
                 T, s2, w)
    if single:
        out = tuple(o[0] for o in out)
    if np_in:
        out = tuple(o.cpu().numpy() for o in out)
        if single:
            out = out[:3] + (float(out[3]),)
    return out


@dataclass
class CpdBatchResult:
    """Per-pair outputs of ``register_batch`` (device tensors)."""
    transformation: torch.Tensor   # (P, 4, 4) f64: s R or the affine B in the 3x3 block, t in the last column
    scale: torch.Tensor            # (P,) f64: s (1 for rigid without scale and for affine)
    sigma2: torch.Tensor           # (P,) f64
    q: torch.Tensor                # (P,) f64
    iters: torch.Tensor            # (P,) int32: iterations run
    status: torch.Tensor           # (P,) int32: 0 ok, 1 empty cloud, 2 non-finite sigma2 or q


def register_batch(src, tgt, n_src=None, n_tgt=None, kind="rigid_scale", w=0.0, maxiter=50, tol=1e-3, init=None):
    """Rigid (``"rigid"``, 0), rigid + scale (``"rigid_scale"``, 1) or affine
    (``"affine"``, 2) CPD of ``P`` pairs in one call: ``src (P, Mmax, 3)`` moves
    onto ``tgt (P, Nmax, 3)``; ``n_src`` / ``n_tgt (P)`` give the valid counts of a
    ragged batch (rows past them are never read).  ``init`` is an optional
    ``(4, 4)`` or ``(P, 4, 4)`` starting transform.  ``tol <= 0`` runs exactly
    ``maxiter`` iterations.  Everything is enqueued on torch's current stream
    (capturable in a ``torch.cuda.graph``); what a 200-pair dataset run should
    call.  With ``tol > 0`` and outside a capture the call synchronises that
    stream after every eighth iteration to read how many pairs have stopped, and
    drops the launches left once all have; ``tol <= 0`` or a capture enqueues
    without any synchronisation.  Counts outside ``[0, Mmax]`` / ``[0, Nmax]``
    are clamped by the kernels.  Inputs are numpy arrays or device tensors; the
    result holds device tensors."""
    src, _ = _cloud("src", src, (3,))
    tgt, _ = _cloud("tgt", tgt, (3,))
    if src.shape[0] != tgt.shape[0] or src.device != tgt.device:
        raise ValueError(f"src {tuple(src.shape)} and tgt {tuple(tgt.shape)} must share batch size and device")
    k = KINDS.get(kind, kind)
    if k not in (0, 1, 2):
        raise ValueError(f"kind={kind!r} must be one of {sorted(KINDS)} or 0, 1, 2")
    if not 0.0 <= float(w) < 1.0:
        raise ValueError(f"w={w} outside [0, 1)")
    P, M, N, dev = src.shape[0], src.shape[1], tgt.shape[1], src.device
    ns, nt = _counts("n_src", n_src, P, dev), _counts("n_tgt", n_tgt, P, dev)
    T0 = None if init is None else _f64_per_pair("init", init, P, dev, (4, 4))
    T = torch.eye(4, dtype=torch.float64, device=dev).repeat(P, 1, 1)
    scale = torch.ones(P, dtype=torch.float64, device=dev)
    sigma2 = torch.zeros(P, dtype=torch.float64, device=dev)
    q = torch.zeros(P, dtype=torch.float64, device=dev)
    iters = torch.zeros(P, dtype=torch.int32, device=dev)
    status = torch.zeros(P, dtype=torch.int32, device=dev)
    scratch = _scratch(P, M, N, dev)
    with torch.cuda.device(dev):
        _lib.call("pcr_cpd_register", _lib.ptr(src), _lib.ptr(tgt), P, M, N, _lib.ptr(ns), _lib.ptr(nt), int(k),
                  float(w), int(maxiter), float(tol), _lib.ptr(T0), _lib.ptr(T), _lib.ptr(scale), _lib.ptr(sigma2),
                  _lib.ptr(q), _lib.ptr(iters), _lib.ptr(status), _lib.ptr(scratch), _lib.stream_handle(dev))
    return CpdBatchResult(T, scale, sigma2, q, iters, status)


def _points(points, f):
    """Apply f (on an f64 device tensor) to numpy or device points, keeping kind and dtype."""
    if isinstance(points, np.ndarray):
        out = f(torch.from_numpy(np.ascontiguousarray(points, dtype=np.float64)).to(_device()))
        return out.cpu().numpy().astype(points.dtype if points.dtype.kind == "f" else np.float64)
    if not isinstance(points, torch.Tensor) or not points.is_cuda:
        raise ValueError("points must be a numpy array or a CUDA (ROCm/HIP) tensor")
    return f(points.to(torch.float64)).to(points.dtype)


def _like(t, as_numpy):
    return t.cpu().numpy() if as_numpy else t


class RigidTransformation:
    """``scale * points @ rot.T + t`` (probreg's ``RigidTransformation``)."""

    def __init__(self, rot, t, scale):
        self.rot, self.t, self.scale = rot, t, scale

    def transform(self, points):
        dev = _device()
        rot, t = torch.as_tensor(self.rot, device=dev), torch.as_tensor(self.t, device=dev)
        return _points(points, lambda p: float(self.scale) * (p @ rot.T) + t)


class AffineTransformation:
    """``points @ b.T + t`` (probreg's ``AffineTransformation``)."""

    def __init__(self, b, t):
        self.b, self.t = b, t

    def transform(self, points):
        dev = _device()
        b, t = torch.as_tensor(self.b, device=dev), torch.as_tensor(self.t, device=dev)
        return _points(points, lambda p: p @ b.T + t)


class NonRigidTransformation:
    """``points + g @ w`` for the source points the Gram matrix ``g`` was built
    on (probreg's ``NonRigidTransformation``)."""

    def __init__(self, g, w):
        self.g, self.w = g, w

    def transform(self, points):
        dev = _device()
        g, w = torch.as_tensor(self.g, device=dev), torch.as_tensor(self.w, device=dev)
        if tuple(points.shape) != (g.shape[0], 3):
            raise ValueError(f"points must be the {g.shape[0]} source points of the registration")
        return _points(points, lambda p: p + g @ w)


class _Cpd:
    def __init__(self, source, use_cuda=True):
        if not use_cuda:
            raise ValueError("use_cuda=False: this module has no CPU path")
        self._source, self._numpy = _cloud("source", source, (2,))

    def _target(self, target):
        tgt, was_np = _cloud("target", target, (2,))
        if was_np != self._numpy or tgt.device != self._source.device:
            raise ValueError("source and target must be of one kind (numpy or device tensors) and device")
        return tgt


class RigidCPD(_Cpd):
    """``probreg.cpd.RigidCPD(source, update_scale=True, use_cuda=True)``."""

    def __init__(self, source, update_scale=True, tf_init_params=None, use_cuda=True):
        super().__init__(source, use_cuda)
        self.update_scale = bool(update_scale)
        self.tf_init_params = tf_init_params or {}

    def _init(self):
        p = self.tf_init_params
        if not p:
            return None
        dev = self._source.device
        T = torch.eye(4, dtype=torch.float64, device=dev)
        T[:3, :3] = float(p.get("scale", 1.0)) * torch.as_tensor(p.get("rot", np.eye(3)), dtype=torch.float64, device=dev)
        T[:3, 3] = torch.as_tensor(p.get("t", np.zeros(3)), dtype=torch.float64, device=dev)
        return T

    def _run(self, target, kind, w, maxiter, tol, init):
        tgt = self._target(target)
        r = register_batch(self._source[None], tgt[None], kind=kind, w=w, maxiter=maxiter, tol=tol, init=init)
        if int(r.status[0]) == 1:
            raise ValueError("source and target must not be empty")
        return r

    def registration(self, target, w=0.0, maxiter=50, tol=0.001):
        r = self._run(target, 1 if self.update_scale else 0, w, maxiter, tol, self._init())
        s = float(r.scale[0])
        T = r.transformation[0]
        tf = RigidTransformation(_like(T[:3, :3] / s, self._numpy), _like(T[:3, 3].clone(), self._numpy), s)
        return tf, float(r.sigma2[0]), float(r.q[0])


class AffineCPD(RigidCPD):
    """``probreg.cpd.AffineCPD(source, use_cuda=True)``."""

    def __init__(self, source, tf_init_params=None, use_cuda=True):
        _Cpd.__init__(self, source, use_cuda)
        self.tf_init_params = tf_init_params or {}

    def _init(self):
        p = self.tf_init_params
        if not p:
            return None
        dev = self._source.device
        T = torch.eye(4, dtype=torch.float64, device=dev)
        T[:3, :3] = torch.as_tensor(p.get("b", np.eye(3)), dtype=torch.float64, device=dev)
        T[:3, 3] = torch.as_tensor(p.get("t", np.zeros(3)), dtype=torch.float64, device=dev)
        return T

    def registration(self, target, w=0.0, maxiter=50, tol=0.001):
        r = self._run(target, 2, w, maxiter, tol, self._init())
        T = r.transformation[0]
        tf = AffineTransformation(_like(T[:3, :3].clone(), self._numpy), _like(T[:3, 3].clone(), self._numpy))
        return tf, float(r.sigma2[0]), float(r.q[0])


class NonRigidCPD(_Cpd):
    """``probreg.cpd.NonRigidCPD(source, beta=2.0, lmd=2.0, use_cuda=True)``: the
    E-step is the library's, the ``(M, M)`` f64 solve is ``torch.linalg.solve``
    on the device, and q is read once per iteration for the stop test."""

    def __init__(self, source, beta=2.0, lmd=2.0, use_cuda=True):
        super().__init__(source, use_cuda)
        self.beta, self.lmd = float(beta), float(lmd)

    def registration(self, target, w=0.0, maxiter=50, tol=0.001):
        tgt = self._target(target)
        Y32 = self._source
        M, N, dev = Y32.shape[0], tgt.shape[0], Y32.device
        if M == 0 or N == 0:
            raise ValueError("source and target must not be empty")
        if not 0.0 <= float(w) < 1.0:
            raise ValueError(f"w={w} outside [0, 1)")
        Y, X = Y32.to(torch.float64), tgt.to(torch.float64)
        G = torch.exp(-torch.cdist(Y, Y, compute_mode="donot_use_mm_for_euclid_dist").square() / (2.0 * self.beta ** 2))
        W = torch.zeros(M, 3, dtype=torch.float64, device=dev)
        eye = torch.eye(M, dtype=torch.float64, device=dev)
        xx = (X * X).sum(1)
        # the initial sigma2 of the contract, about x_0
        xc, yc = X - X[0], Y - X[0]
        sigma2 = ((M * (xc * xc).sum() + N * (yc * yc).sum() - 2.0 * (xc.sum(0) @ yc.sum(0))) / (3.0 * M * N)).reshape(1)
        eps = float(np.finfo(np.float32).eps)
        q, q_prev = 0.0, None
        for it in range(int(maxiter)):
            ts = (Y + G @ W).to(torch.float32)
            pt1, p1, px, _ = _estep(ts[None], tgt[None], None, None, None, sigma2, w)
            pt1, p1, px = pt1[0].double(), p1[0].double(), px[0].double()
            n_p = p1.sum()
            W = torch.linalg.solve(p1[:, None] * G + (self.lmd * sigma2) * eye, px - p1[:, None] * Y)
            TY = Y + G @ W
            resid = (pt1 @ xx) - 2.0 * (px * TY).sum() + (p1 @ (TY * TY).sum(1))
            sigma2 = torch.clamp(resid / (3.0 * n_p), min=eps).reshape(1)
            q = float(resid / (2.0 * sigma2[0]) + 1.5 * n_p * torch.log(sigma2[0]) + 0.5 * self.lmd * (W * (G @ W)).sum())
            if it >= 1 and abs(q - q_prev) < tol:
                break
            q_prev = q
        tf = NonRigidTransformation(_like(G, self._numpy), _like(W, self._numpy))
        return tf, float(sigma2[0]), q
