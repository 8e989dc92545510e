"""f4: the NDP level optimisation as one captured HIP graph per level.

``optimize_deformation_pyramid(src_pcd, tgt_pcd, inds, config, landmarks=None)``
is Registration.optimize_deformation_pyramid (c2p-net/deformationpyramid/model/
registration.py:149-289), both branches.  Without landmarks (the path the C2P
pipeline runs):

  * centre both clouds (:171-174);
  * for each level: Adam(lr) on that level's parameters only, up to ``iters``
    iterations of  warp(level) -> truncated Chamfer of the ``inds`` subset
    (trunc 1e9, :236) [+ w_reg * BCE(nonrigidity, 0) for level > 0, :241-245] ->
    early-stop rule (:246-256) -> backward -> step; the warped sample feeds the
    next level (:268-270);
  * final warp of the whole source through every level (:280-285).

MI355X mapping: one iteration = the layer's MLP forward/backward (hipBLASLt via
torch autograd), the truncated Chamfer on libpcr's nnd kernels (a1/a2/a3), and
two libpcr kernels -- ``pcr_ndp_control`` (the early-stop rule evaluated on the
device) and ``pcr_adam_masked`` (Adam for all tensors of the level, skipped once
the rule fired) -- captured once per level with torch.cuda.graph and replayed
``iters`` times with no host round trip (the reference synchronises on
``loss.item()`` every iteration).  The final all-level warp is libpcr's
pcr_ndp_warp (a10).  Supported: every head of the reference's NDPLayer --
``motion_type`` "SE3", "Sim3" or "sflow" with ``rotation_format`` "axis_angle",
"euler", "quaternion" or "6D" (config/NDP.yaml ships SE3 / axis_angle, the C5
configuration) -- on the fused kernels and on the torch path alike.

With ``landmarks = (src_ldmk (L, 3), tgt_ldmk (L, 3))`` (the branch
config/LNDP.yaml and Registration.load_pcds(..., landmarks=...) drive, :185-227,
266-273): the landmarks are centred by the means of the whole clouds; mode A
(``w_cd > 0``) warps cat([src_ldmk, s_sample]) each iteration, loss =
mean_k sum_c (warped_ldmk - tgt_ldmk)^2 + w_cd * Chamfer of all warped samples
truncated at ``trunc_cd``; mode B (``w_cd <= 0``) warps the landmarks alone, loss =
the landmark term; the BCE regulariser's mean runs over the warped points (L + N
or L); the warped landmarks feed the next level in both modes, the warped samples
in mode A only.  ``w_ldmk`` is in the yaml and never read by the reference, nor
here.  On the fused path the landmark rows ride in front of the samples in one
(L + N, 3) level input, the backward takes their gradient f32(2 / L) (x' - tgt)
from the level output (the landmark block of pcr_ndp_train) and
``pcr_ndp_ldmk_loss`` makes the loss and applies the early-stop rule; the level
graph stays one linear chain.  ``hist`` in mode B holds the final warp only,
(1, N, 3): the reference raises NameError where it records a level there
(:264, ``s_sample_warped`` is never bound), so there is nothing to match.
Measured on one MI355X (N = M = 20,000, L = 1,000, 9 levels x 40 iterations):
mode A replays in 1.015 x the time of the no-landmark loop on all N points, the
torch path in 12.6 x ("Landmark-guided optimisation").
"""
from __future__ import annotations

import ctypes
import os
import time
from dataclasses import dataclass

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as Fn

from . import _lib
from .chamfer import compute_truncated_chamfer_distance
from .ndp import MOTIONS, ROT_ROWS, ROTATION_FORMATS, head_code, warp_pyramid


@dataclass
class NDPConfig:
    """config/NDP.yaml:8-32 (the fields optimize_deformation_pyramid reads)."""
    iters: int = 40
    lr: float = 0.01
    max_break_count: int = 15
    break_threshold_ratio: float = 0.001
    w_reg: float = 0.05
    m: int = 9
    k0: int = -8
    depth: int = 3
    width: int = 128
    motion_type: str = "SE3"
    rotation_format: str = "axis_angle"
    # config/LNDP.yaml:16,19 -- read only when landmarks are given
    w_cd: float = 0.0
    trunc_cd: float = 0.25

    @classmethod
    def from_any(cls, cfg):
        if isinstance(cfg, cls):
            return cfg
        get = (lambda k, d: cfg.get(k, d)) if isinstance(cfg, dict) else \
            (lambda k, d: getattr(cfg, k, d))
        out = cls()
        for k in out.__dataclass_fields__:
            setattr(out, k, type(getattr(out, k))(get(k, getattr(out, k))))
        return out


# --------------------------------------------------------------------------
# mirror of the reference modules (same parameter names: state dicts load
# into either), nets.py:66-177 and rigid_body.py:5-119
# --------------------------------------------------------------------------


class _MLP(nn.Module):
    def __init__(self, depth, width):
        super().__init__()
        self.pts_linears = nn.ModuleList([nn.Linear(width, width) for _ in range(depth - 1)])

    def forward(self, x):
        for lin in self.pts_linears:
            x = Fn.relu(lin(x))
        return x


def _skew(w):
    z = torch.zeros_like(w[..., 0])
    return torch.stack([z, -w[..., 2], w[..., 1], w[..., 2], z, -w[..., 0],
                        -w[..., 1], w[..., 0], z], dim=-1).reshape((-1, 3, 3))


def _euler_to_so3(a):
    """Rx(a0) Ry(a1) Rz(a2) (rigid_body.euler_to_SO3, convention X, Y, Z)."""
    c, s = torch.cos(a), torch.sin(a)
    one, zero = torch.ones_like(a[..., 0]), torch.zeros_like(a[..., 0])

    def mat(*flat):
        return torch.stack(flat, dim=-1).reshape(a.shape[:-1] + (3, 3))
    Rx = mat(one, zero, zero, zero, c[..., 0], -s[..., 0], zero, s[..., 0], c[..., 0])
    Ry = mat(c[..., 1], zero, s[..., 1], zero, one, zero, -s[..., 1], zero, c[..., 1])
    Rz = mat(c[..., 2], -s[..., 2], zero, s[..., 2], c[..., 2], zero, zero, zero, one)
    return torch.matmul(torch.matmul(Rx, Ry), Rz)


def _quaternion_to_so3(o):
    """o / copysign(|o|, o[0]) then rigid_body.quaternion_to_SO3 (nets.py:154-157)."""
    n = torch.sqrt((o * o).sum(-1))
    q = o / torch.where(o[..., 0] < 0, -n, n)[..., None]
    r, i, j, k = torch.unbind(q, -1)
    two_s = 2.0 / (q * q).sum(-1)
    flat = (1 - two_s * (j * j + k * k), two_s * (i * j - k * r), two_s * (i * k + j * r),
            two_s * (i * j + k * r), 1 - two_s * (i * i + k * k), two_s * (j * k - i * r),
            two_s * (i * k - j * r), two_s * (j * k + i * r), 1 - two_s * (i * i + j * j))
    return torch.stack(flat, -1).reshape(q.shape[:-1] + (3, 3))


def _6d_to_so3(d6):
    """rigid_body._6d_to_SO3: Gram-Schmidt of the two 3-vectors, rows b1, b2, b1 x b2."""
    a1, a2 = d6[..., :3], d6[..., 3:]
    b1 = Fn.normalize(a1, dim=-1)
    b2 = Fn.normalize(a2 - (b1 * a2).sum(-1, keepdim=True) * b1, dim=-1)
    return torch.stack((b1, b2, torch.cross(b1, b2, dim=-1)), dim=-2)


class NDPLayer(nn.Module):
    """NDPLayer(depth, width, k0, m, rotation_format, nonrigidity_est, motion) of the
    reference, every head; keyword order differs (rotation_format defaults to
    "axis_angle", the shipped configuration)."""

    def __init__(self, depth, width, k0, m, nonrigidity_est=False, rotation_format="axis_angle",
                 motion="SE3"):
        super().__init__()
        head_code(motion, rotation_format)  # ValueError listing the choices
        self.k0, self.m = k0, m
        self.motion, self.rotation_format = motion, rotation_format
        self.nonrigidity_est = nonrigidity_est
        self.input = nn.Sequential(nn.Linear(6, width), nn.ReLU())
        self.mlp = _MLP(depth, width)
        if motion != "sflow":
            self.rot_brach = nn.Linear(width, ROT_ROWS[rotation_format])
            if motion == "Sim3":
                self.s_branch = nn.Linear(width, 1)
        self.trn_branch = nn.Linear(width, 3)
        if nonrigidity_est:
            self.nr_branch = nn.Linear(width, 1)
        self.mlp_scale = 0.001
        for p in self.parameters():
            if p.dim() > 1:
                nn.init.xavier_uniform_(p)

    def posenc(self, pos):
        mul = 2 ** (self.m + self.k0)
        x, y, z = pos[..., 0:1], pos[..., 1:2], pos[..., 2:3]
        return torch.cat([torch.sin(x * mul), torch.cos(x * mul), torch.sin(y * mul),
                          torch.cos(y * mul), torch.sin(z * mul), torch.cos(z * mul)], dim=-1)

    def forward(self, x):
        fea = self.mlp(self.input(self.posenc(x)))
        t = self.mlp_scale * self.trn_branch(fea)
        if self.motion == "sflow":
            x_ = x + t
        else:
            Rx = (self.get_rotation(fea) @ x[..., None]).squeeze()
            if self.motion == "Sim3":
                Rx = (self.mlp_scale * self.s_branch(fea) + 1) * Rx  # starts at scale 1
            x_ = Rx + t
        if self.nonrigidity_est:
            nr = torch.sigmoid(self.mlp_scale * self.nr_branch(fea))
            x_ = x + nr * (x_ - x)
            nr = nr.squeeze()
        else:
            nr = None
        return x_.squeeze(), nr

    def get_rotation(self, fea):
        r = self.mlp_scale * self.rot_brach(fea)
        if self.rotation_format == "euler":
            return _euler_to_so3(r)
        if self.rotation_format == "quaternion":
            return _quaternion_to_so3(r)
        if self.rotation_format == "6D":
            return _6d_to_so3(r)
        theta = torch.norm(r, dim=-1, keepdim=True)
        W = _skew(r / theta)
        th = theta[..., None]
        return torch.eye(3, device=fea.device)[None] + torch.sin(th) * W + (1 - torch.cos(th)) * W @ W


class DeformationPyramid:
    """Deformation_Pyramid(depth, width, device, k0, m, rotation_format,
    nonrigidity_est, motion) (nets.py:10-65)."""

    def __init__(self, depth, width, device, k0, m, nonrigidity_est=False, rotation_format="axis_angle",
                 motion="SE3"):
        self.motion, self.rotation_format = motion, rotation_format
        self.pyramid = [NDPLayer(depth, width, k0, i + 1, nonrigidity_est and i != 0, rotation_format,
                                 motion).to(device) for i in range(m)]
        self.n_hierarchy = m

    def warp(self, x, max_level=None, min_level=0):
        max_level = self.n_hierarchy - 1 if max_level is None else max_level
        data = {}
        for i in range(min_level, max_level + 1):
            x, nr = self.pyramid[i](x)
            data[i] = (x, nr)
        return x, data

    def gradient_setup(self, optimized_level):
        for i, net in enumerate(self.pyramid):
            for p in net.parameters():
                p.requires_grad = i == optimized_level


# --------------------------------------------------------------------------
# one level
# --------------------------------------------------------------------------


class _AdamTensor(ctypes.Structure):
    _fields_ = [("param", ctypes.c_void_p), ("grad", ctypes.c_void_p), ("exp_avg", ctypes.c_void_p),
                ("exp_avg_sq", ctypes.c_void_p), ("n", ctypes.c_int32), ("reserved", ctypes.c_int32)]


def _bce_to_zero(p):
    """nn.BCELoss()(p, zeros): mean(-max(log(1 - p), -100))."""
    return torch.mean(-torch.clamp(torch.log(1 - p), min=-100.0))


class _Level:
    CHECK = 8  # iterations between the host's looks at the early-stop flag
    # iterations per captured graph (PCR_NDP_GRAPH_STEPS): each graph launch costs
    # a gap of ~8 us on the device; more steps per graph cost capture time
    GRAPH_STEPS = int(os.environ.get("PCR_NDP_GRAPH_STEPS", "2"))

    def __init__(self, layer, s_sample, t_sample, inds, level, cfg: NDPConfig, shared=None, ldmk=None):
        dev = s_sample.device
        # landmark mode (registration.py:211-227): ldmk = (L, tgt_ldmk (L, 3), "A" | "B");
        # s_sample is then the level's whole input, cat([src_ldmk, samples]) in mode A
        # and src_ldmk alone in mode B, and inds is not used
        self.ldmk = ldmk
        # buffers that do not depend on the level (same N, K, M on every level of a
        # pyramid) are allocated once per optimize_deformation_pyramid call
        self.shared = {} if shared is None else shared
        self.layer, self.level, self.cfg = layer, level, cfg
        self.s, self.t, self.inds = s_sample, t_sample, inds
        self.params = [p for p in layer.parameters()]
        # gradients and Adam moments: views of one buffer (one fill per reset)
        sizes = [p.numel() for p in self.params]
        self._gmv = torch.zeros(3, sum(sizes), dtype=self.params[0].dtype, device=dev)
        self.grads, self.m, self.v = ([t.view_as(p) for t, p in zip(self._gmv[r].split(sizes), self.params)]
                                      for r in range(3))
        self.loss = torch.zeros((), dtype=torch.float32, device=dev)
        self.warped = torch.zeros_like(s_sample)
        self.state = torch.zeros(8, dtype=torch.float64, device=dev)
        # loss of every replay (the first state[6] are the evaluated iterations)
        self.log = torch.zeros(cfg.iters + 1, dtype=torch.float32, device=dev)
        self.ctr = torch.zeros(1, dtype=torch.long, device=dev)
        tab = (_AdamTensor * len(self.params))()
        for k, (p, g, m, v) in enumerate(zip(self.params, self.grads, self.m, self.v)):
            tab[k] = _AdamTensor(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), 0)
        raw = np.frombuffer(bytes(tab), dtype=np.uint8).copy()
        self.table = torch.from_numpy(raw).to(dev)
        self.max_numel = max(p.numel() for p in self.params)
        self.reset()

    def reset(self):
        """Fresh optimizer + early-stop state (registration.py:202-206)."""
        st0 = self.shared.get("state0")
        if st0 is None:  # one host -> device copy per pyramid, not per level
            st0 = torch.tensor([1.0, 0.0, 1e6, 0.0, 0.0, 0.0, 0.0, 0.0], dtype=torch.float64,
                               device=self.state.device)
            self.shared["state0"] = st0
        self.state.copy_(st0)
        self._gmv[1:].zero_()
        self.ctr.zero_()

    def step(self):
        cfg = self.cfg
        warped, nr = self.layer(self.s)
        if self.ldmk is None:
            loss = compute_truncated_chamfer_distance(warped[None, self.inds], self.t[None], trunc=1e9)
        else:
            L, tgt_ldmk, mode = self.ldmk
            warped = warped.reshape(-1, 3)  # the layer squeezes a single point to (3,)
            loss = torch.mean(torch.sum((warped[:L] - tgt_ldmk) ** 2, dim=-1))
            if mode == "A":
                loss = loss + cfg.w_cd * compute_truncated_chamfer_distance(
                    warped[None, L:], self.t[None], trunc=cfg.trunc_cd)
        if self.level > 0 and cfg.w_reg > 0:
            loss = loss + cfg.w_reg * _bce_to_zero(nr)
        grads = torch.autograd.grad(loss, self.params)
        for gs, g in zip(self.grads, grads):
            gs.copy_(g)
        self.loss.copy_(loss.detach())
        self.log.index_copy_(0, torch.clamp(self.ctr, max=self.cfg.iters), self.loss.reshape(1))
        self.ctr += 1
        self.warped.copy_(warped.detach())
        st = _lib.stream_handle(self.s.device)
        _lib.call("pcr_ndp_control", _lib.ptr(self.loss), _lib.ptr(self.state),
                  float(cfg.break_threshold_ratio), int(cfg.max_break_count), 1e-4, st)
        _lib.call("pcr_adam_masked", _lib.ptr(self.table), len(self.params), self.max_numel,
                  _lib.ptr(self.state), float(cfg.lr), 0.9, 0.999, 1e-8, st)

    def needs_warmup(self):
        return True  # torch autograd: its allocations must precede the capture

    def run(self, use_graph=True):
        iters = self.cfg.iters
        if not use_graph or iters <= 1:
            for _ in range(iters):
                self.step()
            return
        side = torch.cuda.Stream(device=self.s.device)
        side.wait_stream(torch.cuda.current_stream())
        if self.needs_warmup():
            # warm-up on a side stream (allocator pools, library handles, libpcr
            # workspaces) then restore parameters and optimizer state
            keep = [p.detach().clone() for p in self.params]
            with torch.cuda.stream(side):
                self.step()
            torch.cuda.current_stream().wait_stream(side)
            with torch.no_grad():
                for p, k in zip(self.params, keep):
                    p.copy_(k)
            self.reset()
            side.wait_stream(torch.cuda.current_stream())
        # capture on the side stream (torch.cuda.graph would also synchronise the
        # device and run the garbage collector, ~1 ms per level)
        # a graph of `spg` iterations (the iterations are gated on the rule, so a
        # graph that runs past the stop is a no-op from there on), and one of
        # the remainder
        spg = max(1, min(self.GRAPH_STEPS, iters))
        graphs = {}
        for n in {spg, iters % spg} - {0}:
            g = torch.cuda.CUDAGraph()
            with torch.cuda.stream(side):
                g.capture_begin()
                try:
                    for _ in range(n):
                        self.step()
                finally:
                    g.capture_end()
            graphs[n] = g
        torch.cuda.current_stream().wait_stream(side)
        self.capture_done = time.perf_counter()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        done, seen = 0, 0
        while done < iters:
            n = spg if iters - done >= spg else iters - done
            graphs[n].replay()
            done += n
            # the replays after the rule fired are no-ops (gated kernels); every
            # CHECK iterations the host looks whether the level has stopped and
            # skips the rest (one 8-byte read; the results do not depend on it)
            if done - seen >= self.CHECK and done < iters:
                seen = done
                if self.state[0].item() == 0.0:
                    break
        ev[1].record()
        self.replay_events = ev


class _NdpLevelC(ctypes.Structure):
    _fields_ = [(n, ctypes.c_void_p) for n in ("w_in", "b_in", "w_hid", "b_hid", "w_rot", "b_rot",
                                               "w_trn", "b_trn", "w_nr", "b_nr")] + \
        [("m", ctypes.c_int32), ("reserved", ctypes.c_int32), ("w_s", ctypes.c_void_p),
         ("b_s", ctypes.c_void_p), ("head", ctypes.c_int32), ("reserved2", ctypes.c_int32)]


class _TrainC(ctypes.Structure):
    """pcr_ndp_train (include/pcr_api.h)."""
    _fields_ = [("x", ctypes.c_void_p), ("N", ctypes.c_int32), ("width", ctypes.c_int32),
                ("depth", ctypes.c_int32), ("k0", ctypes.c_int32), ("level", _NdpLevelC),
                ("w_hid", ctypes.c_void_p * 4), ("b_hid", ctypes.c_void_p * 4),
                ("pe", ctypes.c_void_p), ("H", ctypes.c_void_p), ("aux", ctypes.c_void_p),
                ("x_out", ctypes.c_void_p), ("g", ctypes.c_void_p), ("bce_scale", ctypes.c_double),
                ("dO", ctypes.c_void_p), ("D", ctypes.c_void_p),
                ("inv", ctypes.c_void_p), ("xs", ctypes.c_void_p), ("gsub", ctypes.c_void_p),
                ("gacc", ctypes.c_void_p), ("gacc_k", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("ldmk_tgt", ctypes.c_void_p), ("ldmk_n", ctypes.c_int32), ("reserved3", ctypes.c_int32),
                ("cd_scale", ctypes.c_double)]

GACC_REPLICAS = 16  # PCR_NDP_GACC_REPLICAS (include/pcr_api.h)


class _ChamferC(ctypes.Structure):
    """pcr_ndp_chamfer (include/pcr_api.h)."""
    _fields_ = [("xs", ctypes.c_void_p), ("tgt", ctypes.c_void_p), ("K", ctypes.c_int32),
                ("M", ctypes.c_int32), ("trunc", ctypes.c_double), ("d1", ctypes.c_void_p),
                ("d2", ctypes.c_void_p), ("i1", ctypes.c_void_p), ("i2", ctypes.c_void_p),
                ("gacc", ctypes.c_void_p), ("scratch", ctypes.c_void_p)]


class _LevelFused(_Level):
    """One level with the warp forward/backward and the weight gradients on libpcr
    kernels (csrc/ndp_train.hip) instead of torch autograd; same loss, same
    early-stop rule and Adam (pcr_ndp_control / pcr_adam_masked)."""

    # points per weight-gradient partial (split-K chunk; PCR_NDP_CHUNK: a tuning hook)
    CHUNK = int(os.environ.get("PCR_NDP_CHUNK", "128"))

    def __init__(self, layer, s_sample, t_sample, inds, level, cfg: NDPConfig, shared=None, ldmk=None):
        sd = dict(layer.named_parameters())
        self.W = sd["input.0.weight"].shape[0]
        self.nhid = sum(1 for k in sd if k.startswith("mlp.pts_linears.") and k.endswith(".weight"))
        if self.W != 128 or self.nhid > 4:
            raise NotImplementedError("fused NDP training: width 128, depth <= 5")
        super().__init__(layer, s_sample, t_sample, inds, level, cfg, shared, ldmk)
        dev, N, W, d = s_sample.device, s_sample.shape[0], self.W, self.nhid + 1
        f32 = dict(dtype=torch.float32, device=dev)
        i32 = dict(dtype=torch.int32, device=dev)
        # landmark mode: N = L + K points in mode A (the K samples are the Chamfer
        # subset, all of them), N = L in mode B (K = 0: no Chamfer pass)
        L, mode = (ldmk[0], ldmk[2]) if ldmk is not None else (0, None)
        K = inds.shape[0] if ldmk is None else N - L
        # the scratch of the kernels depends on (N, W, depth, K, M) only: shared by
        # the levels of one pyramid (keyed by those sizes)
        key = (N, W, d, K, t_sample.shape[0], t_sample.data_ptr(), inds.data_ptr() if ldmk is None else -L)

        def buf(name, make):
            k = (name,) + key
            b = self.shared.get(k)
            if b is None:
                b = make()
                self.shared[k] = b
            return b
        self._buf = buf
        self.N = N
        self.pe = buf("pe", lambda: torch.zeros(6, N, **f32))
        self.H = buf("H", lambda: torch.zeros(d, W, N, **f32))
        # the head's row map, from the library (include/pcr_api.h: pcr_ndp_head_rows)
        self.head = head = head_code(getattr(layer, "motion", "SE3"),
                                     getattr(layer, "rotation_format", "axis_angle"))
        lib = _lib.load()
        rot_n, rows, brows, trn0, nr0, sc0 = (int(lib.pcr_ndp_head_rows(head, k)) for k in range(6))
        self.nr_row = nr0
        self.aux = buf(f"aux{rows}", lambda: torch.zeros(rows, N, **f32))
        self.dO = buf(f"dO{rows}", lambda: torch.zeros(rows, N, **f32))
        self.D = buf("D", lambda: torch.zeros(d, W, N, **f32))
        self.gx = buf("gx", lambda: torch.zeros(N, 3, **f32))
        self.xo = self.warped  # the forward writes the level output in place
        nparts = lib.pcr_ndp_train_partial_floats_head(N, W, d, self.CHUNK, head)
        self.part = buf(f"part{brows}", lambda: torch.zeros(max(int(nparts), 1), **f32))
        # gradient buffers in the kernel's order; the Adam table must see the same
        # storage, so the branch parameters' grads are row views of one buffer
        self.gw_b = buf(f"gw_b{brows}", lambda: torch.zeros(brows, W, **f32))
        self.gb_b = buf(f"gb_b{brows}", lambda: torch.zeros(brows, **f32))
        names = [n for n, _ in layer.named_parameters()]
        view = {"rot_brach.weight": self.gw_b[0:rot_n], "rot_brach.bias": self.gb_b[0:rot_n],
                "trn_branch.weight": self.gw_b[trn0:trn0 + 3], "trn_branch.bias": self.gb_b[trn0:trn0 + 3],
                "nr_branch.weight": self.gw_b[nr0:nr0 + 1], "nr_branch.bias": self.gb_b[nr0:nr0 + 1]}
        if sc0 >= 0:
            view.update({"s_branch.weight": self.gw_b[sc0:sc0 + 1], "s_branch.bias": self.gb_b[sc0:sc0 + 1]})
        own = {n: buf("g:" + n, lambda p=p: torch.zeros_like(p)) for n, p in layer.named_parameters() if n not in view}
        order = ["input.0.weight", "input.0.bias"]
        for k in range(self.nhid):
            order += [f"mlp.pts_linears.{k}.weight", f"mlp.pts_linears.{k}.bias"]
        kernel_grads = [own[n] for n in order] + [self.gw_b, self.gb_b]
        self.grad_ptrs = (ctypes.c_void_p * len(kernel_grads))(*[g.data_ptr() for g in kernel_grads])
        self._keep = kernel_grads
        self.grads = [view[n] if n in view else own[n] for n in names]
        self._rebuild_table()
        t = _TrainC()
        t.x, t.N, t.width, t.depth, t.k0 = s_sample.data_ptr(), N, W, d, int(layer.k0)
        lv = _NdpLevelC()
        lv.w_in, lv.b_in = sd["input.0.weight"].data_ptr(), sd["input.0.bias"].data_ptr()
        lv.head = head
        if "rot_brach.weight" in sd:
            lv.w_rot, lv.b_rot = sd["rot_brach.weight"].data_ptr(), sd["rot_brach.bias"].data_ptr()
        if "s_branch.weight" in sd:
            lv.w_s, lv.b_s = sd["s_branch.weight"].data_ptr(), sd["s_branch.bias"].data_ptr()
        lv.w_trn, lv.b_trn = sd["trn_branch.weight"].data_ptr(), sd["trn_branch.bias"].data_ptr()
        self.has_nr = "nr_branch.weight" in sd
        if self.has_nr:
            lv.w_nr, lv.b_nr = sd["nr_branch.weight"].data_ptr(), sd["nr_branch.bias"].data_ptr()
        lv.m = int(layer.m)
        t.level = lv
        for k in range(self.nhid):
            t.w_hid[k] = sd[f"mlp.pts_linears.{k}.weight"].data_ptr()
            t.b_hid[k] = sd[f"mlp.pts_linears.{k}.bias"].data_ptr()
        t.pe, t.H, t.aux, t.x_out = (self.pe.data_ptr(), self.H.data_ptr(), self.aux.data_ptr(),
                                     self.xo.data_ptr())
        t.g = self.gx.data_ptr()
        self.bce_on = level > 0 and cfg.w_reg > 0 and self.has_nr
        t.bce_scale = (cfg.w_reg / N) if self.bce_on else 0.0
        t.dO, t.D = self.dO.data_ptr(), self.D.data_ptr()
        M = t_sample.shape[0]
        self.K, self.M = K, M
        if ldmk is not None:
            self.ldmk_tgt = ldmk[1].contiguous()
            t.ldmk_tgt, t.ldmk_n, t.cd_scale = self.ldmk_tgt.data_ptr(), L, float(cfg.w_cd)
            self.ldmk_scratch = buf("ldmk_scratch", lambda: torch.zeros(
                int(lib.pcr_ndp_ldmk_loss_scratch_bytes()), dtype=torch.uint8, device=dev))
            # the glue of the nnd path writes a loss of its own: kept out of the level's log
            self.glue_sink = buf("glue_sink", lambda: (torch.zeros(2, **f32), torch.zeros(1, dtype=torch.long,
                                                                                         device=dev)))
        if mode == "B":
            # every point is a landmark: no subset, no Chamfer pass, no dL/dx' buffer
            t.g = None
            self.use_inv = self.use_nc = False
            self.desc = t
            return
        self.d1 = buf("d1", lambda: torch.zeros(1, K, **f32))
        self.d2 = buf("d2", lambda: torch.zeros(1, M, **f32))
        self.gd1 = buf("gd1", lambda: torch.zeros(1, K, **f32))
        self.gd2 = buf("gd2", lambda: torch.zeros(1, M, **f32))
        # the level Chamfer's answers: shared by the levels, so each level's
        # searches start from the previous level's answers (box path, ndp_chamfer.hip)
        self.i1 = buf("i1", lambda: torch.zeros(1, K, **i32))
        self.i2 = buf("i2", lambda: torch.zeros(1, M, **i32))
        self.gsub = buf("gsub", lambda: torch.zeros(1, K, 3, **f32))
        self.gt = buf("gt", lambda: torch.zeros(1, M, 3, **f32))
        self.t3 = buf("t3", lambda: t_sample[None].contiguous())
        # duplicate-free subset: the forward writes x'[inds] and the backward reads
        # dL/dx' of the subset through inv (no gather / index_add launches)
        self.use_inv = mode == "A" or buf("use_inv", lambda: int(torch.unique(inds).numel()) == K)
        if self.use_inv:
            def make_inv():
                inv = torch.full((N,), -1, **i32)
                if mode == "A":  # inv[p] = p - L: xs is the (K, 3) block of samples
                    inv[L:] = torch.arange(K, **i32)
                else:
                    inv[inds] = torch.arange(K, **i32)
                return inv
            self.inv = buf("inv", make_inv)
            self.xs = buf("xs", lambda: torch.zeros(1, K, 3, **f32))
            t.inv, t.xs, t.gsub = self.inv.data_ptr(), self.xs.data_ptr(), self.gsub.data_ptr()
        # the level's Chamfer with its gradient in one pass (csrc/ndp_chamfer.hip):
        # the target grid built once here, the subset grid rebuilt per iteration
        # the fused pass holds each cloud's grid starts in one workgroup's LDS
        # (K, M <= pcr_ndp_chamfer_max_points()); larger clouds -- an unsampled
        # target above 32K points (c2p.register_c2p passes tgt whole, as the
        # reference's t_sample = tgt_pcd does) -- take the nnd drop-in path
        lim = int(_lib.load().pcr_ndp_chamfer_max_points())
        self.use_nc = (self.use_inv and 1 <= K <= lim and 1 <= M <= lim
                       and os.environ.get("PCR_NDP_CHAMFER", "1") != "0")
        if self.use_nc:
            lib = _lib.load()
            nbytes = int(lib.pcr_ndp_chamfer_scratch_bytes(K, M))
            self.nc_raw = buf("nc_raw", lambda: torch.empty(nbytes + 256, dtype=torch.uint8, device=dev))
            off = (-self.nc_raw.data_ptr()) % 256
            self.gacc = buf("gacc", lambda: torch.zeros(int(lib.pcr_ndp_chamfer_gacc_words(K)), dtype=torch.int64,
                                                        device=dev))
            c = _ChamferC()
            c.xs, c.tgt, c.K, c.M = self.xs.data_ptr(), self.t3.data_ptr(), K, M
            c.trunc = 1e9 if ldmk is None else float(cfg.trunc_cd)
            c.d1, c.d2, c.i1, c.i2 = (self.d1.data_ptr(), self.d2.data_ptr(), self.i1.data_ptr(),
                                      self.i2.data_ptr())
            c.gacc, c.scratch = self.gacc.data_ptr(), self.nc_raw.data_ptr() + off
            self.nc = c
            t.gacc, t.gacc_k = self.gacc.data_ptr(), K
            self.loss_scratch = buf("loss_scratch", lambda: torch.zeros(int(lib.pcr_ndp_loss_scratch_bytes()),
                                                                       dtype=torch.uint8, device=dev))
            self.xs0 = (s_sample.index_select(0, inds) if ldmk is None else s_sample[L:]).contiguous()
            _lib.call("pcr_ndp_chamfer_prepare", ctypes.byref(c), _lib.ptr(self.xs0),
                      _lib.stream_handle(dev))
        self.desc = t

    def needs_warmup(self):
        # libpcr kernels only (no allocation inside a step): one warm-up per
        # pyramid loads the code objects before the first capture
        if self.shared.get("warm"):
            return False
        self.shared["warm"] = True
        return True

    def _rebuild_table(self):
        tab = (_AdamTensor * len(self.params))()
        for k, (p, g, m, v) in enumerate(zip(self.params, self.grads, self.m, self.v)):
            tab[k] = _AdamTensor(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), 0)
        raw = np.frombuffer(bytes(tab), dtype=np.uint8).copy()
        self.table = torch.from_numpy(raw).to(self.s.device)

    def step(self):
        # every libpcr kernel of the iteration is gated on state[0]: after the
        # early-stop rule fired, the remaining replays of the level graph return
        # at once (registration.py:250-256 breaks out of the level)
        _lib.call("pcr_set_gate", _lib.ptr(self.state))
        try:
            self._step()
        finally:
            _lib.call("pcr_set_gate", None)

    def _step(self):
        cfg = self.cfg
        st = _lib.stream_handle(self.s.device)
        desc = ctypes.byref(self.desc)
        _lib.call("pcr_ndp_train_forward", desc, st)
        if self.ldmk is not None:
            # mode A: the Chamfer of all K samples with its gradient (fused pass, or
            # the nnd kernels above its size limit); then landmark term + w_cd Chamfer
            # [+ BCE over all N points] and the early-stop rule in one launch
            L, mode_a = self.ldmk[0], self.ldmk[2] == "A"
            if mode_a and self.use_nc:
                _lib.call("pcr_ndp_chamfer_step", ctypes.byref(self.nc), st)
            elif mode_a:
                self._chamfer_nnd(st)
            _lib.call("pcr_ndp_ldmk_loss", _lib.ptr(self.xo), _lib.ptr(self.ldmk_tgt), L,
                      _lib.ptr(self.d1 if mode_a else None), self.K if mode_a else 0,
                      _lib.ptr(self.d2 if mode_a else None), self.M if mode_a else 0,
                      _lib.ptr(self.aux[self.nr_row] if self.bce_on else None), self.N, float(cfg.w_cd),
                      float(cfg.w_reg), float(cfg.trunc_cd), _lib.ptr(self.loss), _lib.ptr(self.log),
                      _lib.ptr(self.ctr), int(cfg.iters), _lib.ptr(self.state), float(cfg.break_threshold_ratio),
                      int(cfg.max_break_count), 1e-4, _lib.ptr(self.ldmk_scratch), st)
            _lib.call("pcr_ndp_train_backward", desc, _lib.ptr(self.part), self.CHUNK,
                      ctypes.cast(self.grad_ptrs, ctypes.c_void_p), st)
        elif self.use_nc:
            # the Chamfer with its gradient, then the loss and the early-stop rule in one launch
            _lib.call("pcr_ndp_chamfer_step", ctypes.byref(self.nc), st)
            _lib.call("pcr_ndp_chamfer_loss", _lib.ptr(self.d1), self.K, _lib.ptr(self.d2), self.M,
                      _lib.ptr(self.aux[self.nr_row] if self.bce_on else None), self.N, float(cfg.w_reg), 1e9,
                      _lib.ptr(self.loss), _lib.ptr(self.log), _lib.ptr(self.ctr), int(cfg.iters),
                      _lib.ptr(self.state), float(cfg.break_threshold_ratio), int(cfg.max_break_count), 1e-4,
                      _lib.ptr(self.loss_scratch), st)
            _lib.call("pcr_ndp_train_backward", desc, _lib.ptr(self.part), self.CHUNK,
                      ctypes.cast(self.grad_ptrs, ctypes.c_void_p), st)
        else:
            self._chamfer_nnd(st)
            _lib.call("pcr_ndp_train_backward", desc, _lib.ptr(self.part), self.CHUNK,
                      ctypes.cast(self.grad_ptrs, ctypes.c_void_p), st)
            _lib.call("pcr_ndp_control", _lib.ptr(self.loss), _lib.ptr(self.state),
                      float(cfg.break_threshold_ratio), int(cfg.max_break_count), 1e-4, st)
        _lib.call("pcr_adam_masked", _lib.ptr(self.table), len(self.params), self.max_numel,
                  _lib.ptr(self.state), float(cfg.lr), 0.9, 0.999, 1e-8, st)

    def _chamfer_nnd(self, st):
        """The Chamfer pass on the nnd drop-in kernels (a1 forward, the glue, a2
        backward): subsets with repeated indices (no inverse map)."""
        from .nndistance import nnd_backward_cuda, nnd_forward_cuda
        cfg = self.cfg
        xs = self.xs if self.use_inv else self.xo.index_select(0, self.inds)[None].contiguous()
        nnd_forward_cuda(xs, self.t3, self.d1, self.d2, self.i1, self.i2)
        if self.ldmk is not None:
            # landmark mode: only the seeds dL/dd1, dL/dd2 of the Chamfer truncated at
            # trunc_cd (w_cd enters through cd_scale); pcr_ndp_ldmk_loss makes the loss
            sink, sink_ctr = self.glue_sink
            _lib.call("pcr_ndp_chamfer_glue", _lib.ptr(self.d1), self.K, _lib.ptr(self.d2), self.M, None, self.N,
                      0.0, float(cfg.trunc_cd), _lib.ptr(self.gd1), _lib.ptr(self.gd2), _lib.ptr(sink[0:1]),
                      _lib.ptr(sink[1:2]), _lib.ptr(sink_ctr), 0, st)
        else:
            # loss (truncated Chamfer means + BCE), dL/dd1, dL/dd2, the log entry, the counter
            _lib.call("pcr_ndp_chamfer_glue", _lib.ptr(self.d1), self.K, _lib.ptr(self.d2), self.M,
                      _lib.ptr(self.aux[self.nr_row] if self.bce_on else None), self.N, float(cfg.w_reg), 1e9,
                      _lib.ptr(self.gd1), _lib.ptr(self.gd2), _lib.ptr(self.loss), _lib.ptr(self.log),
                      _lib.ptr(self.ctr), int(cfg.iters), st)
        nnd_backward_cuda(xs, self.t3, self.gsub, self.gt, self.gd1, self.gd2, self.i1, self.i2)
        if not self.use_inv:
            self.gx.zero_()
            self.gx.index_add_(0, self.inds, self.gsub[0])


def _check_landmarks(landmarks):
    """(src_ldmk, tgt_ldmk) as (L, 3) f32 numpy / tensors, L >= 1; ValueError otherwise."""
    try:
        a, b = landmarks
    except (TypeError, ValueError):
        raise ValueError("landmarks must be a pair (src_ldmk (L, 3), tgt_ldmk (L, 3))") from None
    a, b = (torch.as_tensor(np.asarray(v) if not torch.is_tensor(v) else v, dtype=torch.float32) for v in (a, b))
    for name, v in (("src_ldmk", a), ("tgt_ldmk", b)):
        if v.dim() != 2 or v.shape[1] != 3:
            raise ValueError(f"landmarks: {name} must be (L, 3), got {tuple(v.shape)}")
    if a.shape != b.shape:
        raise ValueError(f"landmarks: {tuple(a.shape)} source against {tuple(b.shape)} target landmarks")
    if a.shape[0] < 1:
        raise ValueError("landmarks: at least one landmark pair is needed (L = 0)")
    return a, b


def optimize_deformation_pyramid(src_pcd, tgt_pcd, inds, config=None, NDP=None, use_graph=True,
                                 fused=True, landmarks=None):
    """Returns (warped_pcd (N, 3) cuda f32, hist (levels + 1, N_s, 3) numpy, iter_cnt) like
    the reference, plus ``info`` per level {steps, evaluated, last_loss}.  ``NDP`` may be
    the reference's Deformation_Pyramid (any motion and rotation format; its layers
    say which) or this module's mirror; by default a fresh mirror is built from the
    config (``motion_type``, ``rotation_format``), as the reference does.

    ``landmarks = (src_ldmk (L, 3), tgt_ldmk (L, 3))``, coordinates in the frames of
    ``src_pcd`` / ``tgt_pcd`` (L >= 1; ValueError otherwise), selects the landmark
    branch of the reference (Registration.load_pcds(..., landmarks=...),
    config/LNDP.yaml): mode "A" when ``config.w_cd > 0`` (landmark term +
    w_cd * Chamfer of all samples truncated at ``config.trunc_cd``; ``inds`` is not
    used), mode "B" otherwise (the landmark term alone: only the landmarks are
    warped during the optimisation).  ``info[level]["mode"]`` says which (None without
    landmarks) and ``info[level]["ldmk"]`` holds the level's warped landmarks +
    tgt_mean, (L, 3); ``info[level]["chamfer"]`` is "none" in mode B (no Chamfer pass).  ``hist``: mode A as without landmarks; in mode B the
    reference raises NameError where it records the level (registration.py:264:
    ``s_sample_warped`` is never bound), so there is nothing to match and ``hist`` is
    (1, N, 3), the final warp only."""
    cfg = NDPConfig.from_any(config or {})
    if landmarks is not None:
        landmarks = _check_landmarks(landmarks)
    if cfg.motion_type not in MOTIONS:
        raise ValueError(f"motion_type {cfg.motion_type!r} not in {MOTIONS}")
    if cfg.rotation_format not in ROTATION_FORMATS:
        raise ValueError(f"rotation_format {cfg.rotation_format!r} not in {ROTATION_FORMATS}")
    dev = torch.device("cuda", torch.cuda.current_device())
    src = torch.as_tensor(src_pcd, dtype=torch.float32).to(dev)
    tgt = torch.as_tensor(tgt_pcd, dtype=torch.float32).to(dev)
    if NDP is None:
        NDP = DeformationPyramid(cfg.depth, cfg.width, dev, cfg.k0, cfg.m, cfg.w_reg > 0,
                                 cfg.rotation_format, cfg.motion_type)
    src_mean = src.mean(dim=0, keepdim=True)
    tgt_mean = tgt.mean(dim=0, keepdim=True)
    src_c = (src - src_mean).contiguous()
    s_sample = src_c.clone()
    t_sample = (tgt - tgt_mean).contiguous()
    mode, n_ldmk = None, 0
    if landmarks is None:
        ind = torch.as_tensor(np.asarray(inds), dtype=torch.long, device=dev)
    else:
        # registration.py:186-187: centred by the means of the whole clouds
        src_ldmk = (landmarks[0].to(dev) - src_mean).contiguous()
        tgt_ldmk = (landmarks[1].to(dev) - tgt_mean).contiguous()
        mode, n_ldmk, ind = "A" if cfg.w_cd > 0 else "B", src_ldmk.shape[0], None
    hist, info = [], []
    shared = {}  # per-pyramid buffers of the levels (_Level)
    for level in range(NDP.n_hierarchy):
        NDP.gradient_setup(optimized_level=level)
        layer = NDP.pyramid[level]
        use_fused = fused and layer.input[0].weight.shape[0] == 128
        t0 = time.perf_counter()
        if mode is None:
            lv = (_LevelFused if use_fused else _Level)(layer, s_sample, t_sample, ind, level, cfg, shared)
        else:
            # the level's input, landmarks first (registration.py:214): one allocation
            # per level, outside the capture
            x_in = torch.cat([src_ldmk, s_sample]) if mode == "A" else src_ldmk
            lv = (_LevelFused if use_fused else _Level)(layer, x_in, t_sample, ind, level, cfg, shared,
                                                        ldmk=(n_ldmk, tgt_ldmk, mode))
        t1 = time.perf_counter()
        lv.run(use_graph)
        st = lv.state.cpu().numpy()
        t2 = time.perf_counter()
        info.append({"steps": int(st[3]), "evaluated": int(st[6]), "last_loss": float(st[4]),
                     "losses": lv.log[:int(st[6])].cpu().numpy(),
                     # which path ran: the fused HIP MLP kernels (width 128) or torch
                     # autograd, and the fused level Chamfer or the nnd drop-in kernels
                     "mlp": "fused" if use_fused else "torch",
                     "chamfer": "none" if mode == "B" else "fused" if getattr(lv, "use_nc", False) else "nnd",
                     "mode": mode})
        ev = getattr(lv, "replay_events", None)
        if ev is not None:
            info[-1]["replay_ms"] = ev[0].elapsed_time(ev[1])
            info[-1]["capture_ms"] = (lv.capture_done - t1) * 1e3
        if getattr(lv, "use_nc", False):
            # listed (uncertified) queries per direction of the last evaluated iteration
            hdr = lv.nc_raw[(lv.nc.scratch - lv.nc_raw.data_ptr()):][:88].cpu().numpy()
            h32 = hdr[:28].view(np.int32)
            info[-1]["fb_cnt"] = (int(h32[5]), int(h32[6]))
            if os.environ.get("PCR_NC_STATS", "0") != "0":
                # box path: queries, groups and leaves scanned over the level
                info[-1]["nc_stats"] = [int(v) for v in hdr[64:88].view(np.uint64)]
        info[-1]["setup_ms"] = (t1 - t0) * 1e3
        info[-1]["level_ms"] = (t2 - t0) * 1e3
        if mode is None:
            hist.append((lv.warped + tgt_mean).cpu().numpy())
            s_sample = lv.warped.clone()
        else:
            # registration.py:266-270: the warped landmarks feed the next level in both
            # modes, the warped samples in mode A only
            src_ldmk = lv.warped[:n_ldmk].clone()
            info[-1]["ldmk"] = (src_ldmk + tgt_mean).cpu().numpy()
            if mode == "A":
                s_sample = lv.warped[n_ldmk:].clone()
                hist.append((s_sample + tgt_mean).cpu().numpy())
    NDP.gradient_setup(optimized_level=-1)
    warped, _ = warp_pyramid(NDP, src_c)
    warped = warped + tgt_mean
    hist.append(warped.cpu().numpy())
    return warped, np.array(hist), {}, info


__all__ = ["NDPConfig", "NDPLayer", "DeformationPyramid", "optimize_deformation_pyramid"]
