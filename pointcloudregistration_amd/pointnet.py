"""DIP's descriptor network (dip/network.py:50-122) fused for inference.

Mirror of pcr_pointnet_forward (contract in include/pcr_api.h, f64 restatement
with the derived bounds in tests/pointnet_ref.py): per patch the T-net, the 3x3
transform, the two point-wise layers, the max-pool over points and both heads
run on libpcr; no (B, C, P) activation exists in global memory.

* ``fold(linear, bn)``     -- eval-mode BatchNorm folded into a layer, (W', b')
* ``prepare(net)``         -- the eight folded layers of a PointNetFeature on
                              its device: a ``PreparedPointNet``
* ``describe(prepared, patches, want=())`` -- f, mx, amx (and hid, trans,
                              xtrans on request) for (B, 3, P) patches
* ``FusedPointNetFeature`` / ``fuse(net)`` -- a module with the reference's
                              forward() return forms around the original net

f32, CUDA tensors only (no CPU path), forward only: an input that requires grad
under grad mode raises.  Eval mode only: Dropout is the identity and BatchNorm
an affine map there, which is what the fold rests on; a net with a submodule in
training mode is refused.

The folded weights are a SNAPSHOT of the net's parameters and BatchNorm
statistics, taken by prepare() (fuse() calls it): unlike kpconv.fuse and
attention.fuse nothing is shared.  After loading another state dict or moving
the net, call ``FusedPointNetFeature.refresh()`` (or prepare() again).
"""
from __future__ import annotations

import ctypes

import torch

from . import _front, _lib

__all__ = ["fold", "prepare", "describe", "PreparedPointNet", "FusedPointNetFeature", "fuse", "MAX_DIM",
           "MAX_POINTS", "MAX_PATCHES"]

MAX_DIM = 256          # pcr_api.h
MAX_POINTS = 4096
MAX_PATCHES = 1 << 20
_WIDTHS = {"conv1": (128, 3), "conv2": (256, 128), "fc1": (128, 256)}
_LAYERS = ("conv1", "conv2", "fc1", "fc2")
_PATCH_SIZES = (None, 3, None)


def fold(linear, bn=None):
    """(W', b') of ``bn(linear(x))`` in eval mode, as f32 CPU tensors (out, in) and (out,):
    s = gamma / sqrt(running_var + eps), W' = W s, b' = (b - running_mean) s + beta, computed
    in f64 and rounded once.  `linear` is a Linear or a kernel-size-1 Conv1d.  bn None: W, b."""
    w = linear.weight.detach().to("cpu", torch.float64)
    if w.dim() == 3:
        if w.shape[2] != 1:
            raise ValueError(f"Conv1d kernel size {w.shape[2]}: only point-wise (1) layers fold")
        w = w[:, :, 0]
    out = w.shape[0]
    b = linear.bias.detach().to("cpu", torch.float64) if linear.bias is not None else torch.zeros(out, dtype=torch.float64)
    if bn is not None:
        if bn.running_var is None or bn.running_mean is None:
            raise ValueError("BatchNorm without running statistics cannot be folded")
        if bn.running_var.shape[0] != out:
            raise ValueError(f"BatchNorm over {bn.running_var.shape[0]} channels after a layer of {out}")
        s = 1.0 / torch.sqrt(bn.running_var.detach().to("cpu", torch.float64) + bn.eps)
        beta = torch.zeros(out, dtype=torch.float64)
        if bn.affine:
            s = s * bn.weight.detach().to("cpu", torch.float64)
            beta = bn.bias.detach().to("cpu", torch.float64)
        w = w * s[:, None]
        b = (b - bn.running_mean.detach().to("cpu", torch.float64)) * s + beta
    return w.to(torch.float32).contiguous(), b.to(torch.float32).contiguous()


def _parts(block, name):
    """(layer, bn or None) of Sequential(layer, Dropout, BatchNorm1d, ReLU) or Sequential(layer)."""
    mods = list(block.children()) if isinstance(block, torch.nn.Sequential) else [block]
    if not mods or not isinstance(mods[0], (torch.nn.Linear, torch.nn.Conv1d)):
        raise ValueError(f"{name}: expected Sequential(Linear or Conv1d, ...), got {type(block).__name__}")
    bns = [m for m in mods[1:] if isinstance(m, torch.nn.BatchNorm1d)]
    rest = [m for m in mods[1:] if not isinstance(m, (torch.nn.BatchNorm1d, torch.nn.Dropout, torch.nn.ReLU))]
    if rest or len(bns) > 1:
        raise ValueError(f"{name}: only Dropout, one BatchNorm1d and ReLU may follow the layer")
    return mods[0], (bns[0] if bns else None)


def _branch(mod, who, last):
    """The four folded layers of one branch, checked: [(W', b')] * 4.  last: fc2's width, or None."""
    layers = []
    for name in _LAYERS:
        if not hasattr(mod, name):
            raise ValueError(f"{who} has no {name}")
        layer, bn = _parts(getattr(mod, name), f"{who}.{name}")
        w, b = fold(layer, bn)
        want = _WIDTHS.get(name)
        if want is not None and tuple(w.shape) != want:
            raise ValueError(f"{who}.{name} is {w.shape[1]} -> {w.shape[0]}; only {want[1]} -> {want[0]} is built "
                             "(widths 3/128/256/128)")
        if name == "fc2":
            if w.shape[1] != 128:
                raise ValueError(f"{who}.fc2 takes {w.shape[1]} inputs; only 128 is built")
            if last is not None and w.shape[0] != last:
                raise ValueError(f"{who}.fc2 has {w.shape[0]} outputs, expected {last}")
        layers.append((w, b))
    return layers


def _unwrap(net):
    while True:
        if isinstance(net, torch.nn.DataParallel):
            net = net.module
        elif isinstance(net, FusedPointNetFeature):
            net = net.net
        else:
            return net


class PreparedPointNet:
    """The eight folded layers on one device, row-major (out, in), with dim, tnet, l2norm:
    `stn` and `main` are lists of four (W', b') pairs.  A snapshot (see the module docstring)."""

    def __init__(self, stn, main, dim, tnet, l2norm, device):
        self.device = torch.device(device)
        self.dim, self.tnet, self.l2norm = int(dim), bool(tnet), bool(l2norm)
        self.stn = [(w.to(self.device), b.to(self.device)) for w, b in stn]
        self.main = [(w.to(self.device), b.to(self.device)) for w, b in main]
        self.device = self.main[0][0].device   # with its index ("cuda" -> "cuda:0")

    def _struct(self):
        """pcr_pointnet_weights over this object's tensors (which must outlive the call)."""
        def layers(ls):
            y = _lib.PointNetLayers()
            for i, (w, b) in enumerate(ls, 1):
                setattr(y, f"w{i}", w.data_ptr())
                setattr(y, f"b{i}", b.data_ptr())
            return y
        s = _lib.PointNetWeights()
        s.stn = layers(self.stn)
        s.main = layers(self.main)
        return s

    def tnet_as_main(self):
        """The T-net's four layers as the main branch of a tnet = 0, l2norm = 0, dim = 9
        network: step 1 of the contract's composition."""
        return PreparedPointNet(self.stn, self.stn, 9, False, False, self.device)

    def without_tnet(self):
        """The main branch alone: step 3 of the contract's composition."""
        return PreparedPointNet(self.stn, self.main, self.dim, False, self.l2norm, self.device)


def prepare(net, device=None):
    """Fold the eight layers of a PointNetFeature (this package's or the reference's: anything
    with stn3d, conv1, conv2, fc1, fc2, tnet, l2norm laid out as Sequential(layer, Dropout,
    BatchNorm1d, ReLU)) onto `device` (default: the net's).  Looks through DataParallel.  Raises
    on a submodule in training mode, on widths other than 3/128/256/128, on dim outside 1..256."""
    net = _unwrap(net)
    for name in ("stn3d", "tnet", "l2norm") + _LAYERS:
        if not hasattr(net, name):
            raise ValueError(f"{type(net).__name__} has no attribute {name}: not a PointNetFeature")
    training = [n or type(net).__name__ for n, m in net.named_modules() if m.training]
    if training:
        raise ValueError("the fused forward is eval-mode only (BatchNorm would use batch statistics, Dropout "
                         f"would drop): call net.eval() first; in training mode: {', '.join(training[:4])}")
    dim = _parts(net.fc2, "fc2")[0].weight.shape[0]
    if not 1 <= dim <= MAX_DIM:
        raise ValueError(f"dim={dim} outside 1..{MAX_DIM}")
    main = _branch(net, "net", dim)
    stn = _branch(net.stn3d, "net.stn3d", 9)
    if device is None:
        device = net.conv1[0].weight.device
    device = torch.device(device)
    if device.type != "cuda":
        raise ValueError(f"the net lives on {device}: libpcr is a GPU (gfx950) library; move the net to a CUDA "
                         "(ROCm/HIP) device first or pass device=")
    return PreparedPointNet(stn, main, dim, net.tnet, net.l2norm, device)


def _patches(patches, prepared=None):
    """Check (B, 3, P) f32 CUDA patches and return the tensor whose data_ptr and strides go to
    pcr_pointnet_forward: always the caller's own storage (a detached alias), whatever the
    strides -- a contiguous tensor, the transposed view of a (B, P, 3) one and a batch slice all
    go in without a copy."""
    x = _front.tensor(patches, "patches", "(B, 3, P)", _PATCH_SIZES, prepared.device if prepared is not None else None)
    if not 1 <= x.shape[2] <= MAX_POINTS:
        raise ValueError(f"P={x.shape[2]} outside 1..{MAX_POINTS}")
    if x.shape[0] > MAX_PATCHES:
        raise ValueError(f"B={x.shape[0]} above {MAX_PATCHES}")
    return x


def describe(prepared, patches, want=()):
    """f (B, dim), mx (B, 256), amx (B, 256) int64 for patches (B, 3, P) f32 on the prepared
    device, taken by stride (the transposed view of a (B, P, 3) tensor goes in without a copy).
    want: names among "hid" (B, 128), "trans" (B, 9; needs a T-net), "xtrans" (B, 3, P), appended
    to the result in the order given."""
    if not isinstance(prepared, PreparedPointNet):
        raise TypeError("prepared must be a PreparedPointNet (pointnet.prepare(net))")
    _front.forward_only("pointnet.describe", patches)
    x = _patches(patches, prepared)
    want = _front.wanted(want, ("hid", "trans", "xtrans"))
    if "trans" in want and not prepared.tnet:
        raise ValueError("trans requested from a network without a T-net")
    b, _, p = x.shape
    dev, dim = x.device, prepared.dim
    f = torch.empty((b, dim), dtype=torch.float32, device=dev)
    mx = torch.empty((b, 256), dtype=torch.float32, device=dev)
    amx = torch.empty((b, 256), dtype=torch.int32, device=dev)
    extra = {"hid": (b, 128), "trans": (b, 9), "xtrans": (b, 3, p)}
    outs = {n: torch.empty(extra[n], dtype=torch.float32, device=dev) for n in want}
    if b:
        lib = _lib.load()
        w = prepared._struct()
        with torch.cuda.device(dev):
            ws = _front.scratch(lib.pcr_pointnet_scratch_bytes(b, dim, int(prepared.tnet)), dev)
            _lib.call("pcr_pointnet_forward", _lib.ptr(x), x.stride(0), x.stride(1), x.stride(2), b, p,
                      ctypes.byref(w), dim, int(prepared.tnet), int(prepared.l2norm), _lib.ptr(f), _lib.ptr(mx),
                      _lib.ptr(amx), _lib.ptr(outs.get("hid")), _lib.ptr(outs.get("trans")),
                      _lib.ptr(outs.get("xtrans")), _lib.ptr(ws), _lib.stream_handle(dev))
    return (f, mx, amx.to(torch.int64)) + tuple(outs[n] for n in want)


class FusedPointNetFeature(torch.nn.Module):
    """A PointNetFeature (dip.PointNetFeature or the reference's class) run through describe().
    The original net is held as-is, so parameters, buffers and state-dict keys are unchanged
    (``state_dict()`` / ``load_state_dict()`` are the net's own); the folded weights are a
    snapshot taken at construction -- call refresh() after changing the net.  forward() has the
    reference's return forms (network.py:103-119).  It does no chunking of its own."""

    def __init__(self, net):
        super().__init__()
        self.net = _unwrap(net)
        self.prepared = None
        self.refresh()
        self.training = False   # prepare() has just checked that the net is in eval mode

    @property
    def tnet(self):
        return self.net.tnet

    @property
    def l2norm(self):
        return self.net.l2norm

    def refresh(self, device=None):
        """Fold the net's current parameters and statistics again (on its current device)."""
        self.prepared = prepare(self.net, device)
        return self

    def state_dict(self, *args, **kwargs):
        return self.net.state_dict(*args, **kwargs)

    def load_state_dict(self, state_dict, *args, **kwargs):
        out = self.net.load_state_dict(state_dict, *args, **kwargs)
        self.refresh()
        return out

    def _one(self, x, full):
        if full:
            f, mx, amx, trans, xtrans = describe(self.prepared, x, want=("trans", "xtrans"))
            return f, xtrans, trans.view(-1, 3, 3), mx.unsqueeze(2), amx.unsqueeze(2)
        f, mx, amx = describe(self.prepared, x)
        return f, mx.unsqueeze(2), amx.unsqueeze(2)

    def forward(self, xa, xp=None, trans=False):
        """xa (B, 3, P) -> (f, mx (B, 256, 1), amx (B, 256, 1)).  With a second batch xp: with a
        T-net (out1a, xtrans1, trans1, out2a, xtrans2, trans2), else two (f, mx, amx) tuples."""
        if self.training or self.net.training:
            raise RuntimeError("FusedPointNetFeature is inference-only (the folded weights are eval-mode "
                               "BatchNorm): call .eval(); train the wrapped net itself (.net), then refresh()")
        if xp is None or xp.nelement() == 0:
            return self._one(xa, False)
        if self.prepared.tnet:
            return self._one(xa, True)[:3] + self._one(xp, True)[:3]
        return self._one(xa, False), self._one(xp, False)


def fuse(net):
    """The fused module of a loaded, eval-mode PointNetFeature on a CUDA device; a
    FusedPointNetFeature is returned unchanged.  The weights are a snapshot (refresh())."""
    if isinstance(net, FusedPointNetFeature):
        return net
    return FusedPointNetFeature(net)
