"""What the fused modules' Python front ends share: the forward-only rule, the
tensor checker, the layout rules, the scratch buffer, the ``want=`` parser and
the walker behind every ``fuse(model)``.  Private; imports no sibling but _lib.

The checker tests type -> dtype -> shape -> CUDA -> device, so an input with
two defects reports the earlier one.  What goes in by stride and what is copied
is the caller's choice among the layout rules, which are pure functions of a
tensor (``unit_last``, ``rows``, ``Tensor.contiguous``, or none).  These run on
every call of a launch-bound op: keep them free of generators and closures.
"""
from __future__ import annotations

import torch

from . import _lib

_DTYPES = {"f32": (lambda d: d == torch.float32, "torch.float32"),
           "floating": (lambda d: d.is_floating_point, "a floating-point tensor"),   # cast to f32
           "index": (lambda d: d in (torch.int32, torch.int64), "torch.int32 or torch.int64")}


def forward_only(what, *tensors, message=None):
    """Raise where a tensor requires grad under grad mode; `message` replaces the usual text."""
    if torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in tensors):
        raise RuntimeError(message or f"{what} is forward-only (inference): call it under torch.no_grad() or pass "
                           "detached tensors; it would otherwise silently cut the graph")


def tensor(t, name, phrase, sizes, dev=None, dtype="f32", layout=None):
    """Check a CUDA torch.Tensor of `dtype` (a key of _DTYPES) and return it off the graph, on the
    caller's storage, through `layout` (one of the rules below) when one is given.  sizes: the
    rank, or a tuple with one entry per axis, the axis' size or None for any; None: any shape.
    dev: the device it must be on, when given.  `phrase`, e.g. "(B, C, N)", names the shape in
    the message; its {i} fields are filled from `sizes`.  A tensor that requires grad is
    detached; any other one is returned itself, which saves the call its largest cost."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if (t.dtype != torch.float32) if dtype == "f32" else not _DTYPES[dtype][0](t.dtype):
        raise ValueError(f"{name} must be {_DTYPES[dtype][1]}, got {t.dtype}")
    if sizes is not None:
        if type(sizes) is int:
            bad = t.dim() != sizes
        else:
            bad = t.dim() != len(sizes)
            for want, got in zip(sizes, t.shape):
                bad = bad or (want is not None and want != got)
        if bad:
            shape = phrase if type(sizes) is int else phrase.format(*sizes)
            raise ValueError(f"{name} must be {shape}, got {tuple(t.shape)}")
    if not t.is_cuda:
        raise ValueError(f"{name} must be a CUDA (ROCm/HIP) tensor: libpcr is a GPU (gfx950) "
                         "library and this module has no CPU path")
    if dev is not None and t.device != dev:
        raise ValueError(f"{name} on {t.device}, expected {dev}: all inputs must live on one device")
    if t.requires_grad:
        t = t.detach()
    if dtype == "floating":
        t = t.to(torch.float32)
    return t if layout is None else layout(t)


def param(t, name, shape, dev):
    """A contiguous f32 parameter of exactly `shape` on `dev`: one message for every defect."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if not t.is_cuda or t.dtype != torch.float32 or t.device != dev or tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name} must be a {tuple(shape)} torch.float32 tensor on {dev}, got "
                         f"{tuple(t.shape)} {t.dtype} on {t.device}")
    return t.detach().contiguous()


def unit_last(t):
    """`t` where its last axis has unit stride (or at most one entry), else a contiguous copy."""
    return t if t.shape[-1] <= 1 or t.stride(-1) == 1 else t.contiguous()


def rows(t):
    """A (rows, width) `t` where its rows have unit stride and do not overlap, else a copy."""
    return t if not t.shape[1] or (t.stride(1) == 1 and t.stride(0) >= t.shape[1]) else t.contiguous()


def scratch(nbytes, dev, at_least=0, who=""):
    """A uint8 buffer of max(nbytes, at_least) bytes on `dev`, None for none; nbytes < 0 is a
    *_scratch_bytes call that failed: PcrError with the library's text behind `who`."""
    if nbytes < 0:
        raise _lib.PcrError(who + _lib.load().pcr_last_error().decode("utf-8", "replace"))
    if nbytes < at_least:
        nbytes = at_least
    return torch.empty(nbytes, dtype=torch.uint8, device=dev) if nbytes else None


def wanted(want, stages, *, single=False):
    """`want` as a tuple of names among `stages`.  single: a bare string is one name, and the
    result is (tuple, whether it was a bare string)."""
    bare = single and isinstance(want, str)
    want = (want,) if bare else tuple(want)
    for name in want:
        if name not in stages:
            raise ValueError(f"want: unknown output {name!r} (one of {', '.join(stages)})")
    return (want, bare) if single else want


def has(mod, *names):
    return all(hasattr(mod, n) for n in names)


def swap_children(model, kinds, *, refused=None, waves=None, errors=(ValueError,), skip=()):
    """The walk behind fuse(): every child of every module of `model` that matches one of
    `kinds`, a sequence of (match, make), becomes make(child), in place and in its training
    mode.  match: (class name, attribute names) or a predicate on the child; a child takes the
    first kind it matches.  Instances of `skip` are passed over.  A make() that raises one of
    `errors` leaves the child where it is and appends (dotted name, reason) to `refused` when
    that is a list.  waves: tuples of indices into kinds, one full walk each, so that a block
    built in a later wave holds the replacements of an earlier one.  Returns the counts per kind."""
    counts = [0] * len(kinds)
    for wave in waves or (range(len(kinds)),):
        for pname, parent in list(model.named_modules()):
            for name, child in list(parent.named_children()):
                if isinstance(child, skip):
                    continue
                for i in wave:
                    match, make = kinds[i]
                    if not (match(child) if callable(match) else
                            type(child).__name__ == match[0] and has(child, *match[1])):
                        continue
                    try:
                        new = make(child)
                    except errors as e:
                        if refused is not None:
                            refused.append((f"{pname}.{name}" if pname else name, str(e)))
                        break
                    new.train(child.training)
                    setattr(parent, name, new)
                    counts[i] += 1
                    break
    return tuple(counts)
