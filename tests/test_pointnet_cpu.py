"""CPU: the staged f64 restatement of the pcr_pointnet_forward contract
(tests/pointnet_ref.py) agrees, within its own derived bounds, with what the
reference's PointNetFeature returned at every stage boundary with its trained
checkpoint (tests/golden/pointnet_golden.npz).  That is what lets the GPU tests
stand on the restatement.  Also: the bounds have teeth, the fold is the eval-mode
BatchNorm, bad nets and tensors are refused, and the entry points are declared,
exported and bound and refuse bad arguments before any device work.

Teeth, measured: removing a channel's argmax point from the unit-ball patches
moves mx by more than 10 bounds on 94 to 98 % of the live channels.  (Fed with
the checkpoint's xtrans instead, the figure is 47 to 75 % for unit-ball patches
and 91 to 93 % at 2.5 times the scale: this T-net shrinks a unit-ball patch to a
few hundredths, where most live conv2 channels hardly depend on the point; that
is the network, not the bound.)
"""
import ctypes
import os
import re
import shlex
import subprocess

import numpy as np
import pytest
import torch

import pointnet_cases as pc
import pointnet_ref as pr
from pointcloudregistration_amd import _lib, dip, pointnet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH = os.path.join(ROOT, "tests", "golden", "pointnet_golden.npz")
G = np.load(PATH)
STAGES = ("x", "stn_mx", "stn_hid", "trans", "xtrans", "mx", "amx", "fc1", "fc2", "f")
SD = {k[3:]: G[k] for k in G.files if k.startswith("sd/")}
NET = pr.net_from_arrays(SD)
FOLDED = pr.folded_layers(NET)


def _patch(name):
    return {k: G[f"{name}/{k}"] for k in STAGES}


def test_fixture_keys_and_size():
    want = {f"sd/{k}" for k in NET.state_dict()} | {f"{n}/{k}" for n in pc.GOLDEN_PATCHES for k in STAGES}
    assert set(G.files) == want
    assert os.path.getsize(PATH) < 1000 * 1000
    made = pc.golden_patches()
    for n in pc.GOLDEN_PATCHES:
        g = _patch(n)
        assert np.array_equal(g["x"], made[n]) and g["x"].dtype == np.float32
        p = g["x"].shape[1]
        assert g["xtrans"].shape == (3, p) and g["trans"].shape == (9,) and g["f"].shape == (32,)
        assert g["mx"].shape == g["amx"].shape == g["stn_mx"].shape == (256,) and g["amx"].dtype == np.int64
        assert g["fc1"].shape == g["stn_hid"].shape == (128,) and g["fc2"].shape == (32,)
    assert sorted(made[n].shape[1] for n in pc.GOLDEN_PATCHES) == [1, 5, 64, 65, 256, 256, 256, 300]
    assert not made["pad150"][:, 150:].any() and made["pad150"][:, :150].all()
    # the checkpoint's extremes that the fold must not special-case
    var = np.concatenate([v for k, v in SD.items() if k.endswith("running_var")])
    assert 0 < var.min() < 1e-44 and var.max() > 500


@pytest.mark.parametrize("name", pc.GOLDEN_PATCHES)
def test_restatement_agrees_with_reference(name):
    g = _patch(name)
    ratios = pr.stage_ratios(FOLDED, g)
    print(name, {k: round(v, 4) for k, v in ratios.items()})
    assert set(ratios) == {"stn_point", "stn_fc1", "trans", "xtrans", "point", "fc1", "fc2", "norm"}
    assert max(ratios.values()) <= 1.0, ratios
    # argmax: equal wherever the bounds decide it, and they decide at least half of the channels
    ps = pr.point_stage(*FOLDED["main"][:2], g["xtrans"])
    dead, clear = pr.decidable(ps)
    assert (g["amx"][dead] == 0).all() and (g["mx"][dead] == 0).all()
    assert np.array_equal(g["amx"][clear], ps["amx"][clear])
    assert (dead | clear).mean() >= 0.5
    # everywhere: the reference's argmax attains the maximum within the bounds
    rows = np.arange(256)
    assert (ps["h2"][rows, g["amx"]] >= ps["mx"] - 2 * ps["e_mx"]).all()
    # the chained bound holds too (twice: two implementations), and is not vacuous on a unit vector
    f, e = pr.chain(FOLDED, g["x"])
    assert (np.abs(g["f"] - f) <= e).all() and e.max() < 0.01


@pytest.mark.parametrize("name", [n for n in pc.GOLDEN_PATCHES if n != "p1"])
def test_point_stage_bound_has_teeth(name):
    ps = pr.point_stage(*FOLDED["main"][:2], G[f"{name}/x"])
    live = ps["mx"] > 0
    rest = ps["h2"].copy()
    rest[np.arange(256), ps["amx"]] = -np.inf        # the patch without each channel's argmax point
    moved = ps["mx"] - rest.max(1) > 10 * ps["e_mx"]
    print(name, int(live.sum()), float(moved[live].mean()))
    assert live.sum() >= 100 and moved[live].mean() >= 0.9


def _best_cut(fn, layer_, h, live_out):
    """Zero one live input channel at a time: (the largest fraction of the live outputs that move by
    more than 10 bounds, the number of input channels that reach 90 %, the live input channels)."""
    y, e = fn(layer_, h)
    fracs = []
    for c in np.flatnonzero(np.asarray(h) > 0):
        cut = np.asarray(h, np.float64).copy()
        cut[c] = 0.0
        moved = np.abs(fn(layer_, cut)[0] - y) > 10 * e
        fracs.append(float((moved if live_out is None else moved[live_out]).mean()))
    fracs = np.array(fracs)
    return fracs.max(), int((fracs >= 0.9).sum()), len(fracs)


@pytest.mark.parametrize("name", pc.GOLDEN_PATCHES)
def test_head_bounds_have_teeth(name):
    """The channel is chosen from the live ones: with this checkpoint a unit-ball patch leaves 35 to
    67 live channels in mx, each a small part of a hidden unit's sum, and 2 or 3 of them alone move
    90 % of the 14 to 16 live hidden units by 10 bounds (57 of 147 on the patch scaled by 2.5); for
    fc2 every output moves for most live hidden units."""
    g = _patch(name)
    l3, l4 = FOLDED["main"][2:]
    live = pr.fc1(l3, g["mx"])[0] > 0
    best, good, n = _best_cut(pr.fc1, l3, g["mx"], live)
    print(name, "fc1: live outputs", int(live.sum()), "live inputs", n, "reach 90 %:", good, "best", best)
    assert 10 <= live.sum() <= 40 and best >= 0.9
    best, good, n = _best_cut(pr.fc2, l4, g["fc1"], None)
    print(name, "fc2: live inputs", n, "reach 90 %:", good, "best", best)
    assert best >= 0.9


def test_fold_is_eval_mode_batchnorm():
    # f32 torch, the checkpoint's six BatchNorm layers (running_var down to 5.6e-45): within the layer bound
    rng = np.random.default_rng(3)
    seen_tiny = False
    for mod in (NET.stn3d, NET):
        for name in ("conv1", "conv2", "fc1"):
            layer, bn = pointnet._parts(getattr(mod, name), name)
            seen_tiny |= float(bn.running_var.min()) < 1e-44
            w, b = pointnet.fold(layer, bn)
            assert w.dtype == b.dtype == torch.float32 and w.shape == (layer.weight.shape[0], layer.weight.shape[1])
            x = rng.random((w.shape[1], 7)).astype(np.float32)
            xt = torch.from_numpy(x.T.copy())                       # (7, in)
            with torch.no_grad():
                ref = (bn(layer(xt[:, :, None]))[:, :, 0] if layer.weight.dim() == 3 else bn(layer(xt))).numpy().T
            want, bound = pr.layer(w.numpy(), b.numpy(), x)
            assert np.isfinite(ref).all() and (np.abs(ref - want) <= bound).all(), name
    assert seen_tiny
    # f64 torch, random statistics (gamma of both signs, running_var 1e-44 .. 1e2): the fold's only error is
    # the one rounding of W' and b' to f32
    net = pc.random_net(33)
    x = rng.random((3, 5)).astype(np.float32)
    layer, bn = pointnet._parts(net.conv1, "conv1")
    assert (bn.weight < 0).any() and (bn.weight > 0).any() and float(bn.running_var.min()) < 1.1e-44
    w, b = pointnet.fold(layer, bn)
    with torch.no_grad():
        ref = net.double().conv1(torch.from_numpy(x.astype(np.float64))[None])[0].numpy()   # with the ReLU
    want = pr.relu(pr.layer(w.numpy(), b.numpy(), x)[0])
    slack = pr.U * (np.abs(w.numpy().astype(np.float64)) @ np.abs(x) + np.abs(b.numpy())[:, None]) + 1e-300
    assert (np.abs(ref - want) <= 1.01 * slack).all()
    # no BatchNorm: the layer itself
    w, b = pointnet.fold(NET.fc2[0])
    assert torch.equal(w, NET.fc2[0].weight) and torch.equal(b, NET.fc2[0].bias)


def test_prepare_and_describe_refuse():
    net = dip.PointNetFeature(32)       # training mode
    with pytest.raises(ValueError, match="eval-mode only"):
        pointnet.prepare(net)
    net.eval()
    net.stn3d.conv2[2].train()          # one BatchNorm left in training mode
    with pytest.raises(ValueError, match="stn3d.conv2.2"):
        pointnet.prepare(net)
    net.eval()
    net.conv1 = dip._block(torch.nn.Conv1d(3, 64, 1), 64).eval()
    with pytest.raises(ValueError, match=r"net.conv1 is 3 -> 64; only 3 -> 128"):
        pointnet.prepare(net)
    net = dip.PointNetFeature(32).eval()
    net.fc2 = torch.nn.Sequential(torch.nn.Linear(128, 257)).eval()
    with pytest.raises(ValueError, match="dim=257 outside 1..256"):
        pointnet.prepare(net)
    with pytest.raises(ValueError, match="not a PointNetFeature"):
        pointnet.prepare(torch.nn.Linear(3, 3).eval())
    with pytest.raises(ValueError, match="GPU"):
        pointnet.prepare(NET)           # a CPU net: no CPU path
    assert pointnet.prepare.__doc__ and "snapshot" in pointnet.__doc__.lower()

    as_t = [(torch.from_numpy(w), torch.from_numpy(b)) for w, b in FOLDED["main"]]
    prep = pointnet.PreparedPointNet(as_t, as_t, 32, False, True, "cpu")
    x = torch.zeros(2, 3, 8)
    with pytest.raises(ValueError, match="CUDA"):
        pointnet.describe(prep, x)
    with pytest.raises(ValueError, match="float32"):
        pointnet.describe(prep, x.double())
    with pytest.raises(ValueError, match=r"\(B, 3, P\)"):
        pointnet.describe(prep, torch.zeros(2, 8, 3))
    with pytest.raises(RuntimeError, match="forward-only"):
        pointnet.describe(prep, x.clone().requires_grad_(True))
    with torch.no_grad(), pytest.raises(ValueError, match="CUDA"):
        pointnet.describe(prep, x.clone().requires_grad_(True))
    with pytest.raises(TypeError):
        pointnet.describe(NET, x)


def test_entry_points_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "pcr_api.h")).read()
    lib = _lib.load()

    def arity(name, ret):
        m = re.search(r"\b%s\s+%s\s*\(([^;]*)\);" % (ret, name), hdr)
        assert m, name
        return len(m.group(1).split(","))

    s = "pcr_pointnet_forward"
    assert s in _lib.exported_symbols() and s in _lib.SIGNATURES and hasattr(lib, s)
    assert arity(s, "int") == 18 == len(_lib.SIGNATURES[s])
    s = "pcr_pointnet_scratch_bytes"
    assert s in _lib.exported_symbols() and hasattr(lib, s)
    assert arity(s, "int64_t") == 3 == len(getattr(lib, s).argtypes)
    assert ctypes.sizeof(_lib.PointNetWeights) == 16 * ctypes.sizeof(ctypes.c_void_p)
    assert re.search(r"pcr_pointnet_layers stn;.*\n\s*pcr_pointnet_layers main;", hdr)
    import pointcloudregistration_amd as pcr
    assert "pointnet" in pcr.__all__ and pcr.pointnet is pointnet
    for name in ("fold", "prepare", "describe", "FusedPointNetFeature", "fuse", "PreparedPointNet"):
        assert hasattr(pointnet, name) and name in pointnet.__all__
    src = open(os.path.join(ROOT, "pointcloudregistration_amd", "csrc", "Makefile")).read()
    assert " pointnet.hip" in src


def _err(lib):
    return lib.pcr_last_error().decode()


def test_argument_errors_without_gpu():
    lib = _lib.load()
    one = ctypes.c_void_p(256)   # non-null: never dereferenced, validation comes first
    full = _lib.PointNetLayers(*([256] * 8))

    def fwd(x=one, f=one, mx=one, b=1, p=8, dim=32, tnet=1, scratch=one, stn=full, main=full, w=True):
        ws = _lib.PointNetWeights(stn, main)
        return lib.pcr_pointnet_forward(x, 24, 8, 1, b, p, ctypes.byref(ws) if w else None, dim, tnet, 1, f, mx, None,
                                        None, None, None, scratch, None)

    for name in ("x", "f", "mx"):
        assert fwd(**{name: None}) == -1 and "null pointer (x, f and mx are required)" in _err(lib), name
    assert fwd(w=False) == -1 and "null weights" in _err(lib)
    assert fwd(scratch=None) == -1 and "null scratch" in _err(lib)
    hole = _lib.PointNetLayers(*([256] * 5 + [0] + [256] * 2))
    assert fwd(main=hole) == -1 and "main layers" in _err(lib)
    assert fwd(stn=hole) == -1 and "T-net's layers" in _err(lib)
    for kw, msg in ((dict(p=0), "P=0 outside 1..4096"), (dict(p=4097), "P=4097 outside 1..4096"),
                    (dict(dim=0), "dim=0 outside 1..256"), (dict(dim=257), "dim=257 outside 1..256"),
                    (dict(b=-1), "B=-1 outside"), (dict(b=(1 << 20) + 1), "B=1048577 outside")):
        assert fwd(**kw) == -1 and msg in _err(lib), kw
    # an empty batch: no launch, no pointer needed
    assert fwd(b=0, x=None, f=None, mx=None, scratch=None, w=False) == 0
    # scratch: none without a T-net, B (256 + 16) floats with one, rounded up to 256 bytes
    assert lib.pcr_pointnet_scratch_bytes(37, 32, 0) == 0
    assert lib.pcr_pointnet_scratch_bytes(37, 32, 1) == (37 * 272 * 4 + 255) // 256 * 256
    assert lib.pcr_pointnet_scratch_bytes(4096, 256, 1) == 4096 * 272 * 4
    assert lib.pcr_pointnet_scratch_bytes(0, 32, 1) == 0
    assert lib.pcr_pointnet_scratch_bytes(1, 0, 1) == -1 and "dim=0" in _err(lib)
    assert lib.pcr_pointnet_scratch_bytes(-1, 32, 1) == -1 and "B=-1" in _err(lib)


def test_kernels_compile_without_spills(tmp_path):
    """pointnet_points keeps 128 weights and 64 accumulators per lane in registers and relies on the
    compiler leaving conv1's weights in LDS and the pool's masks short-lived (pointnet.hip).  Compile
    the unit as the Makefile does, with the resource remarks on: both kernels must report no spilled
    VGPR or SGPR and no scratch, whatever the compiler version."""
    csrc = os.path.join(ROOT, "pointcloudregistration_amd", "csrc")
    plan = subprocess.run(["make", "-C", csrc, "-n", "-B", "build/pointnet.hip.o"], capture_output=True,
                          text=True, check=True).stdout
    cmd = [ln for ln in plan.splitlines() if "pointnet.hip" in ln and " -c " in ln]
    assert len(cmd) == 1, plan
    argv = shlex.split(cmd[0])
    argv[argv.index("-o") + 1] = str(tmp_path / "pointnet.o")
    run = subprocess.run(argv + ["-Rpass-analysis=kernel-resource-usage"], cwd=csrc, capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    remarks = run.stderr
    kernels = re.findall(r"Function Name: (\S+)", remarks)
    assert len(kernels) == 2 and any("pointnet_points" in k for k in kernels), kernels
    for field in ("SGPRs Spill", "VGPRs Spill", r"ScratchSize \[bytes/lane\]"):
        values = re.findall(field + r": (\d+)", remarks)
        assert len(values) == len(kernels) and set(values) == {"0"}, (field, values)
