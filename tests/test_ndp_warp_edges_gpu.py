"""GPU: pcr_ndp_warp at its edge shapes -- a single partial 32-point workgroup,
every width at depths 1, 2 and 5, the 16-level cap, the optional outputs, the
nonrigidity branch on level 0, an all-zero rotation branch -- against the f64
oracle (oracle.ndp_warp, pinned to the reference's own output by
test_oracle_ndp.py).  The bars are 4 x the f32 floor of the mirror pyramid on
the same cases (tests/golden/ndp_loop_bounds.npz, recorded by
make_ndp_loop_bounds.py and held below the 1e-5 / 1e-6 of test_ndp_gpu.py by
tests/test_ndp_loop_ref_cpu.py); everything else is bit equality."""
import ctypes
import os

import numpy as np
import pytest
import torch

import ndp_loop_ref as ref
from pointcloudregistration_amd import _lib, ndp

pytestmark = pytest.mark.gpu
BOUNDS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ndp_loop_bounds.npz")
BY = {c["name"]: c for c in ref.WARP_CASES}


def _run(levels, x, **kw):
    """PreparedPyramid.warp -> (y, per level (points, nonrigidity or None)) as numpy."""
    pp = ndp.PreparedPyramid(levels)
    y, data = pp.warp(x, **kw)
    torch.cuda.synchronize()
    out = [(data[i][0].cpu().numpy(), None if data[i][1] is None else data[i][1].cpu().numpy())
           for i in sorted(data)]
    return y.cpu().numpy(), out


def _bits(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("c", ref.WARP_CASES, ids=lambda c: c["name"])
def test_warp_case_vs_oracle(oracle, c):
    bar_xyz, bar_s = ref.warp_bars(BOUNDS)
    levels, x = ref.make_warp_case(c)
    y, got = _run(levels, x)
    with np.errstate(invalid="ignore"):
        ry, rdata = oracle.ndp_warp(levels, x)
    want = [rdata[i] for i in range(len(levels))]
    assert len(got) == len(want) and _bits(y, got[-1][0])          # y is the last level's points
    if c["zero_rot"] is None:
        assert np.isfinite(ry).all() and np.abs(ry - x).max() > 1e-3   # the warp is not the identity
    else:   # 0 / 0 from level zero_rot on, the nonrigidity of that level still finite
        assert np.isnan(want[c["zero_rot"]][0]).all() and np.isfinite(want[c["zero_rot"]][1]).all()
        assert np.isfinite(want[c["zero_rot"] - 1][0]).all()
    ex, es = ref.warp_errors(got, want)    # asserts the non-finite positions are the oracle's
    print(f"warp {c['name']}: points {ex:.2e} = {ex / bar_xyz:.3f} of the bar, "
          f"nonrigidity {es:.2e} = {es / bar_s:.3f} of the bar")
    assert ex <= bar_xyz and es <= bar_s, (ex, bar_xyz, es, bar_s)


def test_warp_position_independence():
    """A point's bits do not depend on where it sits in the cloud or on its
    neighbours in the workgroup (csrc/ndp.hip's header)."""
    levels, x = ref.make_warp_case(BY["n65-w128-d2"])
    _, full = _run(levels, x)
    _, head = _run(levels, x[:33])
    for i in (0, 31, 32, 64):
        _, alone = _run(levels, x[i:i + 1])
        for k in range(len(levels)):
            assert _bits(alone[k][0][0], full[k][0][i]), (i, k)
            assert (full[k][1] is None) == (alone[k][1] is None)
            if full[k][1] is not None:
                assert _bits(alone[k][1][:1], full[k][1][i:i + 1]), (i, k)
            if i < 33:
                assert _bits(head[k][0][i], full[k][0][i]), (i, k)
                if full[k][1] is not None:
                    assert _bits(head[k][1][i:i + 1], full[k][1][i:i + 1]), (i, k)


@pytest.mark.parametrize("name", ["n33-w32-d1", "n65-w96-d5", "nr-first"])
def test_warp_optional_outputs_and_level_range(name):
    levels, x = ref.make_warp_case(BY[name])
    pp = ndp.PreparedPyramid(levels)
    y, data = pp.warp(x)
    y2, data2 = pp.warp(x)
    y0, none = pp.warp(x, per_level=False)       # null x_levels / nonrigidity
    assert none == {} and torch.equal(y0, y) and torch.equal(y2, y)
    for k in data:
        assert torch.equal(data[k][0], data2[k][0])
        assert (data[k][1] is None) == ("nr_branch.weight" not in levels[k])
        if data[k][1] is not None:
            assert torch.equal(data[k][1], data2[k][1]) and not torch.isnan(data[k][1]).any()
        # min_level = max_level = k is level k applied to its own input
        xin = torch.from_numpy(x).cuda() if k == 0 else data[k - 1][0]
        yk, dk = pp.warp(xin, max_level=k, min_level=k)
        assert list(dk) == [k] and torch.equal(yk, data[k][0]) and torch.equal(dk[k][0], data[k][0])
        if data[k][1] is not None:
            assert torch.equal(dk[k][1], data[k][1])


def _raw(pp, structs, x, out, width):
    arr = (ndp._Level * max(len(structs), 1))(*structs)
    return _lib.load().pcr_ndp_warp(_lib.ptr(x), x.shape[0], ctypes.cast(arr, ctypes.c_void_p), len(structs),
                                    width, int(pp.depth), int(pp.k0), _lib.ptr(out), None, None,
                                    _lib.stream_handle())


def test_warp_argument_edges():
    levels, x = ref.make_warp_case(BY["n33-w128-d2"])
    pp = ndp.PreparedPyramid(levels)
    xt = torch.from_numpy(x).cuda()
    # zero levels: x unchanged; N = 0: an empty tensor
    y, data = pp.warp(xt, max_level=-1)
    assert data == {} and torch.equal(y, xt)
    y, data = pp.warp(np.zeros((0, 3), np.float32))
    assert y.shape == (0, 3) and all(d[0].shape == (0, 3) for d in data.values())
    # 17 levels and width 48 are refused before anything is written
    for structs, width in ((pp.structs * 6)[:17], 128), (pp.structs, 48):
        out = torch.full_like(xt, -7.0)
        assert _raw(pp, structs, xt, out, width) == -1     # PCR_ERR_ARG
        torch.cuda.synchronize()
        assert (out == -7.0).all()
    assert _raw(pp, (pp.structs * 6)[:16], xt, torch.full_like(xt, -7.0), 128) == 0   # the cap itself runs
    torch.cuda.synchronize()
    with pytest.raises(_lib.PcrError):
        ndp.PreparedPyramid(levels * 6).warp(xt, max_level=16)
    f = np.float32
    sd48 = {"input.0.weight": np.ones((48, 6), f), "input.0.bias": np.ones(48, f),
            "rot_brach.weight": np.ones((3, 48), f), "rot_brach.bias": np.ones(3, f),
            "trn_branch.weight": np.ones((3, 48), f), "trn_branch.bias": np.ones(3, f)}
    with pytest.raises(_lib.PcrError):
        ndp.PreparedPyramid([sd48]).warp(xt)
