"""f2 (csrc/voxel.hip, csrc/voxel_runs.hip, geometry.py) on the inputs of
tests/voxel_cases.py against the oracle's restatement of PointCloud::VoxelDownSample
(oracle/voxel_oracle.cpp): the bytes of points, normals and colors, row order and
per-cloud lengths included.  The contract is the same f64 operations in the same
order, so there is no tolerance anywhere in this file.  Batched calls are compared
with the oracle run cloud by cloud; an empty cloud gives (0, 3) outputs, and None for
the extras that were not passed.  test_voxel_cases_cpu.py proves that each input
still reaches the path it is here for.

The rejections checked here (65-bit keys, bad arguments) happen on the host: the
argument checks before anything is launched, the key-width check after the bounding
box reduction and before the key, sort and emit kernels."""
import ctypes

import numpy as np
import pytest
import torch

import voxel_cases as vc
from pointcloudregistration_amd import _lib, geometry, registration as reg

pytestmark = pytest.mark.gpu

TOO_FINE = r"65-bit voxel keys \(the grid is too fine for one 64-bit sort key\)"


def _bytes(t):
    return (t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)).tobytes()


def _run(case, voxel=None):
    return geometry.voxel_down_sample_batch(case.clouds, case.voxel if voxel is None else voxel,
                                            case.normals, case.colors)


def _assert_same(outs, refs):
    """outs: per cloud (points, normals, colors) from the library; refs: the same from
    the oracle (or from another library call).  Shapes, None-ness and bytes."""
    assert len(outs) == len(refs)
    for b, (got3, ref3) in enumerate(zip(outs, refs)):
        for got, ref, what in zip(got3, ref3, ("points", "normals", "colors")):
            if ref is None:
                assert got is None, (b, what)
                continue
            assert got is not None and tuple(got.shape) == tuple(ref.shape), (b, what)
            assert _bytes(got) == _bytes(ref), (b, what)


def _single(pts, voxel, normals=None, colors=None):
    """One cloud through the Open3D-shaped method: (points, normals, colors) numpy."""
    pcd = reg.PointCloud(pts)
    pcd.normals, pcd.colors = normals, colors
    out = pcd.voxel_down_sample(voxel)
    return np.asarray(out.points), out.normals, out.colors


# ---- cell boundaries ------------------------------------------------------------

@pytest.mark.parametrize("name", vc.LATTICE_NAMES)
def test_lattice_single(oracle, name):
    case = vc.get(name)
    _assert_same([_single(case.clouds[0], case.voxel)], vc.oracle_case(oracle, name))


@pytest.mark.parametrize("voxel", vc.LATTICE_VOXELS)
def test_lattice_all_18_in_one_batch(oracle, voxel):
    """All 18 lattice clouds in one call (nb = 18: 5 cloud bits, not a power of two)
    at each of the six voxel sizes: three of the clouds sit on that size's faces."""
    clouds = [vc.get(n).clouds[0] for n in vc.LATTICE_NAMES]
    assert len(clouds) == 18
    outs = geometry.voxel_down_sample_batch(clouds, voxel)
    _assert_same(outs, [vc.oracle_case(oracle, n, voxel)[0] for n in vc.LATTICE_NAMES])


# ---- wide and unequal key fields ------------------------------------------------

@pytest.mark.parametrize("bits", vc.WIDE_SINGLE)
def test_wide_keys_single(oracle, bits):
    case = vc.get(vc.wide_name(bits))
    _assert_same([_single(case.clouds[0], case.voxel)], vc.oracle_case(oracle, vc.wide_name(bits)))
    _assert_same(_run(case), vc.oracle_case(oracle, vc.wide_name(bits)))


def test_wide_keys_63_bits_and_a_cloud_bit(oracle):
    name = vc.wide_name(vc.WIDE_BATCH)
    assert len(vc.get(name).clouds) == 2
    _assert_same(_run(vc.get(name)), vc.oracle_case(oracle, name))


def test_wide_keys_65_bits_are_rejected(oracle):
    """The one deliberate difference from the reference: a grid too fine for one
    64-bit sort key is an error here, while the oracle alone handles it."""
    name = vc.wide_name(vc.WIDE_TOO_FINE)
    case = vc.get(name)
    assert len(vc.oracle_case(oracle, name)[0][0]) > 0
    with pytest.raises(_lib.PcrError, match=TOO_FINE):
        _run(case)
    with pytest.raises(_lib.PcrError, match=TOO_FINE):
        _single(case.clouds[0], case.voxel)
    # 64 bits alone, 65 with the cloud bit of a 2-cloud batch
    full = vc.get(vc.wide_name(vc.WIDE_SINGLE[0])).clouds[0]
    other = vc.get(vc.wide_name(vc.WIDE_BATCH)).clouds[0]
    for clouds in ([full, other], [other, full]):
        with pytest.raises(_lib.PcrError, match=TOO_FINE):
            geometry.voxel_down_sample_batch(clouds, vc.WIDE_VOXEL)
    # and the library is as usable as before
    _assert_same([_single(other, vc.WIDE_VOXEL)], vc.oracle_case(oracle, vc.wide_name(vc.WIDE_BATCH))[:1])


# ---- the threaded host replay ---------------------------------------------------

def test_threaded_replay_every_cloud(oracle):
    outs = _run(vc.get("threaded"))
    refs = vc.oracle_case(oracle, "threaded")
    assert sum(len(p) for p, _, _ in outs) >= 65536
    _assert_same(outs, refs)


# ---- batch layouts with normals, NaN normals and colors --------------------------

@pytest.mark.parametrize("name", vc.LAYOUT_NAMES)
def test_layouts_with_normals_and_colors(oracle, name):
    case = vc.get(name)
    outs = _run(case)
    _assert_same(outs, vc.oracle_case(oracle, name))
    # the same clouds one by one (an empty cloud has no extras to pass)
    for b, pts in enumerate(case.clouds):
        p, n, c = _single(pts, case.voxel, case.normals[b], case.colors[b])
        if len(pts):
            _assert_same([(p, n, c)], [outs[b]])
        else:
            assert p.shape == (0, 3) and n is None and c is None
    # extras are optional one at a time
    for nr, cl in ((case.normals, None), (None, case.colors)):
        part = geometry.voxel_down_sample_batch(case.clouds, case.voxel, nr, cl)
        _assert_same(part, [(p, n if nr else None, c if cl else None) for p, n, c in outs])


# ---- long runs -------------------------------------------------------------------

def test_long_run(oracle):
    case = vc.get("long_run")
    _assert_same([_single(case.clouds[0], case.voxel)], vc.oracle_case(oracle, "long_run"))


# ---- workspace reuse and streams ---------------------------------------------------

def test_workspace_reuse_large_small_large(oracle):
    big, lat = vc.get("threaded"), vc.get(vc.lattice_name(0.1, -7.3))
    one = np.array([[0.25, -1.5, 3.0]])
    first = _run(big)
    tiny = _single(one, 0.5)
    mid = _single(lat.clouds[0], lat.voxel)
    last = _run(big)
    _assert_same(last, first)
    _assert_same(first, vc.oracle_case(oracle, "threaded"))
    assert _bytes(tiny[0]) == one.tobytes()
    _assert_same([mid], vc.oracle_case(oracle, vc.lattice_name(0.1, -7.3)))


def test_non_default_stream(oracle):
    name = vc.layout_name((300, 0, 0, 300))
    case = vc.get(name)
    want = _run(case)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        got = _run(case)
    s.synchronize()
    torch.cuda.synchronize()
    _assert_same(got, want)
    _assert_same(got, vc.oracle_case(oracle, name))


# ---- the wrapper's input handling --------------------------------------------------

def test_input_types_and_views(oracle):
    rng = np.random.default_rng(21)
    p32 = (rng.random((2500, 3)) * 4.0).astype(np.float32)
    p64 = p32.astype(np.float64)
    nrm, col = rng.standard_normal((2500, 3)), rng.random((2500, 3))
    want = geometry.voxel_down_sample_batch([p64], 0.3, [nrm], [col])
    _assert_same(want, [oracle.voxel_down_sample(p64, 0.3, nrm, col)])
    wide = np.zeros((2500, 7))
    wide[:, 1:4] = p64
    twice = np.repeat(p64, 2, axis=0)
    dev = torch.from_numpy(p64).cuda()
    dev_wide = torch.from_numpy(wide).cuda()
    variants = {"f32 numpy": p32, "f64 device": dev, "f32 device": torch.from_numpy(p32).cuda(),
                "numpy column view": wide[:, 1:4], "numpy row view": twice[::2],
                "device column view": dev_wide[:, 1:4], "list of rows": p64.tolist()}
    assert not wide[:, 1:4].flags.c_contiguous and not twice[::2].flags.c_contiguous
    assert not dev_wide[:, 1:4].is_contiguous()
    for what, pts in variants.items():
        got = geometry.voxel_down_sample_batch([pts], 0.3, [nrm], [col])
        for a, b in zip(got[0], want[0]):
            assert tuple(a.shape) == tuple(b.shape) and _bytes(a) == _bytes(b), what


def test_extras_need_one_row_per_point():
    rng = np.random.default_rng(22)
    a, b = rng.random((50, 3)), rng.random((30, 3))
    with pytest.raises(ValueError, match="normals must have one row per point"):
        geometry.voxel_down_sample_batch([a, b], 0.2, normals=[a, b[:-1]])
    with pytest.raises(ValueError, match="colors must have one row per point"):
        geometry.voxel_down_sample_batch([a, b], 0.2, normals=[a, b], colors=[a])
    with pytest.raises(ValueError, match="colors must have one row per point"):
        geometry.voxel_down_sample_batch([a], 0.2, colors=[np.concatenate([a, b])])


# ---- the C entry's own rules ---------------------------------------------------------

SENTINEL = -12345.0


def _entry(points, n, lens, voxel, cap, null_points=False, null_out_len=False):
    """pcr_voxel_down_sample as the wrapper calls it, but with n, cloud_len and the
    output pointers chosen freely.  Outputs are pre-filled (points with SENTINEL, the
    counts with 77) so that what the entry did not write shows."""
    dev = torch.device("cuda", torch.cuda.current_device())
    P = None if null_points else torch.from_numpy(np.ascontiguousarray(points, np.float64)).to(dev)
    op = None if null_points else torch.full((cap, 3), SENTINEL, dtype=torch.float64, device=dev)
    lens = np.asarray(lens, np.int32)
    out_len = np.full(len(lens), 77, np.int32)
    total = np.full(1, 77, np.int32)
    _lib.call("pcr_voxel_down_sample", _lib.ptr(P), n, lens.ctypes.data_as(_lib._p), len(lens), float(voxel),
              _lib.ptr(None), _lib.ptr(None), _lib.ptr(op), _lib.ptr(None), _lib.ptr(None),
              ctypes.c_void_p(0) if null_out_len else out_len.ctypes.data_as(_lib._p),
              total.ctypes.data_as(_lib._p), _lib.stream_handle(dev))
    torch.cuda.synchronize()
    return (None if op is None else op.cpu().numpy()), out_len, int(total[0])


def test_entry_ignores_rows_past_the_clouds(oracle):
    rng = np.random.default_rng(23)
    pts = rng.random((900, 3)) * 3.0
    pts[500:] = np.inf          # read, these would be the non-finite error
    refs = [oracle.voxel_down_sample(pts[:300], 0.4)[0], oracle.voxel_down_sample(pts[300:500], 0.4)[0]]
    op, out_len, total = _entry(pts, 900, (300, 200), 0.4, cap=900)
    assert list(out_len) == [len(r) for r in refs] and total == sum(out_len)
    assert op[:total].tobytes() == np.concatenate(refs).tobytes()
    assert (op[total:] == SENTINEL).all()


def test_entry_without_points():
    op, out_len, total = _entry(None, 0, (0,), 0.4, cap=0, null_points=True)
    assert list(out_len) == [0] and total == 0
    op, out_len, total = _entry(None, 0, (0, 0, 0), 0.4, cap=0, null_points=True)
    assert list(out_len) == [0, 0, 0] and total == 0
    # points given, every cloud empty: nothing is read or written
    op, out_len, total = _entry(np.full((5, 3), np.inf), 5, (0, 0, 0), 0.4, cap=5)
    assert list(out_len) == [0, 0, 0] and total == 0 and (op == SENTINEL).all()


def test_entry_rejects_bad_arguments():
    pts = np.random.default_rng(24).random((10, 3))
    with pytest.raises(_lib.PcrError, match="negative cloud length"):
        _entry(pts, 10, (5, -1), 0.4, cap=10)
    with pytest.raises(_lib.PcrError, match="bad arguments"):
        _entry(pts, 10, (5, 5), 0.4, cap=10, null_out_len=True)
    with pytest.raises(_lib.PcrError, match="bad arguments"):
        _entry(pts, -1, (5, 5), 0.4, cap=10)
    with pytest.raises(_lib.PcrError, match="null points"):
        _entry(None, 10, (5, 5), 0.4, cap=10, null_points=True)
    with pytest.raises(_lib.PcrError, match=r"clouds sum to 11 > 10 points"):
        _entry(pts, 10, (5, 6), 0.4, cap=10)


def test_entry_single_point(oracle):
    one = np.array([[1.75, -2.5, 1e6 + 0.125]])
    op, out_len, total = _entry(one, 1, (1,), 0.4, cap=3)
    assert list(out_len) == [1] and total == 1
    assert op[:1].tobytes() == one.tobytes() == oracle.voxel_down_sample(one, 0.4)[0].tobytes()
    assert (op[1:] == SENTINEL).all()
