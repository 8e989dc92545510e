"""GPU: the k-NN graph and edge features of NgeNet's GCN
(pointcloudregistration_amd.grouping.knn_graph / graph_features) against the
numpy restatement that tests/test_knn_graph_cpu.py pins to the reference's
get_graph_features, and against the reference's stored outputs themselves.

Bars.  Everything is bit-equal: indices, distances and features have no
tolerance (distances are the direct form without FMA, ties go to the lowest
index, the features are copies and one f32 subtraction).  Against the
reference: the neighbour sets on the float clouds, the ranked distances on the
lattice clouds (topk's tie order is arbitrary there), and the recorded
get_graph_features bytes."""
import os

import numpy as np
import pytest
import torch

import knn_graph_ref as kr
from grouping_ref import sqdist

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, "tests", "golden", "knn_golden.npz"))
CLOUDS = sorted(k.split("/")[1] for k in G.files if k.startswith("cloud/"))
TOPK = sorted(k for k in G.files if k.startswith("topk/"))
KS = (1, 10, 32, 63)


@pytest.fixture(scope="module")
def grp():
    from pointcloudregistration_amd import grouping
    return grouping


def _gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(t):
    return t.cpu().numpy()


def _same_bits(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, what
    bad = got.view(np.uint32) != want.view(np.uint32)
    assert not bad.any(), f"{what}: {bad.sum()} of {bad.size} values differ"


def _check_knn(grp, x, k):
    want_idx, want_d2 = kr.knn_graph(x, k)
    idx, d2 = grp.knn_graph(_gpu(x), k, return_dists=True)
    assert idx.dtype == torch.int64 and d2.dtype == torch.float32 and idx.is_cuda
    assert tuple(idx.shape) == want_idx.shape == (x.shape[0], x.shape[1], min(k, x.shape[1] - 1))
    assert np.array_equal(_np(idx), want_idx)
    _same_bits(_np(d2), want_d2, "d2")
    assert torch.equal(grp.knn_graph(_gpu(x), k), idx)       # without the distances: same rows
    return _np(idx), _np(d2)


# --------------------------------------------------------------------- knn_graph
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("c", CLOUDS)
def test_knn_graph_equals_restatement(grp, c, k):
    _check_knn(grp, G[f"cloud/{c}"], k)


@pytest.mark.parametrize("key", TOPK)
def test_knn_graph_equals_reference(grp, key):
    _, c, k = key.split("/")
    x, k, picks = G[f"cloud/{c}"], int(k[1:]), G[key].astype(np.int64)
    idx, d2 = grp.knn_graph(_gpu(x), k, return_dists=True)
    idx, d2 = _np(idx), _np(d2)
    if c.startswith("f"):
        # the neighbour set of every row, and the dropped column is the row itself
        assert np.array_equal(np.sort(idx, -1), np.sort(picks[..., 1:], -1))
        assert (picks[..., 0] == np.arange(x.shape[1])[None, :]).all()
    else:
        # the ranked direct-form distances of the reference's picks, rank 0 dropped
        b = x.shape[0]
        ref = np.sort(sqdist(x[:, :, None, :], x[np.arange(b)[:, None, None], picks]), axis=-1)
        _same_bits(d2, ref[..., 1:], "ranked distances")


@pytest.mark.parametrize("n", [1, 2, 11, 12, 63, 64, 65])
def test_knn_graph_path_edges(grp, n):
    """k = 10: kk = n - 1 (n <= 11), k + 1 = n (n = 11), the wave boundary."""
    x = np.random.default_rng((7, n)).uniform(-1, 1, (2, n, 3)).astype(np.float32)
    idx, _ = _check_knn(grp, x, 10)
    assert idx.shape[2] == min(10, n - 1)


@pytest.mark.parametrize("n", [64, 65])
def test_knn_graph_k63(grp, n):
    x = np.random.default_rng((63, n)).uniform(-1, 1, (2, n, 3)).astype(np.float32)
    idx, _ = _check_knn(grp, x, 63)
    assert idx.shape[2] == 63


@pytest.fixture(scope="module")
def big_cloud():
    return np.random.default_rng(8193).uniform(-1, 1, (1, 8193, 3)).astype(np.float32)


def test_knn_graph_across_every_lds_chunk(grp, big_cloud):
    """8193 points: four full stages of the cloud and one point in a fifth."""
    idx, _ = _check_knn(grp, big_cloud, 10)
    assert (idx >= 8192).any() and (idx < 2048).any()


def test_knn_graph_batches_are_independent(grp):
    x = np.random.default_rng(3).uniform(-1, 1, (3, 300, 3)).astype(np.float32)
    idx, d2 = _check_knn(grp, x, 10)
    for c in range(3):
        i1, d1 = grp.knn_graph(_gpu(x[c:c + 1]), 10, return_dists=True)
        assert np.array_equal(_np(i1), idx[c:c + 1])
        _same_bits(_np(d1), d2[c:c + 1], "d2")
    assert not np.array_equal(idx[0], idx[1])


def test_knn_graph_identical_points(grp):
    """Every distance is 0: rank r is index r, rank 0 (index 0) is dropped."""
    x = np.full((2, 70, 3), 0.375, np.float32)
    idx, d2 = _check_knn(grp, x, 10)
    assert (idx == np.arange(1, 11)).all() and (d2 == 0).all()


# ---------------------------------------------------------------- graph_features
@pytest.fixture(scope="module")
def feat_case():
    x = G["cloud/f257"]
    f = np.random.default_rng(256).standard_normal((2, 257, 256)).astype(np.float32)
    idx, _ = kr.knn_graph(x, 10)
    return x, f, idx


@pytest.mark.parametrize("c", [1, 3, 64, 65, 256])
def test_graph_features_equal_restatement(grp, feat_case, c):
    x, f, idx = feat_case
    f = np.ascontiguousarray(f[..., :c])
    want = kr.edge_features(f, idx)
    cl = grp.graph_features(_gpu(f), coords=_gpu(x), k=10)
    cf = grp.graph_features(_gpu(f), coords=_gpu(x), k=10, channels_first=True)
    assert tuple(cl.shape) == (2, 257, 10, 2 * c) and tuple(cf.shape) == (2, 2 * c, 257, 10)
    assert cl.is_contiguous() and cf.is_contiguous()
    _same_bits(_np(cl), want, "channels_last")
    _same_bits(_np(cf), kr.edge_features(f, idx, channels_first=True), "channels_first")
    _same_bits(_np(cf.permute(0, 2, 3, 1)), _np(cl), "channels_first vs channels_last")


def test_graph_features_equal_reference(grp):
    x, f, k = G["feat/cloud"], G["feat/feats"], int(G["feat/k"])
    ref = G["feat/out"]
    out, inds = grp.graph_features(_gpu(f), coords=_gpu(x), k=k, return_inds=True)
    _same_bits(_np(out), ref, "get_graph_features")
    cf = grp.graph_features(_gpu(f), coords=_gpu(x), k=k, channels_first=True)
    _same_bits(_np(cf), np.transpose(ref, (0, 3, 1, 2)), "get_graph_features, permuted")
    assert inds.dtype == torch.int64 and np.array_equal(_np(inds), kr.knn_graph(x, k)[0])


@pytest.mark.parametrize("n", [1, 5])
def test_graph_features_small_clouds_have_the_reference_shapes(grp, n):
    x = torch.rand(2, n, 3, device="cuda")
    f = torch.rand(2, n, 8, device="cuda")
    want = tuple(G[f"shape/n{n}/k10"])
    out, inds = grp.graph_features(f, coords=x, k=10, return_inds=True)
    assert tuple(out.shape) == want and tuple(inds.shape) == (2, n, n - 1)
    assert tuple(grp.graph_features(f, coords=x, k=10, channels_first=True).shape) == \
        (want[0], want[3], want[1], want[2])
    assert tuple(grp.knn_graph(x, 10).shape) == (2, n, n - 1)
    if n > 1:
        _same_bits(_np(out), kr.edge_features(_np(f), _np(inds)), "n = 5")


def test_inds_and_coords_give_the_same_bytes(grp, feat_case):
    x, f, idx = feat_case
    fd, xd = _gpu(f[..., :64]), _gpu(x)
    inds = grp.knn_graph(xd, 10)
    for cf in (False, True):
        a, ia = grp.graph_features(fd, coords=xd, k=10, channels_first=cf, return_inds=True)
        b, ib = grp.graph_features(fd, inds=inds, channels_first=cf, return_inds=True)
        c = grp.graph_features(fd, inds=inds.int(), channels_first=cf)
        assert torch.equal(ia, inds) and torch.equal(ib, inds)
        _same_bits(_np(a), _np(b), "inds vs coords")
        _same_bits(_np(a), _np(c), "int32 inds")


def test_side_stream_non_contiguous_and_repeat(grp, feat_case):
    x, f, idx = feat_case
    xd, fd = _gpu(x), _gpu(f[..., :65])
    i0, d0 = grp.knn_graph(xd, 10, return_dists=True)
    o0 = grp.graph_features(fd, inds=i0)
    c0 = grp.graph_features(fd, inds=i0, channels_first=True)
    # twice: identical bytes
    i1, d1 = grp.knn_graph(xd, 10, return_dists=True)
    assert torch.equal(i0, i1)
    _same_bits(_np(d0), _np(d1), "d2, second run")
    _same_bits(_np(grp.graph_features(fd, inds=i0)), _np(o0), "features, second run")
    # a non-default stream
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        i2, d2 = grp.knn_graph(xd, 10, return_dists=True)
        o2 = grp.graph_features(fd, coords=xd, k=10)
        c2 = grp.graph_features(fd, inds=i2, channels_first=True)
    side.synchronize()
    assert torch.equal(i0, i2)
    _same_bits(_np(d0), _np(d2), "d2, side stream")
    _same_bits(_np(o2), _np(o0), "features, side stream")
    _same_bits(_np(c2), _np(c0), "channels_first, side stream")
    # non-contiguous inputs: (B,3,N) / (B,C,N) views, as GCN.forward holds them
    xt = xd.permute(0, 2, 1).contiguous().permute(0, 2, 1)
    ft = fd.permute(0, 2, 1).contiguous().permute(0, 2, 1)
    assert not xt.is_contiguous() and not ft.is_contiguous()
    assert torch.equal(grp.knn_graph(xt, 10), i0)
    _same_bits(_np(grp.graph_features(ft, coords=xt, k=10)), _np(o0), "non-contiguous")
    _same_bits(_np(grp.graph_features(ft, inds=i0[:, :, ::1], channels_first=True)), _np(c0),
               "non-contiguous, channels_first")


def test_bad_inputs_raise(grp):
    xc = torch.from_numpy(G["cloud/l65"])
    fc = torch.zeros(1, 65, 4)
    x, f = xc.cuda(), fc.cuda()
    with pytest.raises(ValueError, match="CUDA"):
        grp.knn_graph(xc, 4)
    with pytest.raises(ValueError, match="CUDA"):
        grp.graph_features(fc, coords=xc, k=4)
    with pytest.raises(ValueError, match="float32"):
        grp.knn_graph(x.double(), 4)
    with pytest.raises(ValueError, match="float32"):
        grp.graph_features(f.double(), coords=x, k=4)
    with pytest.raises(ValueError, match="float32"):
        grp.graph_features(f, coords=x.double(), k=4)
    with pytest.raises(ValueError, match="match"):
        grp.graph_features(f.expand(2, -1, -1), coords=x, k=4)          # mismatched batch
    inds = grp.knn_graph(x, 4)
    with pytest.raises(ValueError, match="inds must be"):
        grp.graph_features(f.expand(2, -1, -1), inds=inds)
    with pytest.raises(ValueError, match="exactly one"):
        grp.graph_features(f, coords=x, inds=inds)
    with pytest.raises(ValueError, match="exactly one"):
        grp.graph_features(f)
    with pytest.raises(ValueError, match="integer"):
        grp.graph_features(f, inds=inds.float())
    for k in (0, 64, -1):
        with pytest.raises(ValueError, match="outside 1..63"):
            grp.knn_graph(x, k)
        with pytest.raises(ValueError, match="outside 1..63"):
            grp.graph_features(f, coords=x, k=k)
    xg, fg = x.clone().requires_grad_(True), f.clone().requires_grad_(True)
    with pytest.raises(RuntimeError, match="forward-only"):
        grp.knn_graph(xg, 4)
    with pytest.raises(RuntimeError, match="forward-only"):
        grp.graph_features(fg, coords=x, k=4)
    with pytest.raises(RuntimeError, match="forward-only"):
        grp.graph_features(f, coords=xg, k=4)
    with torch.no_grad():                                   # grad mode off: nothing to cut
        assert grp.graph_features(fg, coords=xg, k=4).shape == (1, 65, 4, 8)
