"""GPU: farthest-point sampling, ball query, sample_and_group and the fused
point-pair group (pointcloudregistration_amd.grouping) against the reference's
outputs in tests/golden/grouping_golden.npz and, where the fixture has no case,
against the numpy restatement that tests/test_grouping_cpu.py pins to it.

Bars.  Every index array, the density and channels 0-5 of the features:
bit-equal.  Channels 6-9 (three atan2f angles, one sqrtf norm): within 4x the
fixture's recorded spread of the f64 evaluation of the same formulas on the
same f32 normals and f32 g -- the spread is the reference's own distance from
that evaluation; the device's atan2f / sqrtf and the host libm are different
few-ulp implementations (hence the factor), while the products and differences
that feed them are identical without FMA."""
import os

import numpy as np
import pytest
import torch

import grouping_ref as gr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, "tests", "golden", "grouping_golden.npz"))
FPS_SEED = 77   # make_golden_grouping.py
CLOUDS = sorted(k.split("/")[1] for k in G.files if k.startswith("cloud/"))
FPS = sorted(k for k in G.files if k.startswith("fps/"))
BQ = sorted(k[:-4] for k in G.files if k.startswith("bq/") and k.endswith("/idx"))
SG = sorted({k.split("/")[1] for k in G.files if k.startswith("sg/")})
PPF = sorted({k.split("/")[1] for k in G.files if k.startswith("ppf/")})


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


# --------------------------------------------------------------------------- fps
@pytest.mark.parametrize("key", FPS)
def test_fps_equals_reference(grp, key):
    _, c, m = key.split("/")
    want = G[key].astype(np.int64)
    got = grp.fps(_gpu(G[f"cloud/{c}"]), int(m[1:]), start=torch.from_numpy(want[:, 0].copy()))
    assert got.dtype == torch.int64 and got.is_cuda
    assert np.array_equal(_np(got), want)


def test_fps_draws_the_reference_start(grp):
    x = _gpu(G["cloud/l257"])
    torch.manual_seed(FPS_SEED)
    got = grp.fps(x, 3)
    assert np.array_equal(_np(got), G["fps/l257/m3"].astype(np.int64))


@pytest.fixture(scope="module")
def big_cloud():
    return np.random.default_rng(8192).uniform(-1, 1, (1, 8193, 3)).astype(np.float32)


@pytest.mark.parametrize("n", [2048, 2049, 8192, 8193])
def test_fps_contract_at_the_path_boundaries(grp, big_cloud, n):
    """2 / 8 points per thread in registers (<= 2048 / <= 8192 points) and the
    overflow path above, against the restatement."""
    x = big_cloud[:, :n]
    start = np.array([n - 1])
    want = gr.fps(x, start, 32)
    got = grp.fps(_gpu(x), 32, start=torch.from_numpy(start))
    assert np.array_equal(_np(got), want)


def test_fps_register_and_overflow_paths_agree(grp, big_cloud):
    """8192 points from registers; the same cloud with a copy of point 0 appended
    takes the overflow path, and the copy (equal distance, higher index) is never
    picked: identical samples."""
    x = big_cloud[:, :8192]
    y = np.concatenate([x, x[:, :1]], axis=1)
    start = torch.tensor([5])
    a = grp.fps(_gpu(x), 64, start=start)
    b = grp.fps(_gpu(y), 64, start=start)
    assert torch.equal(a, b)


@pytest.mark.parametrize("extra", [0, 3])
def test_fps_all_points_and_beyond_on_the_ropnet_cloud(grp, extra):
    """m = n and m = n + 3 at 2048 float points: the contract (the reference's own
    expanded-form rounding leaves it there; see the generator's docstring)."""
    x = G["cloud/f2048"]
    start = G["fps/f2048/m1"][:, 0].astype(np.int64)
    want = gr.fps(x, start, 2048 + extra)
    got = grp.fps(_gpu(x), 2048 + extra, start=torch.from_numpy(start))
    assert np.array_equal(_np(got), want)
    assert np.array_equal(np.sort(want[:, :2048], axis=1), np.tile(np.arange(2048), (2, 1)))


# -------------------------------------------------------------------- ball query
@pytest.mark.parametrize("key", BQ)
def test_ball_query_equals_reference(grp, key):
    _, c, r, k = key.split("/")
    x = _gpu(G[f"cloud/{c}"])
    n = x.shape[1]
    want = G[key + "/idx"].astype(np.int64)
    idx, density = grp.ball_query(x, x, float(r[1:]), int(k[1:]), rt_density=True)
    assert idx.dtype == torch.int64 and tuple(idx.shape) == want.shape   # min(K, N) columns
    assert np.array_equal(_np(idx), want)
    assert density.dtype == torch.float32
    want_density = (torch.from_numpy(G[key + "/count"].astype(np.int64)) / n).numpy()
    _same_bits(_np(density), want_density, "density")
    # without the counts a full row stops the scan early: same rows
    assert torch.equal(grp.ball_query(x, x, float(r[1:]), int(k[1:])), idx)


def test_ball_query_without_neighbours_returns_the_sentinel(grp):
    x = _gpu(G["cloud/l65"])
    q = torch.full((1, 3, 3), 50.0, device="cuda")
    q[0, 1] = x[0, 7]
    idx, density = grp.ball_query(x, q, 0.25, 16, rt_density=True)
    assert (idx[0, 0] == 65).all() and (idx[0, 2] == 65).all()
    assert density[0, 0] == 0 and density[0, 2] == 0
    assert (idx[0, 1] < 65).all() and density[0, 1] > 0


def test_ball_query_more_points_than_one_lds_stage(grp, big_cloud):
    """4100 points: three stages of the cloud, neighbours appended across them."""
    x = big_cloud[:, :4100]
    q = x[:, ::41]
    want, wcount = gr.ball_query(x, q, 0.2, 24)
    idx, density = grp.ball_query(_gpu(x), _gpu(q), 0.2, 24, rt_density=True)
    assert np.array_equal(_np(idx), want)
    assert np.array_equal(_np(density), (torch.from_numpy(wcount) / 4100).numpy())
    assert (wcount > 24).any() and (wcount < 24).any()
    assert torch.equal(grp.ball_query(_gpu(x), _gpu(q), 0.2, 24), idx)


# -------------------------------------------------------------- sample_and_group
@pytest.mark.parametrize("c", SG)
def test_sample_and_group_with_fps_equals_reference(grp, c):
    x = _gpu(G[f"cloud/{c}"])
    M, r, k = int(G[f"sg/{c}/M"]), float(G[f"sg/{c}/r"]), int(G[f"sg/{c}/k"])
    torch.manual_seed(FPS_SEED)
    new_xyz, new_points, inds, grouped_xyz, density = grp.sample_and_group(
        x, None, M, r, k, rt_density=True)
    _same_bits(_np(new_xyz), G[f"sg/{c}/new_xyz"], "new_xyz")
    assert np.array_equal(_np(inds), G[f"sg/{c}/idx"].astype(np.int64))
    _same_bits(_np(density), (torch.from_numpy(G[f"sg/{c}/count"].astype(np.int64)) / x.shape[1]).numpy(),
               "density")
    xh, ih = G[f"cloud/{c}"], G[f"sg/{c}/idx"].astype(np.int64)
    want = xh[np.arange(xh.shape[0])[:, None, None], ih] - G[f"sg/{c}/new_xyz"][:, :, None, :]
    _same_bits(_np(grouped_xyz), want, "grouped_xyz")
    assert torch.equal(new_points, grouped_xyz)


@pytest.mark.parametrize("p", PPF)
def test_sample_and_group_every_point_a_centre(grp, p):
    c = str(G[f"ppf/{p}/cloud"])
    r, k = float(G[f"ppf/{p}/r"]), int(G[f"ppf/{p}/k"])
    x, nrm = _gpu(G[f"cloud/{c}"]), _gpu(G[f"ppf/{p}/normals"])
    new_xyz, new_points, inds, grouped_xyz = grp.sample_and_group(x, nrm, -1, r, k)
    assert new_xyz is x or torch.equal(new_xyz, x)
    assert np.array_equal(_np(inds), G[f"bq/{c}/r{r}/k{k}/idx"].astype(np.int64))
    ref = np.transpose(G[f"ppf/{p}/feat10"], (0, 3, 2, 1))
    _same_bits(_np(grouped_xyz), ref[..., 3:6], "grouped_xyz")
    _same_bits(_np(new_points[..., :3]), ref[..., 3:6], "new_points xyz")
    assert torch.equal(new_points[..., 3:], grp.gather_points(nrm, inds))


# ------------------------------------------------------------------- fused group
@pytest.mark.parametrize("p", PPF)
def test_local_ppf_features_equal_reference(grp, p):
    c = str(G[f"ppf/{p}/cloud"])
    r, k = float(G[f"ppf/{p}/r"]), int(G[f"ppf/{p}/k"])
    xh, nh = G[f"cloud/{c}"], G[f"ppf/{p}/normals"]
    x, nrm = _gpu(xh), _gpu(nh)
    ref10, ref6 = G[f"ppf/{p}/feat10"], G[f"ppf/{p}/feat6"]
    want_idx = G[f"bq/{c}/r{r}/k{k}/idx"].astype(np.int64)

    cf, inds = grp.local_ppf_features(x, nrm, r, k, channels_first=True, return_inds=True)
    assert tuple(cf.shape) == ref10.shape and inds.dtype == torch.int64
    assert np.array_equal(_np(inds), want_idx)
    cf = _np(cf)
    _same_bits(cf[:, :6], ref10[:, :6], "channels 0-5")
    e64 = np.transpose(gr.group_ppf(xh, nh, want_idx, np.float64), (0, 3, 2, 1))
    sa, sn = float(G[f"ppf/{p}/spread_angle"]), float(G[f"ppf/{p}/spread_norm"])
    ea = np.abs(cf[:, 6:9] - e64[:, 6:9]).max()
    en = np.abs(cf[:, 9] - e64[:, 9]).max()
    print(f"{p}: angles {ea:.3e} (spread {sa:.3e}), norm {en:.3e} (spread {sn:.3e})")
    assert ea <= 4 * sa
    assert en <= 4 * sn
    assert (cf[:, 6][cf[:, 9] == 0] == 0).all()          # angle(n_i, 0) = 0, negative normals included

    cl = grp.local_ppf_features(x, nrm, r, k, channels_first=False)
    _same_bits(np.transpose(_np(cl), (0, 3, 2, 1)), cf, "channels_last vs channels_first")
    six = grp.local_ppf_features(x, None, r, k)
    _same_bits(_np(six), ref6, "6 channels")
    six_cl = grp.local_ppf_features(x, None, r, k, channels_first=False)
    _same_bits(np.transpose(_np(six_cl), (0, 3, 2, 1)), ref6, "6 channels, channels_last")


@pytest.mark.parametrize("c,r,k", [("f2048", 0.3, 64), ("l65", 0.5, 5), ("l1025", 0.5, 33)])
def test_local_ppf_features_tiles(grp, c, r, k):
    """The ROPNet shape, and K / N that are no multiple of the 16 x 64 tile: the
    group indices and channels 0-5 against the restatement, both layouts."""
    xh = G[f"cloud/{c}"]
    nh = np.roll(xh, 1, axis=1)      # any vectors do: channels 6-9 are compared between the layouts only
    want_idx, _ = gr.ball_query(xh, xh, r, k)
    want = gr.group_ppf(xh, None, want_idx)
    cf, inds = grp.local_ppf_features(_gpu(xh), _gpu(nh), r, k, return_inds=True)
    cl = grp.local_ppf_features(_gpu(xh), _gpu(nh), r, k, channels_first=False)
    assert np.array_equal(_np(inds), want_idx)
    _same_bits(_np(cl)[..., :6], want, "channels 0-5")
    _same_bits(np.transpose(_np(cf), (0, 3, 2, 1)), _np(cl), "layouts")


# ------------------------------------------------------------------ the interface
def test_cpu_tensors_and_grad_inputs_raise(grp):
    xc = torch.from_numpy(G["cloud/l65"])
    with pytest.raises(ValueError, match="CUDA"):
        grp.fps(xc, 4)
    with pytest.raises(ValueError, match="CUDA"):
        grp.ball_query(xc, xc, 0.25, 4)
    with pytest.raises(ValueError, match="CUDA"):
        grp.sample_and_group(xc, None, -1, 0.25, 4)
    with pytest.raises(ValueError, match="CUDA"):
        grp.local_ppf_features(xc, None, 0.25, 4)
    xg = xc.cuda().requires_grad_(True)
    x = xc.cuda()
    with pytest.raises(RuntimeError, match="forward-only"):
        grp.fps(xg, 4)
    with pytest.raises(RuntimeError, match="forward-only"):
        grp.ball_query(x, xg, 0.25, 4)
    with pytest.raises(RuntimeError, match="forward-only"):
        grp.sample_and_group(x, xg, -1, 0.25, 4)
    with pytest.raises(RuntimeError, match="forward-only"):
        grp.local_ppf_features(x, xg, 0.25, 4)
    with torch.no_grad():                                   # grad mode off: nothing to cut
        assert grp.fps(xg, 4, start=torch.tensor([0])).shape == (1, 4)
    with pytest.raises(ValueError, match="start"):
        grp.fps(x, 4, start=torch.tensor([65]))


def test_side_stream_and_batch_independence(grp):
    """b = 3 on a non-default stream gives the rows of three b = 1 calls."""
    xh, nh = G["cloud/l257"], G["ppf/l257/normals"]
    x, nrm = _gpu(xh), _gpu(nh)
    start = torch.tensor([3, 100, 256])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        s3 = grp.fps(x, 40, start=start)
        i3, d3 = grp.ball_query(x, x, 0.5, 16, rt_density=True)
        f3, j3 = grp.local_ppf_features(x, nrm, 0.25, 16, return_inds=True)
    side.synchronize()
    for c in range(3):
        xc, nc = x[c:c + 1].contiguous(), nrm[c:c + 1].contiguous()
        assert torch.equal(grp.fps(xc, 40, start=start[c:c + 1]), s3[c:c + 1])
        i1, d1 = grp.ball_query(xc, xc, 0.5, 16, rt_density=True)
        assert torch.equal(i1, i3[c:c + 1]) and torch.equal(d1, d3[c:c + 1])
        f1, j1 = grp.local_ppf_features(xc, nc, 0.25, 16, return_inds=True)
        assert torch.equal(j1, j3[c:c + 1])
        _same_bits(_np(f1), _np(f3[c:c + 1]), "features")
