"""f2: Open3D voxel_down_sample (dip/demo.py:73-74) on the GPU vs the oracle's
restatement of PointCloud::VoxelDownSample (oracle/voxel_oracle.cpp) -- bit for
bit, emission order included -- and vs an independent numpy grouping (order-free
check of the voxel means).  Open3D is absent: parity vs Open3D itself is
unpinned beyond its published algorithm."""
import numpy as np
import pytest

from pointcloudregistration_amd import geometry, registration as reg, synth
from voxel_cases import _numpy_groups, sorted_rows as _sorted_rows

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n,voxel,scale", [(10000, 1.0, 40.0), (3000, 0.05, 1.0), (20000, 0.025, 1.0),
                                           (500, 10.0, 40.0)])
def test_voxel_down_sample_vs_oracle(oracle, n, voxel, scale):
    rng = np.random.default_rng(n)
    pts = synth.surface_points(rng, n) * scale
    out = reg.PointCloud(pts).voxel_down_sample(voxel)
    ref, _, _ = oracle.voxel_down_sample(pts, voxel)
    assert np.asarray(out.points).tobytes() == ref.tobytes()
    assert np.array_equal(_sorted_rows(ref), _sorted_rows(_numpy_groups(pts, voxel)))


def test_voxel_down_sample_normals_colors_nan_and_dups(oracle):
    rng = np.random.default_rng(3)
    pts = np.round(rng.random((4000, 3)) * 8) / 8.0       # many exact duplicates
    nrm = rng.standard_normal((4000, 3))
    nrm[::7, 1] = np.nan                                   # skipped by AddPoint
    col = rng.random((4000, 3))
    pcd = reg.PointCloud(pts)
    pcd.normals, pcd.colors = nrm, col
    out = pcd.voxel_down_sample(0.2)
    rp, rn, rc = oracle.voxel_down_sample(pts, 0.2, nrm, col)
    assert np.asarray(out.points).tobytes() == rp.tobytes()
    assert out.normals.tobytes() == rn.tobytes() and out.colors.tobytes() == rc.tobytes()
    # uniform painting survives (demo.py paints before down-sampling)
    p2 = reg.PointCloud(pts).paint_uniform_color([0.5, 0.3, 0.6]).voxel_down_sample(0.2)
    assert np.allclose(p2.colors, [0.5, 0.3, 0.6], rtol=0, atol=1e-15)


def test_voxel_down_sample_batch_equals_single(oracle):
    rng = np.random.default_rng(8)
    clouds = [synth.surface_points(rng, k) * 30 if k else np.zeros((0, 3)) for k in (5000, 0, 123, 9000)]
    outs = geometry.voxel_down_sample_batch(clouds, 1.5)
    for c, (p, _, _) in zip(clouds, outs):
        ref, _, _ = oracle.voxel_down_sample(c, 1.5) if len(c) else (np.zeros((0, 3)), None, None)
        assert p.cpu().numpy().tobytes() == ref.tobytes()


def test_voxel_down_sample_errors():
    pts = np.random.default_rng(0).random((100, 3))
    with pytest.raises(Exception, match="voxel_size <= 0"):
        reg.PointCloud(pts).voxel_down_sample(0.0)
    with pytest.raises(Exception, match="too small"):
        reg.PointCloud(pts * 1e6).voxel_down_sample(1e-6)
    bad = pts.copy()
    bad[3, 1] = np.inf
    with pytest.raises(Exception, match="non-finite"):
        reg.PointCloud(bad).voxel_down_sample(0.1)
