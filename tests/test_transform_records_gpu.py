"""GPU: transform_batch and the C4 record kernel (csrc/procrustes.hip) at tails,
with caller-owned outputs, and the record's Chamfer sum in its real order.

transform_batch: bit-equal to records_ref.transform_f32 (((R0 x + R1 y) + R2 z)
+ t in f64, rounded to f32) for N around the 256-thread block and B in {1, 3},
a general upper 3x4 and a garbage fourth row; nothing outside a caller's `out`
is written; empty inputs touch nothing; B > 65535 is refused.

pcr_pipeline_records, called on its own through _PipelineIO with crafted device
buffers (P = 3, D = 1): slots 0-35 and 37-39 are the inputs bit for bit; slot
36 is records_ref.chamfer_mean bit for bit -- the 1024-lane order -- on
distances over 2^-40 ... 2^20 that tell that order apart from the 256-lane
order and from np.sum (asserted on the CPU before the GPU call), and within the
order-free bound (N + M) 2^-53 of the math.fsum means; a lone 1.0 among zeros
is found at every guard of the 8-wide runs.
"""
import ctypes

import numpy as np
import pytest
import torch

import records_ref as rr

pytestmark = pytest.mark.gpu
SENTINEL = 0x7FC5A5A5          # a quiet NaN with a payload no kernel here writes


# ---------------------------------------------------------------------------
# transform_batch
# ---------------------------------------------------------------------------
def _general_T(rng, B):
    """Non-orthogonal upper 3x4 (so a transposed or normalised R shows) and a
    fourth row that must not be read."""
    T = rng.uniform(-2.0, 2.0, (B, 4, 4))
    T[:, 3] = [np.nan, np.inf, -1e300, 7.0]
    return T


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("N", [1, 255, 256, 257, 1000])
def test_transform_batch_tails(N, B):
    from pointcloudregistration_amd import registration as reg
    rng = np.random.default_rng([N, B])
    x = rng.uniform(-1, 1, (B, N, 3)).astype(np.float32)
    T = _general_T(rng, B)
    want = rr.transform_f32(x, T)
    xg, Tg = torch.from_numpy(x).cuda(), torch.from_numpy(T).cuda()
    got = reg.transform_batch(xg, Tg)
    assert got.dtype == torch.float32 and got.shape == (B, N, 3)
    assert got.cpu().numpy().tobytes() == want.tobytes()
    # caller's out: a view into a larger buffer of sentinels
    pad, n = 1031, B * N * 3
    buf = torch.full((pad + n + pad,), SENTINEL, dtype=torch.int32, device="cuda")
    out = buf.view(torch.float32)[pad:pad + n].view(B, N, 3)
    ret = reg.transform_batch(xg, Tg, out=out)
    assert ret.data_ptr() == out.data_ptr()
    host = buf.cpu().numpy()
    assert np.all(host[:pad] == SENTINEL) and np.all(host[pad + n:] == SENTINEL)
    assert host[pad:pad + n].view(np.float32).tobytes() == want.tobytes()


@pytest.mark.parametrize("shape", [(3, 0, 3), (0, 7, 3)])
def test_transform_batch_empty_touches_nothing(shape):
    from pointcloudregistration_amd import registration as reg
    buf = torch.full((64,), SENTINEL, dtype=torch.int32, device="cuda")
    T = torch.zeros(shape[0], 4, 4, dtype=torch.float64, device="cuda")
    x = torch.empty(shape, device="cuda")
    reg.transform_batch(x, T, out=buf.view(torch.float32))
    assert torch.all(buf == SENTINEL)
    assert reg.transform_batch(x, T).shape == shape


def test_transform_batch_refuses_large_batch():
    from pointcloudregistration_amd import _lib, registration as reg
    B = 65536       # the batch rides on gridDim.y; N = 1: an empty call returns before the check
    x = torch.zeros(B, 1, 3, device="cuda")
    T = torch.zeros(B, 4, 4, dtype=torch.float64, device="cuda")
    with pytest.raises(_lib.PcrError, match="B=65536 > 65535"):
        reg.transform_batch(x, T)


# ---------------------------------------------------------------------------
# pcr_pipeline_records
# ---------------------------------------------------------------------------
def _inputs(rng, P):
    """Every buffer the record kernel copies, with values whose bits must
    survive (signed zero, infinities, a subnormal) and stats columns that
    cannot be mistaken for each other."""
    f = dict(T_ransac=rng.standard_normal((P, 16)), T_icp=rng.standard_normal((P, 16)),
             fit_ransac=rng.random((P, 2)), fit_icp=rng.random((P, 2)))
    f["T_ransac"][0, :4] = [-0.0, np.inf, -np.inf, 5e-324]
    f["T_icp"][-1, -1] = -0.0
    i = dict(stats_ransac=(np.arange(P * 5).reshape(P, 5) * 1000 + 17).astype(np.int32),
             stats_icp=np.full((P, 2), -7, np.int32),
             n_corres=rng.integers(0, 1 << 30, P).astype(np.int32))
    i["stats_ransac"][0, 0] = 2 ** 31 - 1
    return f, i


def _run_records(d1, d2, f, i, P=None, N=None, M=None, spare_rows=1):
    """pcr_pipeline_records on crafted buffers -> records (P + spare_rows, 40)."""
    from pointcloudregistration_amd import _lib
    from pointcloudregistration_amd.pipeline import _PipelineIO
    d1, d2 = np.atleast_2d(d1), np.atleast_2d(d2)
    P = d1.shape[0] if P is None else P
    dev = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in {**f, **i}.items()}
    dev["d1"] = torch.from_numpy(np.ascontiguousarray(d1, np.float32)).cuda()
    dev["d2"] = torch.from_numpy(np.ascontiguousarray(d2, np.float32)).cuda()
    rec = torch.full((P + spare_rows, 40), float("nan"), dtype=torch.float64, device="cuda")
    io = _PipelineIO()
    io.P, io.D = P, 1
    io.N = d1.shape[1] if N is None else N
    io.M = d2.shape[1] if M is None else M
    for k, t in dev.items():
        assert t.data_ptr() != 0
        setattr(io, k, t.data_ptr())
    io.records = rec.data_ptr()
    _lib.call("pcr_pipeline_records", ctypes.byref(io), _lib.stream_handle(rec.device))
    return rec.cpu().numpy()


def _bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("N,M", rr.SHAPES)
def test_records_slots_and_chamfer_order(N, M):
    d1, d2 = rr.distances(N, M)
    # on the CPU, before the GPU call: these inputs tell the orders apart
    assert rr.discriminates(d1, d2)
    want = rr.chamfer_mean(d1, d2)
    if max(N, M) >= 1024:
        assert np.any((want != rr.chamfer_mean_256(d1, d2)) & (want != rr.chamfer_mean_np(d1, d2)))
    f, i = _inputs(np.random.default_rng([N, M, 1]), rr.P)
    rec = _run_records(d1, d2, f, i)
    P = rr.P
    assert np.all(np.isnan(rec[P]))                                  # nothing past the P records
    assert _bits(rec[:P, 0:16], f["T_ransac"]) and _bits(rec[:P, 16:32], f["T_icp"])
    assert _bits(rec[:P, 32:34], f["fit_ransac"]) and _bits(rec[:P, 34:36], f["fit_icp"])
    assert _bits(rec[:P, 37], i["stats_ransac"][:, 0].astype(np.float64))
    assert _bits(rec[:P, 38], i["stats_ransac"][:, 3].astype(np.float64))
    assert _bits(rec[:P, 39], i["n_corres"].astype(np.float64))
    got = rec[:P, 36]
    print(f"FIG records ({N},{M}): got {got.tolist()} want {want.tolist()}")
    assert _bits(got, want)
    # any order: n non-negative terms sum within (n - 1) u relative (u = 2^-53),
    # each division and the last addition add u: below (N + M) u for both means
    ref = rr.chamfer_mean_fsum(d1, d2)
    assert np.all(np.abs(got - ref) <= (N + M) * 2.0 ** -53 * ref)


def _probe_positions(n):
    """Indices where an element can go missing: both ends, the wave and block
    edges, and the last index of each 8-wide run boundary (7 * 1024 + t is the
    eighth element of thread t's first run, 8 * 1024 + t the first of its
    second; the i < len guard cuts inside a run)."""
    cand = [0, 1, 63, 64, 1023, 1024, 7 * 1024 - 1, 7 * 1024, 7 * 1024 + 5, 8 * 1024 - 1, 8 * 1024,
            8 * 1024 + 5, 8 * 1024 + 807, n - 2, n - 1]
    return sorted({c for c in cand if 0 <= c < n})


@pytest.mark.parametrize("N,M", rr.SHAPES)
def test_records_lone_one_is_never_dropped(N, M):
    """d all zeros except 1.0 at one index: slot 36 is exactly 1 / len, wherever
    the index falls (no wide magnitudes needed: a dropped element reads 0)."""
    f, i = _inputs(np.random.default_rng(5), rr.P)
    for side, n in ((0, N), (1, M)):
        pos = _probe_positions(n)
        for k in range(0, len(pos), rr.P):
            chunk = (pos[k:k + rr.P] * rr.P)[:rr.P]
            d = [np.zeros((rr.P, N), np.float32), np.zeros((rr.P, M), np.float32)]
            for p, c in enumerate(chunk):
                d[side][p, c] = 1.0
            rec = _run_records(d[0], d[1], f, i)
            assert np.array_equal(rec[:rr.P, 36], np.full(rr.P, 1.0 / n)), (side, chunk, rec[:rr.P, 36])


def test_records_empty_clouds_and_no_pairs():
    from pointcloudregistration_amd import _lib
    f, i = _inputs(np.random.default_rng(6), rr.P)
    d = np.ones((rr.P, 4), np.float32)
    for N, M in ((0, 4), (4, 0)):
        with pytest.raises(_lib.PcrError, match="empty clouds"):
            _run_records(d, d, f, i, N=N, M=M)
    rec = _run_records(d, d, f, i, P=0, spare_rows=rr.P)      # P = 0: OK, nothing written
    assert np.all(np.isnan(rec))
