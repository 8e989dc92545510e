"""The batch Chamfer's LDS-resident query (nng_query_lds, csrc/nnd_grid.hip)
against the oracle, next to the L2 query (nng_query), which stays the default
(the LDS walk measured slower, DESIGN 6 round 8, and runs only when forced).

Bar: bit-exact (distances as raw f32 bits, indices exactly), as in
test_nnd_gpu.py.  PCR_NND_QUERY=lds is strict -- it is an error where the
grid does not fit LDS -- so a forced call that returns proves the LDS kernel
served it; =l2 and =auto run nng_query."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

QUERIES = ["lds", "l2"]


def _gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _forward(x1, x2):
    from pointcloudregistration_amd import nndistance as nd
    d1, d2, i1, i2 = nd.nnd_with_index(_gpu(x1), _gpu(x2))
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in (d1, d2, i1, i2)]


def assert_bitexact(got, exp, what):
    """Bit-exact for every non-NaN float, exact NaN positions, exact ints."""
    assert got.shape == exp.shape, what
    if got.dtype == np.float32:
        gn, en = np.isnan(got), np.isnan(exp)
        assert np.array_equal(gn, en), f"{what}: NaN positions differ ({(gn != en).sum()})"
        bad = (got.view(np.uint32) != exp.view(np.uint32)) & ~gn
        assert not bad.any(), f"{what}: {bad.sum()} of {bad.size} values differ"
    else:
        bad = got != exp
        assert not bad.any(), f"{what}: {bad.sum()} of {bad.size} entries differ"


def _check(oracle, monkeypatch, x1, x2, what, queries=QUERIES):
    """Every query mode against one oracle result."""
    monkeypatch.setenv("PCR_NND_ALGO", "grid")
    with np.errstate(invalid="ignore", over="ignore"):
        exp = oracle.nnd_forward(x1, x2)
        for q in queries:
            monkeypatch.setenv("PCR_NND_QUERY", q)
            got = _forward(x1, x2)
            for k, g, e in zip(("d1", "d2", "i1", "i2"), got, exp):
                assert_bitexact(g, e, f"{what}/{q}/{k}")


def _uniform(rng, b, n, m):
    x1 = (rng.random((b, n, 3), dtype=np.float32) * 2 - 1).astype(np.float32)
    x2 = (rng.random((b, m, 3), dtype=np.float32) * 2 - 1).astype(np.float32)
    return x1, x2


def _adversarial(kind, rng):
    """The generators of test_nnd_gpu.py."""
    if kind == "outliers":       # far queries: rings never certify -> per-query full scan
        x1 = rng.random((2, 1500, 3), dtype=np.float32)
        x1[:, ::50] += np.float32(100.0)
        x2 = rng.random((2, 1400, 3), dtype=np.float32)
    elif kind == "planar":       # zero-thickness box
        x1 = rng.random((1, 2000, 3), dtype=np.float32)
        x1[..., 2] = 0.5
        x2 = rng.random((1, 2100, 3), dtype=np.float32)
        x2[..., 2] = 0.5
    elif kind == "identical":    # every point the same: all distances tie
        x1 = np.full((1, 1200, 3), 0.25, np.float32)
        x2 = np.full((1, 1300, 3), 0.25, np.float32)
    elif kind == "quantised":    # many exact ties
        x1 = (rng.integers(0, 8, (2, 2048, 3)) / 8).astype(np.float32)
        x2 = (rng.integers(0, 8, (2, 2048, 3)) / 8).astype(np.float32)
    elif kind == "huge_offset":
        x1 = (rng.random((1, 1500, 3)) * 10 + 3e6).astype(np.float32)
        x2 = (rng.random((1, 1600, 3)) * 10 + 3e6).astype(np.float32)
    elif kind == "inf":          # non-finite: the reference loop (seed rule) answers
        x1 = rng.random((2, 1100, 3), dtype=np.float32)
        x2 = rng.random((2, 1200, 3), dtype=np.float32)
        x2[1, 0, 1] = np.inf
        x1[0, 5, 0] = -np.inf
    else:                        # "nan"
        x1 = rng.random((1, 1100, 3), dtype=np.float32)
        x2 = rng.random((1, 1200, 3), dtype=np.float32)
        x2[0, 0, 2] = np.nan
        x1[0, 9, 1] = np.nan
    return x1, x2


@pytest.mark.parametrize("b,n,m", [
    (3, 1027, 1500),    # n != m, neither a multiple of the 64-query chunk
    (2, 1000, 1024),    # nmax = 1024: S = 1024, the last size before the table doubles
    (2, 1025, 1000),    # nmax = 1025: S = 2048
    (2, 2000, 2000),    # K = 8 workgroups share each cloud's chunks
    (1, 8192, 8192),    # the C4 cloud, the largest shape that fits LDS
    (200, 1024, 1024),  # K = 1, more workgroups than CUs
])
def test_lds_query_bitexact_vs_oracle(oracle, monkeypatch, b, n, m):
    x1, x2 = _uniform(np.random.default_rng(b * 7 + n), b, n, m)
    _check(oracle, monkeypatch, x1, x2, f"{b}x{n}x{m}")


@pytest.mark.parametrize("kind", ["outliers", "planar", "identical", "quantised",
                                  "huge_offset", "inf", "nan"])
def test_lds_query_adversarial_vs_oracle(oracle, monkeypatch, kind):
    """Where certification is hard: the fallback scan over the LDS points, ties,
    and the clouds the reference loop answers (no grid is staged for them)."""
    x1, x2 = _adversarial(kind, np.random.default_rng(len(kind)))
    _check(oracle, monkeypatch, x1, x2, kind)


def test_lds_query_mixed_batch_vs_oracle(oracle, monkeypatch):
    """70 clouds holding every hard kind at once: reference-loop workgroups (a
    NaN and an Inf pair) run beside workgroups that stage a grid."""
    rng = np.random.default_rng(64)
    B, n, m = 70, 1100, 1200
    x1 = rng.random((B, n, 3), dtype=np.float32)
    x2 = rng.random((B, m, 3), dtype=np.float32)
    x1[0, ::50] += np.float32(100.0)                        # outliers
    x1[1, :, 2] = 0.5
    x2[1, :, 2] = 0.5                                       # planar
    x1[2] = 0.25
    x2[2] = 0.25                                            # identical
    x1[3] = (rng.integers(0, 8, (n, 3)) / 8).astype(np.float32)
    x2[3] = (rng.integers(0, 8, (m, 3)) / 8).astype(np.float32)   # quantised ties
    x2[4, 0, 2] = np.nan
    x1[5, 7, 0] = np.inf                                    # the reference loop
    _check(oracle, monkeypatch, x1, x2, "mixed")


def test_grid_too_large_for_lds_falls_back_or_raises(oracle, monkeypatch):
    """9000 candidates need 16384 slots: 176,770 B, more than a workgroup's LDS.
    auto answers through the L2 query, bit-exact; lds is an error that names
    the hook."""
    from pointcloudregistration_amd import _lib
    x1, x2 = _uniform(np.random.default_rng(9), 1, 1100, 9000)
    _check(oracle, monkeypatch, x1, x2, "1x1100x9000", queries=["auto"])
    monkeypatch.setenv("PCR_NND_QUERY", "lds")
    with pytest.raises(_lib.PcrError, match="PCR_NND_QUERY=lds"):
        _forward(x1, x2)
    monkeypatch.setenv("PCR_NND_QUERY", "sideways")
    with pytest.raises(_lib.PcrError, match="PCR_NND_QUERY=sideways"):
        _forward(x1, x2)


def test_pipeline_step_equal_under_both_queries(monkeypatch):
    """pcr_pipeline_step's Chamfer (the fused-transform entry,
    nnd_forward_grid_xf) under the LDS and the L2 query: the aligned clouds,
    distances, indices and records bit for bit."""
    from pointcloudregistration_amd import synth
    from pointcloudregistration_amd.pipeline import PairPipeline, default_params
    monkeypatch.setenv("PCR_NND_ALGO", "grid")
    b = synth.make_batch(2, n=1024, m=1024, d=32, base_seed=1000, feat_noise=1.0)
    out = {}
    for q in QUERIES:
        monkeypatch.setenv("PCR_NND_QUERY", q)
        pipe = PairPipeline(b.src, b.tgt, b.src_feat, b.tgt_feat, default_params(seed=0),
                            pair_ids=np.arange(2, dtype=np.int32))
        pipe.run()
        torch.cuda.synchronize()
        out[q] = [t.cpu().numpy() for t in (pipe.aligned, pipe.d1, pipe.d2, pipe.i1, pipe.i2, pipe.records())]
    for name, got, want in zip(("aligned", "d1", "d2", "i1", "i2", "records"), out["lds"], out["l2"]):
        assert got.shape == want.shape and got.tobytes() == want.tobytes(), name
    assert np.isfinite(out["lds"][1]).all() and (out["lds"][3] >= 0).all()
