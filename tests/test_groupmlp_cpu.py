"""pcr_edge_conv / pcr_group_mlp without a GPU: the golden (what the reference's
own modules returned) against the f64 restatement and its derived bounds
(tests/groupmlp_ref.py), the two identities the kernels rest on, the scratch
formulas, argument validation and the ABI surface."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import groupmlp_cases as cases  # noqa: E402
import groupmlp_ref as ref  # noqa: E402
import knn_graph_ref as kr  # noqa: E402

from pointcloudregistration_amd import _lib  # noqa: E402

GOLDEN = np.load(os.path.join(HERE, "golden", "groupmlp_golden.npz"))


def test_golden_holds_results_only_and_is_small():
    want = {f"gcn/{n}/{k}" for n in cases.GCN_CASES for k in ("feats1", "feats2", "out")} | \
        {f"mlp/{n}/out" for n in cases.MLP_CASES}
    assert set(GOLDEN.files) == want
    assert os.path.getsize(os.path.join(HERE, "golden", "groupmlp_golden.npz")) < 512 * 1024


@pytest.mark.parametrize("name", list(cases.GCN_CASES))
def test_gcn_golden_within_bound(name):
    c = cases.gcn_case(name)
    idx, _ = kr.knn_graph(np.ascontiguousarray(c["coords"].transpose(0, 2, 1)), c["k"])
    f1, f2, out = (GOLDEN[f"gcn/{name}/{k}"] for k in ("feats1", "feats2", "out"))
    b, ch, n = c["feats"].shape
    assert f1.shape == (b, ch, n) and f2.shape == (b, 2 * ch, n) and out.shape == (b, ch, n)
    for i in range(b):
        f0 = c["feats"][i].T
        # every element, none excluded; each stage from the reference's own previous one
        w1, e1 = ref.edge_conv(c["conv1"], f0, idx[i], cases.EPS, cases.GCN_SLOPE)
        assert ref.ratio(f1[i].T, w1, e1) <= 1.0
        w2, e2 = ref.edge_conv(c["conv2"], f1[i].T, idx[i], cases.EPS, cases.GCN_SLOPE)
        assert ref.ratio(f2[i].T, w2, e2) <= 1.0
        # conv3 (torch's on both sides of fuse()): a layer and an instance norm over the points
        h = np.concatenate([f0, f1[i].T, f2[i].T], 1)
        y3, e3 = ref.layer(c["conv3"], h)
        w3, e3 = ref.norm_act(y3, e3, None, None, cases.EPS, cases.GCN_SLOPE)
        assert ref.ratio(out[i].T, w3, e3) <= 1.0
        # the reference's form of the edge conv is the kernel's, in f64
        r, q, _, _ = ref.edge_rq(c["conv1"], f0)
        y, _ = ref.edge_y(r, q, idx[i])
        yr = ref.edge_y_reference(c["conv1"], f0, idx[i])
        assert np.abs(y - yr).max() <= 1e-12 * np.abs(yr).max()


@pytest.mark.parametrize("name", list(cases.MLP_CASES))
def test_mlp_golden_within_bound(name):
    c = cases.mlp_case(name)
    kind, b, n, k, _, widths = cases.MLP_CASES[name]
    out = GOLDEN[f"mlp/{name}/out"]
    assert out.shape == (b, widths[-1], n) and c["x"].shape == (b, n, k, 6 if kind == "rop6" else 10)
    if kind != "ppf":   # the affine has every sign
        assert all((g < 0).any() and (g == 0).any() and (g > 0).any() for g in c["gammas"])
    for i in range(b):
        want, bound, _ = ref.group_mlp(c["x"][i], c["weights"], c["gammas"], c["betas"], cases.EPS, 0.0,
                                       1 if c["norm"] == "instance" else 32)
        assert ref.ratio(out[i].T, want, bound) <= 1.0


def test_max_commutes_with_norm_and_activation():
    """max_k act(y a + b) = act(max_k y a + b) for a >= 0 and act(min_k y a + b) for a < 0, bit for
    bit: every operation is monotone, rounding included (f64 here as f32 on the device)."""
    rng = np.random.default_rng(3)
    y = rng.standard_normal((50, 17, 96))
    y[:, 3:9] = y[:, 3:4]                       # repeated neighbours, as a padded group has
    a = rng.standard_normal(96)
    a[::6] = 0.0
    b = rng.standard_normal(96)
    for slope in (0.0, 0.2, 1.0):
        direct = ref.act(y * a + b, slope).max(1)
        pick = np.where(a >= 0, y.max(1), y.min(1))
        assert (direct == ref.act(pick * a + b, slope)).all()
    # and through the restatement: the pooled bound is the largest member bound
    h, e = ref.norm_act(y.reshape(50 * 17, 96), 0.0, a, b, 1e-5, 0.0, 32)
    out, bound = ref.pool(h.reshape(50, 17, 96), e.reshape(50, 17, 96))
    assert (out == h.reshape(50, 17, 96).max(1)).all() and (bound <= e.max()).all()


def test_edge_conv_is_two_per_point_products():
    rng = np.random.default_rng(4)
    f = rng.standard_normal((40, 32)).astype(np.float32)
    w = rng.standard_normal((64, 64)).astype(np.float32)
    idx = rng.integers(0, 40, (40, 10))
    r, q, e_r, e_q = ref.edge_rq(w, f)
    y, e = ref.edge_y(r, q, idx, e_r, e_q)
    yr = ref.edge_y_reference(w, f, idx)
    assert y.shape == (40, 10, 64) and np.abs(y - yr).max() <= 1e-12 * np.abs(yr).max()
    # an f32 evaluation in the reference's form lies within the derived bound
    g = np.concatenate([np.repeat(f[:, None], 10, 1), f[idx] - f[:, None]], -1)
    y32 = (g.reshape(400, 64) @ w.T).astype(np.float32).reshape(40, 10, 64)
    assert ref.ratio(y32, y, e) <= 1.0


def test_statistics_bounds_cover_an_f32_rounding_of_the_values():
    rng = np.random.default_rng(5)
    y = rng.standard_normal((300, 64)) * 3 + 1
    e = np.abs(y) * ref.U
    y32 = y.astype(np.float32)
    for group in (1, 32):
        mean, var = ref.moments(y, group)
        m32, v32 = ref.moments(y32, group)
        e_mean, e_var = ref.moments_bound(y, e, group)
        assert (np.abs(m32 - mean) <= e_mean).all() and (np.abs(v32 - var) <= e_var).all()


def _tiles(n, k):
    return -(-n // (64 // k)) if k <= 64 else n * -(-k // 64)


def test_scratch_formulas():
    lib = _lib.load()
    # edge conv: 4 b n co + 2 b co floats, 2 b ceil(n / 8) co doubles; no term in kk
    for b, n, c, co in ((1, 2048, 256, 256), (3, 129, 32, 512)):
        want = 4 * (4 * b * n * co + 2 * b * co) + 8 * 2 * b * -(-n // 8) * co
        got = {kk: lib.pcr_edge_conv_scratch_bytes(b, n, kk, c, co) for kk in (1, 10, 63)}
        assert got[1] == got[10] == got[63] == want
    # grouped MLP: the terms in K are the documented ones -- the tiles' partials and, above 64, the slots
    for b, n, widths in ((1, 2048, (256, 512, 256)), (2, 129, (32, 64, 0)), (2, 70, (128, 0, 0))):
        nl = sum(1 for c in widths if c)
        cl, cmax = widths[nl - 1], max(widths)
        got = {}
        for k in (1, 7, 64, 128):
            got[k] = lib.pcr_group_mlp_scratch_bytes(b, n, k, nl, *widths)
            slots = n * -(-k // 64)
            assert got[k] == 4 * (2 * b * sum(widths) + 2 * b * slots * cl) + 8 * 2 * b * _tiles(n, k) * cmax
        part = {k: 16 * b * _tiles(n, k) * cmax for k in got}
        assert got[1] - part[1] == got[64] - part[64]
        # one 64th of a materialised activation (and a 4096th at K = 1)
        assert part[64] == n * 64 * cmax * b * 4 // 16
    # a call's scratch at the real shape is far below ONE activation
    assert lib.pcr_group_mlp_scratch_bytes(1, 2048, 64, 3, 256, 512, 256) < 2048 * 64 * 512 * 4 // 10


def _err(lib):
    return lib.pcr_last_error().decode()


def test_argument_errors_without_gpu():
    lib = _lib.load()
    for args, text in (((1, 1, 10, 32, 32), "n=1"), ((1, 64, 0, 32, 32), "kk=0"), ((1, 64, 64, 32, 32), "kk=64"),
                       ((1, 64, 10, 48, 32), "multiples of 32"), ((1, 64, 10, 32, 544), "multiples of 32"),
                       ((-1, 64, 10, 32, 32), "b=-1")):
        assert lib.pcr_edge_conv_scratch_bytes(*args) == -1 and text in _err(lib), args
    for args, text in (((1, 64, 0, 3, 32, 64, 32), "K=0"), ((1, 64, 129, 3, 32, 64, 32), "K=129"),
                       ((1, 64, 16, 4, 32, 64, 32), "layers=4"), ((1, 64, 16, 0, 32, 64, 32), "layers=0"),
                       ((1, 64, 16, 2, 32, 40, 0), "width 40 of layer 2"), ((1, 1, 16, 1, 32, 0, 0), "n=1")):
        assert lib.pcr_group_mlp_scratch_bytes(*args) == -1 and text in _err(lib), args
    assert lib.pcr_group_mlp_scratch_bytes(1, 64, 16, 1, 32, 7, 9) > 0       # widths past `layers` are not read
    one = ctypes.c_void_p(256)   # non-null: never dereferenced, validation comes first

    def edge(feats=one, idx=one, w=one, out=one, scratch=one, n=64, kk=10, c=32, co=32, eps=1e-5):
        return lib.pcr_edge_conv(feats, 64 * 32, 32, 1, idx, 1, n, kk, c, co, w, eps, 0.2, 0, out, None, None, scratch,
                                 None)
    for name in ("feats", "idx", "w", "out", "scratch"):
        assert edge(**{name: None}) == -1 and "null pointer" in _err(lib), name
    assert edge(n=1) == -1 and "n=1" in _err(lib)
    assert edge(eps=-1.0) == -1 and "eps" in _err(lib)
    assert edge(scratch=ctypes.c_void_p(260)) == -1 and "16-byte aligned" in _err(lib)

    def mlp(x=one, out=one, scratch=one, net=True, layers=3, group=32, cin=10, k=16, w2=256, eps=1e-5):
        s = _lib.GroupMlpNet()
        s.layers = layers
        for i, c in enumerate((32, 64, 32)):
            s.width[i] = c
            s.w[i] = 256
        s.w[1] = w2
        return lib.pcr_group_mlp(x, 1, 64, k, cin, ctypes.byref(s) if net else None, group, eps, 0.0, 1, out, scratch,
                                 None)
    for name in ("x", "out", "scratch"):
        assert mlp(**{name: None}) == -1 and "null pointer" in _err(lib), name
    assert mlp(net=False) == -1 and "null net" in _err(lib)
    assert mlp(w2=None) == -1 and "null weight of layer 2" in _err(lib)
    assert mlp(group=16) == -1 and "group=16" in _err(lib)
    assert mlp(cin=17) == -1 and "cin=17" in _err(lib)
    assert mlp(k=200) == -1 and "K=200" in _err(lib)
    assert mlp(layers=0) == -1 and "layers=0" in _err(lib)
    assert mlp(scratch=ctypes.c_void_p(264)) == -1 and "16-byte aligned" in _err(lib)


def test_python_checks_without_gpu():
    torch = pytest.importorskip("torch")
    from pointcloudregistration_amd import groupmlp
    f, idx, w = torch.zeros(1, 8, 32), torch.zeros(1, 8, 3, dtype=torch.long), torch.zeros(32, 64)
    with pytest.raises(ValueError, match="CUDA"):
        groupmlp.edge_conv(f, idx, w)
    with pytest.raises(ValueError, match="CUDA"):
        groupmlp.group_mlp(torch.zeros(1, 8, 4, 6), [torch.zeros(32, 6)])
    with pytest.raises(RuntimeError, match="forward-only"):
        groupmlp.edge_conv(f, idx, w.clone().requires_grad_(True))
    with pytest.raises(RuntimeError, match="forward-only"):
        groupmlp.group_mlp(torch.zeros(1, 8, 4, 6), [torch.zeros(32, 6, requires_grad=True)])
    with pytest.raises(ValueError, match="one to three"):
        groupmlp.group_mlp(torch.zeros(1, 8, 4, 6), [])
    with pytest.raises(TypeError):
        groupmlp.edge_conv(np.zeros((1, 8, 32), np.float32), idx, w)
    # fuse() looks at structure only: it runs on CPU modules
    nn = torch.nn

    class GCN(nn.Module):
        def __init__(self, affine=False, bias=False):
            super().__init__()
            self.conv1 = nn.Sequential(nn.Conv2d(64, 32, 1, bias=bias), nn.InstanceNorm2d(32, affine=affine),
                                       nn.LeakyReLU(0.2))
            self.conv2 = nn.Sequential(nn.Conv2d(64, 64, 1, bias=False), nn.InstanceNorm2d(64), nn.LeakyReLU(0.2))
            self.conv3 = nn.Sequential(nn.Conv1d(128, 32, 1, bias=False), nn.InstanceNorm1d(32), nn.LeakyReLU(0.2))
            self.k = 10

    class Net(nn.Module):
        def __init__(self):
            super().__init__()
            self.a, self.b, self.c = GCN(), GCN(affine=True), GCN(bias=True)

    net, refused = Net(), []
    assert groupmlp.fuse(net, refused) == (1, 0, 0) and isinstance(net.a, groupmlp.GCN)
    assert [r[0] for r in refused] == ["b", "c"] and "affine" in refused[0][1] and "without bias" in refused[1][1]
    assert net.a.conv1 is not None and groupmlp.fuse(net) == (0, 0, 0)


def test_entry_points_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "pcr_api.h")).read()
    lib = _lib.load()

    def arity(name, ret):
        m = re.search(r"\b%s\s+%s\s*\(([^;]*)\);" % (ret, name), hdr)
        assert m, name
        return len(m.group(1).split(","))

    for s, n in (("pcr_edge_conv", 19), ("pcr_group_mlp", 13)):
        assert s in _lib.exported_symbols() and s in _lib.SIGNATURES and hasattr(lib, s)
        assert arity(s, "int") == n == len(_lib.SIGNATURES[s])
    for s, n in (("pcr_edge_conv_scratch_bytes", 5), ("pcr_group_mlp_scratch_bytes", 7)):
        assert s in _lib.exported_symbols() and hasattr(lib, s)
        assert arity(s, "int64_t") == n == len(getattr(lib, s).argtypes)
    ptr = ctypes.sizeof(ctypes.c_void_p)
    assert ctypes.sizeof(_lib.GroupMlpNet) == 16 + 15 * ptr
    assert re.search(r"typedef struct pcr_group_mlp_net \{\s*int32_t layers;", hdr)
    import pointcloudregistration_amd as pcr
    from pointcloudregistration_amd import groupmlp, grouping
    assert "groupmlp" in pcr.__all__ and pcr.groupmlp is groupmlp
    for name in ("edge_conv", "group_mlp", "GCN", "PPF", "LocalFeature", "fuse"):
        assert hasattr(groupmlp, name) and name in groupmlp.__all__
    assert "groupmlp" in grouping.__doc__
    src = open(os.path.join(ROOT, "pointcloudregistration_amd", "csrc", "Makefile")).read()
    assert " groupmlp.hip" in src
