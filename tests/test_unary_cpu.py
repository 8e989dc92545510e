"""CPU: the f64 restatement of pcr_unary_forward (tests/unary_ref.py) against the
reference's recorded outputs (tests/golden/unary_golden.npz, written by
make_golden_unary.py from the reference's own blocks): every UnaryBlock,
up-sample + cat + UnaryBlock, SimpleBlock and ResnetBottleneckBlock output within
the derived bound; teeth: a dropped last input channel or a last row left out of
the statistics exceeds it; the second-order constant of the product's bound at
2048 links in exact arithmetic; the C ABI's argument errors and scratch sizes,
the Python checks and fuse()'s structure, none of which needs a GPU."""
import ctypes
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import unary_cases as uc
import unary_ref as ur
from pointcloudregistration_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "unary_golden.npz"))


def _err(lib):
    return lib.pcr_last_error().decode()


def _tail_case(kind, name):
    """(w, x0, gather, x1, keyword arguments, golden) of a UNARY / UPCAT case."""
    if kind == "unary":
        n, cin, cout, use_bn, relu = uc.UNARY[name]
        c = uc.make_unary(name)
        args = (c["w"], c["x"], None, None)
    else:
        m0, n, c0, c1, cout, use_bn, relu = uc.UPCAT[name]
        c = uc.make_upcat(name)
        args = (c["w"], c["x0"], c["up"][:, 0], c["x1"])
    return args, dict(bias=c["bias"], norm=use_bn, eps=uc.EPS, slope=uc.SLOPE, act=relu), GOLD[f"{kind}/{name}"]


TAILS = [("unary", k) for k in uc.UNARY] + [("upcat", k) for k in uc.UPCAT]


@pytest.mark.parametrize("kind,name", TAILS)
def test_golden_within_bound(kind, name):
    args, kw, gold = _tail_case(kind, name)
    want, bound, _ = ur.unary(*args, **kw)
    r = ur.ratio(gold, want, bound)
    print(f"{kind}/{name}: max err / bound = {r:.4f}")
    assert gold.dtype == np.float32 and gold.shape == want.shape and r <= 1


@pytest.mark.parametrize("kind,name", TAILS)
def test_teeth_dropped_channel_and_row(kind, name):
    """A case that cannot see a dropped tail is a bad case: the restatement without the operand's last
    channel, and (with the norm) with the last row left out of the statistics, must miss the bound."""
    (w, x0, g, x1), kw, gold = _tail_case(kind, name)
    _, bound, y = ur.unary(w, x0, g, x1, **kw)
    rows = ur.operand(x0, g, x1)
    short, _, _ = ur.unary(w[:, :-1], rows[:, :-1], **kw)
    assert ur.ratio(gold, short, bound) > 1, "the last input channel is invisible"
    if kw["norm"]:
        mean, var = ur.moments(y[:-1])
        z = (y - mean) / np.sqrt(var + kw["eps"])
        less = np.where(z > 0, z, kw["slope"] * z) if kw["act"] else z
        assert ur.ratio(gold, less, bound) > 1, "the last row's part in the statistics is invisible"


@pytest.mark.parametrize("name", sorted(uc.BLOCKS))
def test_block_stages_within_bound(name):
    c = uc.make_block(name)
    conv_out = GOLD[f"block/{name}/conv_out"]
    has_in = f"block/{name}/conv_in" in GOLD.files
    conv_in = GOLD[f"block/{name}/conv_in"] if has_in else c["f"]
    st = ur.block_stages(uc.BLOCKS[name][0], c, conv_in, conv_out, uc.EPS, uc.SLOPE)
    assert has_in == (st["conv_in"] is not None)
    if has_in:
        assert ur.ratio(conv_in, *st["conv_in"]) <= 1
    assert ur.ratio(conv_out, *st["conv_out"]) <= 1
    r = ur.ratio(GOLD[f"block/{name}/out"], *st["out"])
    print(f"block/{name}: out err / bound = {r:.4f}")
    assert r <= 1


def test_layer_constant_holds_for_2048_links():
    """unary_ref's argument in exact arithmetic: g_n = n u / (1 - n u) <= (n + 1) u up to n = 2048 (and
    to 4095), so groupmlp_ref.layer's (n + 2) u covers the chain; and the gap to the next u is real."""
    u = Fraction(1, 2 ** 24)
    assert ur.U == float(u)
    for n in (512, 770, 2048, 4095):
        assert n * (n + 1) * u <= 1
        assert n * u / (1 - n * u) <= (n + 1) * u
        assert (1 + u) ** n - 1 <= (n + 1) * u
    assert 4096 * u / (1 - 4096 * u) > 4097 * u


def test_restatement_operand_and_stages():
    rng = np.random.default_rng(3)
    x0 = rng.standard_normal((5, 3)).astype(np.float32)
    x1 = rng.standard_normal((4, 2)).astype(np.float32)
    rows = ur.operand(x0, np.array([4, -1, 5, 4]), x1)
    assert rows.shape == (4, 5) and not rows[1, :3].any() and not rows[2, :3].any()
    assert np.array_equal(rows[0, :3], x0[4]) and np.array_equal(rows[3, :3], x0[4])
    assert np.array_equal(rows[:, 3:], x1)
    y, e = ur.product(None, x0)
    assert np.array_equal(y, x0) and not e.any()
    out, b = ur.finish(y, 0.0, norm=False, act=False)
    assert np.array_equal(out, y) and not b.any()
    res = rng.standard_normal((5, 3)).astype(np.float32)
    out, b = ur.finish(y, 0.0, bias=np.ones(3, np.float32), norm=False, slope=0.1, act=True, res=res)
    z = x0.astype(np.float64) + 1 + res
    assert np.allclose(out, np.where(z > 0, z, 0.1 * z)) and (b > 0).all() and (b < 1e-6).all()
    with pytest.raises(ValueError):
        ur.finish(y, 0.0, bias=np.ones(3), norm=True)


def test_argument_errors_without_gpu():
    lib = _lib.load()
    for args, text in (((-1, 8), "n=-1"), (((1 << 22) + 1, 8), "n=4194305"), ((64, 0), "cout=0"),
                       ((64, 1025), "cout=1025")):
        assert lib.pcr_unary_scratch_bytes(*args) == -1 and text in _err(lib), args
    assert lib.pcr_unary_scratch_bytes(0, 1) > 0
    # a | b, 16-byte aligned, then two doubles per (tile, channel)
    for n, cout in ((1, 1), (64, 34), (65, 34), (4096, 129), (1 << 22, 1024)):
        assert lib.pcr_unary_scratch_bytes(n, cout) == (8 * cout + 15) // 16 * 16 + 16 * ((n + 63) // 64) * cout
    one = 256   # non-null: never dereferenced, validation comes first

    def call(scratch=one, null_args=False, **kw):
        a = _lib.UnaryArgs()
        a.n, a.m0, a.c0, a.c1, a.cout = 64, 64, 32, 16, 8
        a.x0, a.x1, a.w, a.out = one, one, one, one
        a.ld0, a.ld1, a.norm, a.eps, a.act, a.slope = 32, 16, 1, 1e-5, 1, 0.1
        for k, v in kw.items():
            setattr(a, k, v)
        return lib.pcr_unary_forward(None if null_args else ctypes.byref(a), ctypes.c_void_p(scratch), None)

    assert call(null_args=True) == -1 and "null args" in _err(lib)
    for name in ("x0", "out"):
        assert call(**{name: None}) == -1 and "null pointer" in _err(lib), name
    assert call(scratch=None) == -1 and "null pointer" in _err(lib)
    assert call(scratch=260) == -1 and "16-byte aligned" in _err(lib)
    for kw, text in ((dict(n=1), "at least two rows"), (dict(bias=one), "bias together with norm"),
                     (dict(norm=0, stats=one), "stats without norm"), (dict(w=None), "w is null and cout=8"),
                     (dict(m0=63), "g0 is null and m0=63"), (dict(x1=None), "x1 is null and c1=16"),
                     (dict(c0=0), "c0=0"), (dict(c0=2040), "c0 + c1 <= 2048"), (dict(cout=1025), "cout=1025"),
                     (dict(eps=-1.0), "eps"), (dict(slope=1.5), "slope"), (dict(ld0=31), "row stride"),
                     (dict(n=-1), "n=-1"), (dict(m0=0, g0=one), "m0=0")):
        assert call(**kw) == -1 and text in _err(lib), (kw, _err(lib))
    assert call(n=0, m0=0) == 0            # no rows: PCR_OK without a launch
    assert call(n=0, x0=None, out=None, scratch=None) == 0


def test_entry_points_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "pcr_api.h")).read()
    lib = _lib.load()
    assert "pcr_unary_forward" in _lib.SIGNATURES and len(_lib.SIGNATURES["pcr_unary_forward"]) == 3
    for s in ("pcr_unary_forward", "pcr_unary_scratch_bytes"):
        assert s in _lib.exported_symbols() and hasattr(lib, s)
    assert re.search(r"int64_t\s+pcr_unary_scratch_bytes\(int32_t n, int32_t cout\);", hdr)
    assert re.search(r"int\s+pcr_unary_forward\(const pcr_unary_args \*a, void \*scratch, pcr_stream_t stream\);", hdr)
    fields = re.search(r"typedef struct pcr_unary_args \{(.*?)\} pcr_unary_args;", hdr, re.S).group(1)
    fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S)
    names = [n.strip(" *") for decl in fields.split(";") for n in re.sub(r"^\s*(const\s+)?\w+\s", "", decl).split(",")
             if n.strip()]
    assert names == [f[0] for f in _lib.UnaryArgs._fields_]
    ptr = ctypes.sizeof(ctypes.c_void_p)
    assert ptr != 8 or ctypes.sizeof(_lib.UnaryArgs) == 136   # 5 int32 (padded to 24), then 14 eight-byte slots
    import pointcloudregistration_amd as pcr
    from pointcloudregistration_amd import c2p, ngenet
    assert "ngenet" in pcr.__all__ and pcr.ngenet is ngenet
    for name in ("unary_forward", "norm_act", "Unary", "NearestUpsample", "Simple", "ResnetBottleneck", "fuse",
                 "forward"):
        assert hasattr(ngenet, name) and name in ngenet.__all__
    assert "describe" in c2p.__all__
    src = open(os.path.join(ROOT, "pointcloudregistration_amd", "csrc", "Makefile")).read()
    assert " unary.hip" in src and " norm_finalize.h" in src
    # the finalize rule is shared, not copied
    csrc = os.path.join(ROOT, "pointcloudregistration_amd", "csrc")
    for unit in ("groupmlp.hip", "unary.hip"):
        text = open(os.path.join(csrc, unit)).read()
        assert '#include "norm_finalize.h"' in text and "void norm_finalize(" not in text


def test_python_checks_without_gpu():
    torch = pytest.importorskip("torch")
    from pointcloudregistration_amd import ngenet
    x, w = torch.zeros(8, 4), torch.zeros(3, 4)
    with pytest.raises(ValueError, match="CUDA"):
        ngenet.unary_forward(x, w)
    with pytest.raises(ValueError, match="CUDA"):
        ngenet.norm_act(x)
    with pytest.raises(RuntimeError, match="forward-only"):
        ngenet.unary_forward(x, w.clone().requires_grad_(True))
    with pytest.raises(TypeError):
        ngenet.unary_forward(np.zeros((8, 4), np.float32), w)
    with pytest.raises(ValueError, match="needs a weight"):
        ngenet.unary_forward(x, None)


def test_modules_keys_and_fuse_structure():
    """State-dict keys and strict loads of the fresh modules; fuse() by class name and attribute
    shape on CPU modules: shared parameters, the four counts, zeros on the second call, both orders
    with kpconv.fuse."""
    torch = pytest.importorskip("torch")
    import unary_blocks as ub
    from pointcloudregistration_amd import kpconv, ngenet
    nn = torch.nn

    assert set(ngenet.Unary(5, 3, True, 0.02).state_dict()) == {"mlp.weight"}
    last = ngenet.Unary(5, 3, False, 0.02, relu=False)
    assert set(last.state_dict()) == {"mlp.weight", "bn.bias"} and not hasattr(last, "leaky_relu")
    ref = ub.UnaryBlock(5, 3, False, 0.02, relu=False)
    res = last.load_state_dict(ref.state_dict(), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    ngenet.Unary(5, 3, True, 0.02).load_state_dict(ub.UnaryBlock(5, 3, True, 0.02).state_dict(), strict=True)
    assert not ngenet.NearestUpsample(2).state_dict() and ngenet.NearestUpsample(2).layer_ind == 2

    class Net(nn.Module):
        def __init__(self):
            super().__init__()
            self.blocks = nn.ModuleList([ub.make_block(n)[0] for n in ("simple", "resnet_id", "resnet_strided_proj")])
            self.dec = nn.ModuleList([ub.NearestUpsampleBlock(0), ub.UnaryBlock(9, 4, True, 0.02),
                                      ub.UnaryBlock(4, 3, False, 0.02, relu=False)])
            self.odd = ub.UnaryBlock(4, 4, True, 0.02)
            self.odd.bn.batch_norm = nn.InstanceNorm1d(4, affine=True)
            self.lin = nn.Linear(3, 3)

    for order in ("ngenet first", "kpconv first"):
        net = Net().eval()
        keys = list(net.state_dict())
        params = {k: v for k, v in net.named_parameters()}
        if order == "kpconv first":
            assert kpconv.fuse(net) == (3, 2)
        refused = []
        # unaries: resnet_id has unary1 + unary2, resnet_strided_proj all three, the decoder two; `odd` is refused
        assert ngenet.fuse(net, refused) == (7, 1, 1, 2), order
        assert [r[0] for r in refused] == ["odd"] and "affine" in refused[0][1]
        assert ngenet.fuse(net) == (0, 0, 0, 0)
        if order == "ngenet first":
            assert kpconv.fuse(net) == (3, 2)
            assert kpconv.fuse(net) == (0, 0)
        assert isinstance(net.blocks[0], ngenet.Simple) and isinstance(net.blocks[1], ngenet.ResnetBottleneck)
        assert isinstance(net.blocks[2].unary_shortcut, ngenet.Unary) and isinstance(net.blocks[1].unary2, ngenet.Unary)
        assert isinstance(net.blocks[1].unary_shortcut, nn.Identity)
        assert isinstance(net.blocks[1].KPConv, kpconv.KPConv) and isinstance(net.blocks[2].max_pool, kpconv.MaxPool)
        assert isinstance(net.dec[0], ngenet.NearestUpsample) and isinstance(net.dec[2], ngenet.Unary)
        assert isinstance(net.odd, ub.UnaryBlock) and isinstance(net.lin, nn.Linear)
        assert list(net.state_dict()) == keys, "state-dict keys must survive the swap"
        after = {k: v for k, v in net.named_parameters()}
        assert after.keys() == params.keys() and all(after[k] is params[k] for k in params), \
            "parameters must be shared, not copied"
        net.load_state_dict(Net().state_dict(), strict=True)
