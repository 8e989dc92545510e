"""GPU: pcr_unary_forward through pointcloudregistration_amd.ngenet (unary_forward,
norm_act) against the f64 restatement (tests/unary_ref.py, itself pinned to the
reference's blocks by test_unary_cpu.py).  Every stage is checked within its
derived bound from the call's own previous stage: y from the inputs, the
statistics from the call's y, out from the call's y.  Then what the contract
promises bit for bit: two calls alike, y and stats unchanged by the residual
and the activation, out without norm equal to y + bias; the gather's pad,
negative and repeated indices; a constant channel; the call without a weight;
and the memory the call takes."""
import functools

import numpy as np
import pytest
import torch

import unary_ref as ur

pytestmark = pytest.mark.gpu

ROWS = (2, 63, 64, 65, 129, 1093)       # 1093 = 17 tiles + 5 rows: the 16 runs are uneven
WIDTHS = ((1, 0, 1), (3, 0, 34), (129, 256, 64), (258, 512, 129), (64, 128, 34), (2048, 0, 32), (32, 0, 1024))


@functools.lru_cache(maxsize=None)
def inputs(n, c0, c1, cout, gather="none"):
    """Seeded inputs of one shape as numpy (shared, never modified).  gather: "none"; "up" (a coarser
    x0 of n // 3 + 1 rows, so indices repeat); "pads" (the same with the pad index m0, a negative
    index and an index far outside mixed in)."""
    rng = np.random.default_rng((n, c0, c1, cout, len(gather)))
    m0 = n if gather == "none" else n // 3 + 1
    d = {"x0": rng.standard_normal((m0, c0)).astype(np.float32),
         "x1": rng.standard_normal((n, c1)).astype(np.float32) if c1 else None,
         "w": (rng.standard_normal((cout, c0 + c1)) / np.sqrt(c0 + c1)).astype(np.float32),
         "bias": rng.standard_normal(cout).astype(np.float32),
         "res": rng.standard_normal((n, cout)).astype(np.float32), "g": None}
    if gather != "none":
        g = rng.integers(0, m0, n)
        if gather == "pads":
            g[rng.random(n) < 0.2] = m0
            g[0], g[-1] = -1, m0
            if n > 4:
                g[2], g[3] = -2 ** 31, 2 ** 31 - 1
        d["g"] = g.astype(np.int64)
    return d


def cuda(a):
    return None if a is None else torch.from_numpy(a).cuda()


def run(d, *, weight=True, norm=True, bias=False, res=False, act=True, slope=0.1, want=("y", "stats")):
    from pointcloudregistration_amd import ngenet
    if not norm:
        want = tuple(k for k in want if k != "stats")
    kw = dict(gather=cuda(d["g"]), x1=cuda(d["x1"]), bias=cuda(d["bias"]) if bias else None, norm=norm, slope=slope,
              act=act, residual=cuda(d["res"]) if res else None, want=want)
    with torch.no_grad():
        got = ngenet.unary_forward(cuda(d["x0"]), cuda(d["w"]), **kw) if weight else \
            ngenet.norm_act(cuda(d["x0"]), **kw)
    got = got if isinstance(got, tuple) else (got,)
    torch.cuda.synchronize()
    return dict(zip(("out",) + want, (t.cpu().numpy() for t in got)))


def check_stages(d, got, tag, *, weight=True, norm=True, bias=False, res=False, act=True, slope=0.1):
    """Each stage within its bound, taken from the call's own previous stage."""
    y_ref, e_y = ur.product(d["w"] if weight else None, d["x0"], d["g"], d["x1"])
    r_y = ur.ratio(got["y"], y_ref, e_y)
    y = got["y"]
    r_m = r_v = 0.0
    if norm:
        mean, var = ur.moments(y)
        e_mean, e_var = ur.moments_bound(y, 0.0)
        r_m = ur.ratio(got["stats"][:, 0], mean, e_mean)
        r_v = ur.ratio(got["stats"][:, 1], var, e_var)
    out_ref, e_out = ur.finish(y, 0.0, d["bias"] if bias else None, norm, 1e-5, slope, act, d["res"] if res else None)
    r_o = ur.ratio(got["out"], out_ref, e_out)
    print(f"{tag}: err / bound  y {r_y:.4f}  mean {r_m:.4f}  var {r_v:.4f}  out {r_o:.4f}")
    assert got["out"].shape == y_ref.shape and got["out"].dtype == np.float32
    assert r_y <= 1 and r_m <= 1 and r_v <= 1 and r_o <= 1, (tag, r_y, r_m, r_v, r_o)


@pytest.mark.parametrize("n", ROWS)
def test_rows_within_bound(n):
    """Every row count through the decoder's shape (a concat, cout no multiple of 32), norm, residual
    and activation on."""
    d = inputs(n, 64, 128, 34)
    check_stages(d, run(d, res=True), f"n={n}", res=True)


@pytest.mark.parametrize("c0,c1,cout", WIDTHS)
def test_widths_within_bound(c0, c1, cout):
    """Every width at n = 129 (two tiles and a row), through an up-sampling gather."""
    d = inputs(129, c0, c1, cout, "up")
    check_stages(d, run(d, res=True), f"{c0}+{c1}->{cout}", res=True)


def test_one_row_without_norm():
    d = inputs(1, 64, 128, 34)
    got = run(d, norm=False, bias=True, res=True)
    check_stages(d, got, "n=1", norm=False, bias=True, res=True)
    from pointcloudregistration_amd import ngenet
    with pytest.raises(ValueError, match="two rows"):
        ngenet.unary_forward(cuda(d["x0"]), cuda(d["w"]), x1=cuda(d["x1"]))


@pytest.mark.parametrize("c0,c1,cout", ((129, 256, 64), (3, 0, 34)))
def test_gather_pads_negative_and_repeats(c0, c1, cout):
    """A pad index m0, a negative one and the int32 extremes read a row of zeros; repeats read the
    same row.  The y rows of padded indices equal W [0 | x1[i]] within the bound like any other, and
    with c1 = 0 they are exactly +0."""
    d = inputs(129, c0, c1, cout, "pads")
    got = run(d)
    check_stages(d, got, f"pads {c0}+{c1}")
    bad = (d["g"] < 0) | (d["g"] >= d["x0"].shape[0])
    assert bad.sum() >= 4
    if c1 == 0:
        assert not got["y"][bad].any()
    first = {}
    for i, g in enumerate(d["g"]):
        if not bad[i] and c1 == 0:
            assert np.array_equal(got["y"][i], got["y"][first.setdefault(int(g), i)])


def test_constant_channel_has_zero_variance():
    d = dict(inputs(129, 64, 128, 34))
    w = d["w"].copy()
    w[5] = 0.0                      # y[:, 5] = 0 for every row
    x = np.ones((129, 4), np.float32)
    d["w"] = w
    got = run(d)
    check_stages(d, got, "zero channel")
    assert got["stats"][5, 0] == 0 and got["stats"][5, 1] == 0 and not got["out"][:, 5].any()
    # a non-zero constant: x = 1, one weight row -> every y equal, var clamps at >= 0, out = b + y a ~ 0
    dc = {"x0": x, "x1": None, "g": None, "w": np.full((3, 4), 0.3, np.float32), "bias": None, "res": None}
    got = run(dc)
    assert (got["stats"][:, 1] >= 0).all() and (got["stats"][:, 1] < 1e-12).all()
    assert np.abs(got["out"]).max() < 1e-3
    check_stages(dc, got, "constant channel")


@pytest.mark.parametrize("n,c0,c1", ((65, 34, 0), (1093, 129, 130), (129, 5, 300)))
def test_without_weight(n, c0, c1):
    """w = NULL: BatchNormBlock on an existing tensor (and on a gathered, concatenated one)."""
    d = inputs(n, c0, c1, c0 + c1, "pads" if c1 else "none")
    got = run(d, weight=False, res=True)
    check_stages(d, got, f"no weight n={n}", weight=False, res=True)
    assert np.array_equal(got["y"], ur.operand(d["x0"], d["g"], d["x1"]).astype(np.float32))
    got = run(d, weight=False, norm=False, bias=True, act=False, want=())
    assert np.array_equal(got["out"], ur.operand(d["x0"], d["g"], d["x1"]).astype(np.float32) + d["bias"])


@pytest.mark.parametrize("shape", ((1093, 129, 256, 64), (129, 258, 512, 129)))
def test_bit_identities(shape):
    d = inputs(*shape, "up")
    a = run(d, res=True)
    b = run(d, res=True)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), f"two calls differ in {k}"
    plain = run(d, res=False, act=False)
    assert plain["y"].tobytes() == a["y"].tobytes() and plain["stats"].tobytes() == a["stats"].tobytes(), \
        "y / stats must not depend on res / act"
    assert plain["out"].tobytes() != a["out"].tobytes()
    nb = run(d, norm=False, bias=True, act=False, want=("y",))
    assert nb["y"].tobytes() == a["y"].tobytes()
    assert nb["out"].tobytes() == (nb["y"] + d["bias"]).tobytes(), "out without norm must be y + bias bit for bit"
    nn = run(d, norm=False, act=False, want=("y",))
    assert nn["out"].tobytes() == nn["y"].tobytes()


def test_strided_operands_are_taken_in_place():
    """Column slices of wider tensors (row stride above the width) give the bytes of their copies."""
    d = inputs(129, 64, 128, 34)
    from pointcloudregistration_amd import ngenet
    wide0 = torch.zeros(129, 100).cuda()
    wide1 = torch.zeros(129, 200).cuda()
    wide0[:, 7:71] = cuda(d["x0"])
    wide1[:, 3:131] = cuda(d["x1"])
    with torch.no_grad():
        a = ngenet.unary_forward(wide0[:, 7:71], cuda(d["w"]), x1=wide1[:, 3:131])
        b = ngenet.unary_forward(cuda(d["x0"]), cuda(d["w"]), x1=cuda(d["x1"]))
    assert torch.equal(a, b)


def test_memory_is_the_output_and_the_scratch():
    """At n = 4096, (258, 512, 129) the call allocates out and its scratch (and the allocator's
    rounding, allowed for as in test_kpconv_conv_gpu): nothing of the operand's size (n (c0 + c1)
    floats = 6 times out)."""
    from pointcloudregistration_amd import _lib, ngenet
    n, c0, c1, cout = 4096, 258, 512, 129
    g = torch.Generator().manual_seed(5)
    x0 = torch.randn(n // 4, c0, generator=g).cuda()
    x1 = torch.randn(n, c1, generator=g).cuda()
    w = (torch.randn(cout, c0 + c1, generator=g) / (c0 + c1) ** 0.5).cuda()
    idx = torch.randint(0, n // 4, (n,), generator=g, dtype=torch.int32).cuda()
    with torch.no_grad():
        ngenet.unary_forward(x0[:64], w, gather=idx[:64] % 64, x1=x1[:64])   # library load, first launches
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.max_memory_allocated()
        out = ngenet.unary_forward(x0, w, gather=idx, x1=x1)
        torch.cuda.synchronize()
        grown = torch.cuda.max_memory_allocated() - before
    out_bytes = n * cout * 4
    scratch = _lib.load().pcr_unary_scratch_bytes(n, cout)
    assert scratch == (2 * cout * 4 + 15) // 16 * 16 + 2 * (n // 64) * cout * 8   # a | b, then the partials
    allowed = out_bytes + scratch + (1 << 20)
    print(f"memory: grown {grown}, out {out_bytes}, scratch {scratch}, operand {n * (c0 + c1) * 4}")
    assert grown <= allowed, (grown, allowed)
    assert n * (c0 + c1) * 4 > 5.9 * out_bytes
    assert torch.isfinite(out).all()


def test_error_paths():
    from pointcloudregistration_amd import ngenet
    d = inputs(65, 64, 128, 34)
    x0, x1, w = cuda(d["x0"]), cuda(d["x1"]), cuda(d["w"])
    with torch.no_grad():
        assert ngenet.unary_forward(x0, w, x1=x1).shape == (65, 34)
        assert ngenet.unary_forward(x0[:0], w, x1=x1[:0]).shape == (0, 34)
        with pytest.raises(ValueError, match="CUDA"):
            ngenet.unary_forward(x0.cpu(), w, x1=x1)
        with pytest.raises(ValueError, match="float32"):
            ngenet.unary_forward(x0.double(), w, x1=x1)
        with pytest.raises(ValueError, match="c0 \\+ c1"):
            ngenet.unary_forward(x0, w)
        with pytest.raises(ValueError, match="rows"):
            ngenet.unary_forward(x0, w, x1=x1[:-1])
        with pytest.raises(ValueError, match="bias together with norm"):
            ngenet.unary_forward(x0, w, x1=x1, bias=cuda(d["bias"]))
        with pytest.raises(ValueError, match="integer"):
            ngenet.unary_forward(x0, w, x1=x1, gather=torch.zeros(65).cuda())
        with pytest.raises(ValueError, match="residual"):
            ngenet.unary_forward(x0, w, x1=x1, residual=x1)
        with pytest.raises(ValueError, match="slope"):
            ngenet.unary_forward(x0, w, x1=x1, slope=1.5)
        with pytest.raises(ValueError, match="stats without norm"):
            ngenet.unary_forward(x0, w, x1=x1, norm=False, want=("stats",))
        with pytest.raises(ValueError, match="above 2048"):
            ngenet.norm_act(torch.zeros(4, 2049).cuda())
    with pytest.raises(RuntimeError, match="forward-only"):
        ngenet.unary_forward(x0, w.clone().requires_grad_(True), x1=x1)
