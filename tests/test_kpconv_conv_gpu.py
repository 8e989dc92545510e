"""GPU: the fused KPConv forward and the neighbour max-pool
(pointcloudregistration_amd.kpconv: kpconv_forward, neighbor_max, KPConv, fuse)
against the f64 restatement (tests/kpconv_conv_ref.py, itself pinned to the
reference's outputs by test_kpconv_conv_cpu.py): every output within the
derived bound, all-pad queries exactly zero, two calls bit-identical, int32 and
int64 indices and every pad value alike, the pool byte-equal to torch's gather
and max, the module and fuse(), the memory the call takes, and the error paths."""
import functools

import numpy as np
import pytest
import torch

import kpconv_conv_cases as kc
import kpconv_conv_ref as kr

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def case(name):
    """The case's inputs, the f64 restatement per influence and the CUDA tensors
    (computed once, shared, never modified)."""
    c = kc.make(name)
    want = {infl: kr.kpconv(c["q"], c["s"], c["f"], c["idx"], c["kp"], c["W"], c["extent"], infl)
            for infl in ("linear", "constant")}
    t = {k: torch.from_numpy(v).cuda() for k, v in c.items() if isinstance(v, np.ndarray)}
    return c, want, t


def run(t, c, infl="linear", idx=None):
    from pointcloudregistration_amd import kpconv
    with torch.no_grad():
        return kpconv.kpconv_forward(t["q"], t["s"], t["f"], t["idx"] if idx is None else idx, t["kp"], t["W"],
                                     c["extent"], infl)


@pytest.mark.parametrize("infl", ("linear", "constant"))
@pytest.mark.parametrize("name", sorted(kc.CASES))
def test_accuracy_within_bound(name, infl):
    c, want, t = case(name)
    ref, bound, allpad = want[infl]
    out = run(t, c, infl)
    assert out.dtype == torch.float32 and tuple(out.shape) == ref.shape
    got = out.cpu().numpy()
    err = np.abs(got.astype(np.float64) - ref)
    ratio = float((err[bound > 0] / bound[bound > 0]).max())
    print(f"{name}/{infl}: max err / bound = {ratio:.4f}")
    assert (err <= bound).all(), f"max err / bound = {ratio}"
    assert allpad.any() and not got[allpad].any(), "all-pad queries must be exactly 0"


@pytest.mark.parametrize("name", ("c32", "deep"))
def test_two_calls_are_bit_identical(name):
    c, _, t = case(name)
    assert torch.equal(run(t, c), run(t, c))


@pytest.mark.parametrize("name", ("first", "pads", "ragged"))
def test_index_widths_and_pad_values(name):
    c, _, t = case(name)
    m = c["s"].shape[0]
    base = run(t, c)
    assert torch.equal(run(t, c, idx=t["idx"].to(torch.int32)), base)
    for pad in (-1, m + 5):
        alt = torch.where(t["idx"] == m, torch.full_like(t["idx"], pad), t["idx"])
        assert torch.equal(run(t, c, idx=alt), base), pad
        assert torch.equal(run(t, c, idx=alt.to(torch.int32)), base), pad


def test_limits_of_the_tiling():
    """k = 256 with K = 16 (the neighbour table fills the LDS: the narrowest
    channel pass, five of them), C_out = 272 (a second block of output channels
    with a single 16-wide tile, split four ways over the kernel rows)."""
    from pointcloudregistration_amd import kpconv
    n, m, k, K, c_in, c_out = 20, 50, 256, 16, 80, 272
    rng = np.random.default_rng(11)
    s = rng.random((m, 3)).astype(np.float32)
    q = rng.random((n, 3)).astype(np.float32)
    idx = rng.integers(0, m, (n, k))
    idx[rng.random((n, k)) < 0.3] = m
    idx[3] = m
    f = rng.standard_normal((m, c_in)).astype(np.float32)
    kp = (0.3 * rng.standard_normal((K, 3))).astype(np.float32)
    W = (rng.standard_normal((K, c_in, c_out)) / np.sqrt(K * c_in)).astype(np.float32)
    ref, bound, allpad = kr.kpconv(q, s, f, idx, kp, W, 0.6)
    with torch.no_grad():
        got = kpconv.kpconv_forward(*(torch.from_numpy(a).cuda() for a in (q, s, f, idx, kp, W)), 0.6).cpu().numpy()
    assert (np.abs(got - ref) <= bound).all()
    assert allpad[3] and not got[3].any()


@pytest.mark.parametrize("n,c_out", ((2100, 64), (2100, 128), (4100, 32), (4100, 40)))
def test_output_block_plans(n, c_out):
    """The launch plan's other branches: the small cases all run 16 output
    channels per workgroup; these run 32 (two tiles, the kernel rows split in
    two), 64, and 256 with two tiles (split) and with three (one wave idle)."""
    from pointcloudregistration_amd import kpconv
    m, k, K, c_in = 200, 6, 15, 16
    rng = np.random.default_rng((n, c_out))
    s = rng.random((m, 3)).astype(np.float32)
    q = rng.random((n, 3)).astype(np.float32)
    idx = rng.integers(0, m + 20, (n, k))     # about a tenth are pads, of several values
    idx[-1] = m
    f = rng.standard_normal((m, c_in)).astype(np.float32)
    kp = (0.3 * rng.standard_normal((K, 3))).astype(np.float32)
    W = (rng.standard_normal((K, c_in, c_out)) / np.sqrt(K * c_in)).astype(np.float32)
    ref, bound, allpad = kr.kpconv(q, s, f, idx, kp, W, 0.6)
    with torch.no_grad():
        got = kpconv.kpconv_forward(*(torch.from_numpy(a).cuda() for a in (q, s, f, idx, kp, W)), 0.6).cpu().numpy()
    assert (np.abs(got - ref) <= bound).all()
    assert allpad[-1] and not got[allpad].any()


def torch_pool(feats, idx):
    m = feats.shape[0]
    padded = torch.cat([feats, torch.zeros_like(feats[:1])], 0)
    idx = torch.where((idx >= 0) & (idx < m), idx, torch.full_like(idx, m)).long()
    return padded[idx].max(dim=1)[0]


@pytest.mark.parametrize("name", sorted(kc.CASES))
def test_neighbor_max_is_byte_equal(name):
    from pointcloudregistration_amd import kpconv
    c, _, t = case(name)
    m = c["s"].shape[0]
    want = torch_pool(t["f"], t["idx"])
    assert want.cpu().numpy().tobytes() == kr.neighbor_max(c["f"], c["idx"]).tobytes()
    for idx in (t["idx"], t["idx"].to(torch.int32),
                torch.where(t["idx"] == m, torch.full_like(t["idx"], -1), t["idx"])):
        got = kpconv.neighbor_max(t["f"], idx)
        assert got.dtype == torch.float32 and torch.equal(got, want)


@pytest.mark.parametrize("C", (1, 130))
def test_neighbor_max_channel_widths(C):
    from pointcloudregistration_amd import kpconv
    c, _, t = case("ragged")
    m = c["s"].shape[0]
    g = torch.Generator().manual_seed(C)
    feats = torch.randn(m, C, generator=g).cuda()   # signed: a pad's 0 wins over an all-negative column set
    got = kpconv.neighbor_max(feats, t["idx"])
    assert torch.equal(got, torch_pool(feats, t["idx"]))


def test_module_loads_reference_state_dict():
    from pointcloudregistration_amd import kpconv
    c, _, t = case("ragged")
    (n, m, k, K, c_in, c_out), _r = kc.CASES["ragged"]
    mod = kpconv.KPConv(c_in, c_out, 0.35, torch.zeros(K, 3), c["extent"]).cuda().eval()
    assert set(mod.state_dict()) == {"weights", "kernel_points"}
    assert (mod.K, mod.KP_influence, mod.aggregation_mode, mod.radius) == (K, "linear", "sum", 0.35)
    assert not mod.kernel_points.requires_grad and mod.weights.requires_grad
    res = mod.load_state_dict({"weights": t["W"].cpu(), "kernel_points": t["kp"].cpu()}, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    with torch.no_grad():
        out = mod(t["q"], t["s"], t["f"], t["idx"])
    assert torch.equal(out, run(t, c))


class _RefShapedConv(torch.nn.Module):
    """A torch composite with the reference KPConv's attributes (blocks.py:73-128)."""

    def __init__(self, kp, W, extent):
        super().__init__()
        self.weights = torch.nn.Parameter(W.clone())
        self.kernel_points = torch.nn.Parameter(kp.clone(), requires_grad=False)
        self.K, self.KP_extent, self.KP_influence, self.aggregation_mode = kp.shape[0], extent, "linear", "sum"
        self.radius = 1.0

    def forward(self, q, s, f, idx):
        s = torch.cat([s, torch.zeros_like(s[:1]) + 1e6], 0)
        f = torch.cat([f, torch.zeros_like(f[:1])], 0)
        nf = f[idx]
        d = (s[idx] - q[:, None]).unsqueeze(2) - self.kernel_points
        h = torch.clamp(1 - torch.sqrt((d ** 2).sum(-1) + 1e-8) / self.KP_extent, min=0).transpose(1, 2)
        out = torch.matmul(torch.matmul(h, nf).transpose(0, 1), self.weights).sum(0)
        return out / torch.clamp((nf.sum(-1) > 0).sum(-1), min=1).unsqueeze(1)


class MaxPoolBlock(torch.nn.Module):
    def __init__(self, layer_ind):
        super().__init__()
        self.layer_ind = layer_ind

    def forward(self, feats, batch):
        return torch_pool(feats, batch["pools"][self.layer_ind])


class _Tree(torch.nn.Module):
    """Two convolutions (one nested a level deeper) and a pool over the same inputs."""

    def __init__(self, kp, W, extent):
        super().__init__()
        self.a = _RefShapedConv(kp, W, extent)
        self.inner = torch.nn.Sequential(_RefShapedConv(kp, W.flip(0), extent))
        self.pool = MaxPoolBlock(0)
        self.lin = torch.nn.Linear(W.shape[2], W.shape[2], bias=False)

    def forward(self, q, s, f, idx):
        return self.a(q, s, f, idx), self.inner[0](q, s, f, idx), self.pool(f, {"pools": [idx]})


def test_fuse_swaps_conv_and_pool_shaped_children():
    from pointcloudregistration_amd import kpconv
    c, want, t = case("ragged")
    tree = _Tree(t["kp"], t["W"], c["extent"]).cuda().eval()
    with torch.no_grad():
        before = tree(t["q"], t["s"], t["f"], t["idx"])
    w_a, w_b = tree.a.weights, tree.inner[0].weights
    assert kpconv.fuse(tree) == (2, 1)
    assert isinstance(tree.a, kpconv.KPConv) and isinstance(tree.inner[0], kpconv.KPConv)
    assert isinstance(tree.pool, kpconv.MaxPool) and isinstance(tree.lin, torch.nn.Linear)
    assert tree.a.weights is w_a and tree.inner[0].weights is w_b, "parameters must be shared, not copied"
    assert kpconv.fuse(tree) == (0, 0)
    with torch.no_grad():
        after = tree(t["q"], t["s"], t["f"], t["idx"])
    assert torch.equal(after[2], before[2])
    # unchanged within the bound: the composite and the fused tree both lie within it of the restatement
    refs = (want["linear"][:2],
            kr.kpconv(c["q"], c["s"], c["f"], c["idx"], c["kp"], c["W"][::-1], c["extent"])[:2])
    for outs in (before, after):
        for y, (ref, bound) in zip(outs[:2], refs):
            assert (np.abs(y.cpu().numpy() - ref) <= bound).all()
    assert not torch.equal(after[0], after[1])


def test_memory_is_the_output_and_the_row_flags():
    from pointcloudregistration_amd import kpconv
    n = m = 20000
    k, K, C = 40, 15, 64
    g = torch.Generator().manual_seed(3)
    q = torch.rand(n, 3, generator=g).cuda()
    f = torch.rand(m, C, generator=g).cuda()
    idx = torch.randint(0, m, (n, k), generator=g).cuda()
    kp = (0.05 * torch.randn(K, 3, generator=g)).cuda()
    W = (torch.randn(K, C, C, generator=g) / (K * C) ** 0.5).cuda()
    with torch.no_grad():
        kpconv.kpconv_forward(q[:64], q, f, idx[:64], kp, W, 0.5)   # library load and first-launch allocations
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.max_memory_allocated()
        out = kpconv.kpconv_forward(q, q, f, idx, kp, W, 0.5)
        torch.cuda.synchronize()
        grown = torch.cuda.max_memory_allocated() - before
    out_bytes = out.numel() * 4
    assert n * k * C * 4 > 200e6            # the gathered tensor alone
    assert grown < 2 * out_bytes + (1 << 20), grown
    assert torch.isfinite(out).all()
    # spot-check 48 rows of the large call against the restatement
    rows = torch.arange(0, n, n // 48)[:48]
    ref, bound, _ = kr.kpconv(q[rows].cpu().numpy(), q.cpu().numpy(), f.cpu().numpy(), idx[rows].cpu().numpy(),
                              kp.cpu().numpy(), W.cpu().numpy(), 0.5)
    assert (np.abs(out[rows].cpu().numpy() - ref) <= bound).all()


def test_error_paths():
    from pointcloudregistration_amd import kpconv
    c, _, t = case("m1")
    args = [t["q"], t["s"], t["f"], t["idx"], t["kp"], t["W"], c["extent"]]

    def call(pos=None, val=None, **kw):
        a = list(args)
        if pos is not None:
            a[pos] = val
        with torch.no_grad():
            return kpconv.kpconv_forward(*a, **kw)

    call()
    for pos in (0, 1, 2, 3, 4, 5):
        with pytest.raises((ValueError, TypeError)):
            call(pos, args[pos].cpu())
    with pytest.raises(ValueError, match="int32 or torch.int64"):
        call(3, t["idx"].float())
    with pytest.raises(ValueError):
        call(3, t["idx"][:-1])                       # n mismatch
    with pytest.raises(ValueError):
        call(2, t["f"][:, :-1].contiguous())         # C_in mismatch
    with pytest.raises(ValueError):
        call(4, t["kp"][:-1])                        # K mismatch
    with pytest.raises(ValueError):
        call(0, t["q"][:, :2].contiguous())
    with pytest.raises(ValueError, match="KP_influence"):
        call(KP_influence="gaussian")
    with pytest.raises(NotImplementedError, match="cloest"):
        kpconv.KPConv(8, 8, 1.0, t["kp"], 0.4, aggregation_mode="cloest")
    with pytest.raises(ValueError):
        kpconv.neighbor_max(t["f"].cpu(), t["idx"])
    with pytest.raises(ValueError):
        kpconv.neighbor_max(t["f"], t["idx"].float())
    # forward-only: grad mode with a tensor that requires grad
    w = t["W"].clone().requires_grad_(True)
    with pytest.raises(RuntimeError, match="forward-only"):
        kpconv.kpconv_forward(*args[:5], w, c["extent"])
    with pytest.raises(RuntimeError, match="forward-only"):
        kpconv.neighbor_max(t["f"].clone().requires_grad_(True), t["idx"])
    mod = kpconv.KPConv(8, 8, 1.0, t["kp"], c["extent"]).cuda()
    with pytest.raises(RuntimeError, match="forward-only"):
        mod(t["q"], t["s"], t["f"], t["idx"])
    with torch.no_grad():
        assert mod(t["q"], t["s"], t["f"], t["idx"]).shape == (33, 8)
