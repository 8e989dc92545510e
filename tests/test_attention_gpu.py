"""GPU: the fused attention (pointcloudregistration_amd.attention) against the
f64 restatement (tests/attention_ref.py, itself pinned to the reference's
outputs by test_attention_cpu.py): every output within the derived bound at the
tiling's edges, every single weight in the identity-value case, the online
softmax under stress, the offset form's corners, determinism, the memory the
calls take (without and with a key split), the modules and fuse(), and the
error paths.

The tiling these shapes are cut to (csrc/attention.hip): 128 queries per
workgroup (n = 130: a second one), key tiles of 32 (m = 17, 33, 130), 64 value
channels per workgroup (dv = 65, 80, 192, 256: more of them) with dv <= 4 on
the narrow path (dv = 4, 5), kernels unrolled for d <= 48, 64, 128, 256
(d = 48, 49, 64, 65, 128, 129, 256), and a key split where the grid is at most
64 workgroups and there are at least 8 key tiles (m = 300, 1434)."""
import functools

import numpy as np
import pytest
import torch

import attention_cases as ac
import attention_ref as ar

pytestmark = pytest.mark.gpu


def att():
    from pointcloudregistration_amd import attention
    return attention


def cuda(*arrays):
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def check(got, want, bound, what):
    got = got.detach().cpu().numpy().astype(np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.isfinite(got).all(), what
    err = np.abs(got - want)
    ratio = float((err / bound).max())
    print(f"{what}: max err / bound = {ratio:.4f}")
    assert (err <= bound).all(), f"{what}: max err / bound = {ratio}"


# (b, h, n, m, d, dv)
MHA_SHAPES = (
    (1, 1, 1, 1, 1, 1), (1, 1, 1, 17, 3, 5), (3, 4, 33, 17, 48, 64), (1, 4, 16, 16, 64, 80),
    (3, 1, 65, 130, 256, 192), (1, 1, 65, 130, 64, 256), (1, 4, 130, 33, 49, 4), (1, 1, 40, 300, 65, 65),
    (1, 1, 40, 1434, 256, 1), (3, 4, 16, 16, 128, 5), (1, 1, 33, 17, 129, 1),
)


@functools.lru_cache(maxsize=None)
def mha_case(shape):
    """Inputs, the f64 restatement with its bound, CUDA tensors: computed once, shared, never modified."""
    b, h, n, m, d, dv = shape
    q, k, v = ac.random_mha(np.random.default_rng(shape), b, d, h, n, m, dv)
    return (q, k, v), ar.multi_head(q, k, v), cuda(q, k, v)


@pytest.mark.parametrize("shape", MHA_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_multi_head_within_bound(shape):
    _, (want, bound), t = mha_case(shape)
    with torch.no_grad():
        out = att().multi_head_attention(*t)
    assert out.dtype == torch.float32 and out.is_contiguous()
    check(out, want, bound, f"mha {shape}")


def test_interleaved_heads_go_in_by_stride():
    """The (B, dim, nhead, N) reshape of a (B, C, N) tensor and column slices of a wider tensor are
    taken as they are: same bits as from contiguous copies, and within the bound."""
    a = att()
    shape = (3, 4, 33, 17, 48, 64)
    (q, k, v), (want, bound), _ = mha_case(shape)
    b, h, n, m, d, dv = shape
    wide = torch.from_numpy(np.concatenate([q, k], axis=3)).cuda()          # (B, d, h, n + m)
    vwide = torch.from_numpy(np.concatenate([v, v[..., :5]], axis=3)).cuda()
    qs, ks, vs = wide[..., :n], wide[..., n:], vwide[..., :m]
    assert not qs.is_contiguous() and not ks.is_contiguous() and ks.storage_offset() == n
    with torch.no_grad():
        out = a.multi_head_attention(qs, ks, vs)
        base = a.multi_head_attention(qs.contiguous(), ks.contiguous(), vs.contiguous())
        flat = a.multi_head_attention(qs.contiguous().reshape(b, d * h, n).reshape(b, d, h, n), ks, vs)
        # a view without unit token stride is copied once, not misread
        perm = a.multi_head_attention(qs.permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2), ks, vs)
    check(out, want, bound, "column slices")
    assert torch.equal(out, base) and torch.equal(flat, base) and torch.equal(perm, base)


@functools.lru_cache(maxsize=None)
def overlap_case():
    rng = np.random.default_rng(27)
    n1, n2, C = 65, 130, 256
    f = ac.unit_rows(rng, n1 + n2, C)
    s = rng.random((n1 + n2, 1)).astype(np.float32)
    temp = ac.OVERLAP_CASE["temperature"]
    return f, s, n1, temp, ar.overlap_scores(f, s, n1, temp)


def test_overlap_scores_within_bound():
    """A scale of about 27 on unit rows; the transposed view of a (1, C, n) tensor in place."""
    a = att()
    f, s, n1, temp, (want, bound) = overlap_case()
    assert 25 < 1 / temp < 29
    feats = torch.from_numpy(f.T.copy()).cuda()[None]                      # (1, C, n) as the network holds it
    fn = feats.squeeze(0).transpose(0, 1)                                 # (n, C), stride (1, n)
    sc = torch.from_numpy(s.T.copy()).cuda().transpose(0, 1)              # (n, 1), stride (1, n)
    with torch.no_grad():
        out = a.overlap_scores(fn, sc, n1, torch.tensor(temp, dtype=torch.float64))
        copied = a.overlap_scores(fn.contiguous(), sc.contiguous(), n1, temp)
    assert tuple(out.shape) == (f.shape[0], 1)
    check(out, want, bound, "overlap scores")
    assert torch.equal(out, copied)


# (b, n, d, dv, with ol_score)
OFFSET_SHAPES = (
    (1, 1, 1, 1, True), (1, 17, 3, 5, False), (3, 33, 48, 64, True), (1, 16, 64, 80, False),
    (3, 130, 256, 192, True), (1, 65, 48, 256, False), (1, 130, 49, 1, True), (1, 33, 129, 65, False),
)


@functools.lru_cache(maxsize=None)
def offset_case(shape):
    b, n, d, dv, with_ol = shape
    rng = np.random.default_rng(shape[:4])
    q = (rng.standard_normal((b, d, n)) / d ** 0.25).astype(np.float32)    # scores of unit variance
    k = (rng.standard_normal((b, d, n)) / d ** 0.25).astype(np.float32)
    v = rng.standard_normal((b, dv, n)).astype(np.float32)
    ol = rng.random((b, n)).astype(np.float32) if with_ol else None
    if with_ol and n > 3:
        ol[:, 3] = 0.0                                                     # a zero ol_score row
    return (q, k, v, ol), ar.offset_batched(q, k, v, ol), cuda(q, k, v, ol)


@pytest.mark.parametrize("shape", OFFSET_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_offset_within_bound(shape):
    _, (want, bound), t = offset_case(shape)
    with torch.no_grad():
        out = att().offset_attention(*t)
    assert out.dtype == torch.float32
    check(out, want, bound, f"offset {shape}")


def test_identity_values_check_every_weight():
    """V = I with dv = m = 80: the output is the softmax matrix itself.  Scores of order 1, so that
    every weight is over 100 times its bound (checked here): a dropped, doubled or misplaced key
    column cannot pass.  The same for the offset form with V = I over the rows."""
    a = att()
    rng = np.random.default_rng(80)
    n, m, d = 45, 80, 16
    q = rng.standard_normal((1, d, 1, n)).astype(np.float32)
    k = rng.standard_normal((1, d, 1, m)).astype(np.float32)
    v = np.eye(m, dtype=np.float32).reshape(1, m, 1, m)
    out_ref, bound, p, _ = ar.attention(q[0, :, 0], k[0, :, 0], v[0, :, 0], 1 / np.sqrt(d))
    assert np.array_equal(out_ref, p.T) and (p.T > 100 * bound).all()
    with torch.no_grad():
        out = a.multi_head_attention(*cuda(q, k, v))
    check(out[0, :, 0], out_ref, bound, "identity values")

    qo = (rng.standard_normal((1, d, m)) / 2).astype(np.float32)
    ko = (rng.standard_normal((1, d, m)) / 2).astype(np.float32)
    ol = (0.5 + rng.random((1, m))).astype(np.float32)
    vo = np.eye(m, dtype=np.float32)[None]
    want, bo, P = ar.offset_attention(qo[0], ko[0], vo[0], ol[0])
    assert (want > 100 * bo).all()       # want[i, j] = P_ij / (1e-9 + c_j)
    with torch.no_grad():
        out = a.offset_attention(*cuda(qo, ko, vo, ol))
    check(out[0], want, bo, "identity values, offset form")


def _stress(kind, rng, n, m):
    """d = 2, scale 1 / sqrt(2): s_ij = base_j + a_i b_j with |a_i b_j| <= 1."""
    base = rng.uniform(-1, 1, m)
    if kind == "late_max":          # the row maximum in the last key tile, >= 60 above all before it
        base[m - 2] = 70.0
    elif kind == "early_max":       # the maximum first, everything after it about 100 below
        base = base - 100.0
        base[1] = 0.0
    else:                           # all scores equal
        base[:] = 0.7
    bj = np.zeros(m) if kind == "equal" else rng.uniform(-1, 1, m)
    ai = rng.uniform(-1, 1, n)
    q = (np.sqrt(2.0) * np.stack([np.ones(n), ai])).astype(np.float32)      # (2, n)
    k = np.stack([base, bj]).astype(np.float32)                            # (2, m)
    return q, k


@pytest.mark.parametrize("dv", (1, 64))
@pytest.mark.parametrize("kind", ("late_max", "early_max", "equal"))
def test_online_softmax_stress(kind, dv):
    rng = np.random.default_rng((len(kind), dv))
    n, m = 40, 130                                   # five key tiles, the last one ragged
    q, k = _stress(kind, rng, n, m)
    v = rng.standard_normal((dv, m)).astype(np.float32)
    want, bound, p, _ = ar.attention(q, k, v, 1 / np.sqrt(2.0))
    s = (q.astype(np.float64).T @ k.astype(np.float64)) / np.sqrt(2.0)
    if kind == "late_max":
        assert (s[:, m - 2] - np.delete(s, m - 2, 1).max(1) >= 60).all() and (m - 2) // 32 == (m - 1) // 32
    elif kind == "early_max":
        assert (s[:, 1:2] - np.delete(s, 1, 1) >= 96).all() and (np.delete(p, 1, 1) < 2.0 ** -126).all()
    else:
        assert np.ptp(s, axis=1).max() == 0 and np.allclose(p, 1.0 / m, rtol=1e-12)
    with torch.no_grad():
        out = att().multi_head_attention(*cuda(q[None, :, None], k[None, :, None], v[None, :, None]))
    check(out[0, :, 0], want, bound, f"stress {kind} dv={dv}")


@pytest.mark.parametrize("with_ol", (True, False))
def test_offset_column_without_attention(with_ol):
    """One column gets weights of about e^-40 from every row: c_j is far below the 1e-9 it is added
    to.  A zero ol_score row attends uniformly (to that column too)."""
    rng = np.random.default_rng(9 + with_ol)
    n, dv, jz = 70, 64, 37
    base = rng.uniform(-1, 1, n)
    base[jz] = -40.0
    q = np.stack([np.ones(n), rng.uniform(-1, 1, n)]).astype(np.float32)
    k = np.stack([base, rng.uniform(-1, 1, n)]).astype(np.float32)
    v = rng.standard_normal((dv, n)).astype(np.float32)
    ol = None
    if with_ol:
        ol = rng.uniform(0.9, 1.0, n).astype(np.float32)
        ol[5] = 0.0
    want, bound, P = ar.offset_attention(q, k, v, ol)
    c = P.sum(0)
    if with_ol:
        assert np.allclose(P[5], 1.0 / n) and c[jz] > 1e-3     # the uniform row alone carries the column
        assert np.delete(P[:, jz], 5).max() < 1e-14
    else:
        assert c[jz] < 1e-12                                    # the 1e-9 dominates
        assert np.abs(want[:, jz]).max() < 1e-3 * np.abs(want).max()
    with torch.no_grad():
        out = att().offset_attention(*cuda(q[None], k[None], v[None], None if ol is None else ol[None]))
    check(out[0], want, bound, f"offset, column without attention, ol={with_ol}")


def test_determinism_and_batch_independence():
    a = att()
    with torch.no_grad():
        for shape in ((3, 4, 33, 17, 48, 64), (1, 1, 40, 300, 65, 65), (1, 1, 40, 1434, 256, 1)):
            _, _, t = mha_case(shape)
            assert torch.equal(a.multi_head_attention(*t), a.multi_head_attention(*t)), shape
        # batch element 0 alone = its slice of the b = 3 call (neither call splits the keys)
        _, _, t = mha_case((3, 4, 33, 17, 48, 64))
        assert torch.equal(a.multi_head_attention(*(x[:1] for x in t)), a.multi_head_attention(*t)[:1])
        _, _, t = offset_case((3, 130, 256, 192, True))
        full = a.offset_attention(*t)
        assert torch.equal(a.offset_attention(*t), full)
        assert torch.equal(a.offset_attention(*(x[:1] for x in t)), full[:1])


def _peak(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    return out, torch.cuda.max_memory_allocated() - before


def test_memory_multi_head():
    """h = 4, n = m = 4096, d = dv = 64: the scores alone would be 268 MB; the call may take less than
    twice its output plus 1 MiB."""
    a = att()
    g = torch.Generator(device="cuda").manual_seed(4096)
    q, k, v = (torch.randn((1, 64, 4, 4096), device="cuda", generator=g) for _ in range(3))
    with torch.no_grad():
        a.multi_head_attention(q[..., :64], k[..., :64], v[..., :64])      # library start-up is not the call's
        out, peak = _peak(lambda: a.multi_head_attention(q, k, v))
    out_bytes = out.numel() * 4
    print(f"peak {peak} bytes, output {out_bytes}")
    assert peak < 2 * out_bytes + (1 << 20)
    rows = np.random.default_rng(0).choice(4096, 48, replace=False)
    qn, kn, vn = (x.cpu().numpy() for x in (q, k, v))
    want, bound = ar.multi_head(qn[..., rows], kn, vn)
    check(out[..., torch.from_numpy(rows).cuda()], want, bound, "48 rows of 4096")


def test_memory_offset():
    """n = 4096, d = 48, dv = 192 (ROPNet's block at four times its length)."""
    a = att()
    g = torch.Generator(device="cuda").manual_seed(192)
    n = 4096
    q = torch.randn((1, 48, n), device="cuda", generator=g) / 48 ** 0.25
    k = torch.randn((1, 48, n), device="cuda", generator=g) / 48 ** 0.25
    v = torch.randn((1, 192, n), device="cuda", generator=g)
    ol = torch.rand((1, n), device="cuda", generator=g)
    with torch.no_grad():
        a.offset_attention(q[..., :64], k[..., :64], v[..., :64], ol[:, :64])
        out, peak = _peak(lambda: a.offset_attention(q, k, v, ol))
    out_bytes = out.numel() * 4
    print(f"peak {peak} bytes, output {out_bytes}")
    assert peak < 2 * out_bytes + (1 << 20)
    cols = np.sort(np.random.default_rng(1).choice(n, 48, replace=False))
    want, bound, _ = ar.offset_attention(q[0].cpu().numpy(), k[0].cpu().numpy(), v[0].cpu().numpy(),
                                         ol[0].cpu().numpy(), cols=cols)
    check(out[0][:, torch.from_numpy(cols).cuda()], want, bound, "48 columns of 4096")


@pytest.mark.parametrize("shape", ((1, 1, 40, 1434, 256, 1), (1, 4, 1024, 1024, 64, 64)),
                         ids=lambda s: "x".join(map(str, s)))
def test_memory_with_a_key_split(shape):
    """Where the keys are split the call takes its output and the documented scratch, splits * b * h *
    (dv + 2) * n floats with at most 16 splits, i.e. at most 16 (1 + 2 / dv) times the output, and
    nothing of the scores' size."""
    from pointcloudregistration_amd import _lib
    a = att()
    b, h, n, m, d, dv = shape
    g = torch.Generator(device="cuda").manual_seed(n)
    q = torch.randn((b, d, h, n), device="cuda", generator=g)
    k = torch.randn((b, d, h, m), device="cuda", generator=g)
    v = torch.randn((b, dv, h, m), device="cuda", generator=g)
    scratch = _lib.load().pcr_attention_scratch_bytes(b, h, n, m, d, dv)
    out_bytes = b * dv * h * n * 4
    assert 0 < scratch <= 16 * (dv + 2) * b * h * n * 4 + 255
    assert scratch % (b * h * (dv + 2) * n * 4) < 256          # a whole number of runs, rounded up to 256
    with torch.no_grad():
        a.multi_head_attention(q[..., :8], k[..., :8], v[..., :8])
        out, peak = _peak(lambda: a.multi_head_attention(q, k, v))
    print(f"peak {peak} bytes, output {out_bytes}, scratch {scratch}, scores {4 * b * h * n * m}")
    # torch's caching allocator rounds a block up to 512 bytes and, from 1 MiB on, may hand out a cached
    # block up to 1 MiB larger than asked for (it does not split off a smaller remainder)
    block = lambda x: -(-x // 512) * 512 + ((1 << 20) if x >= (1 << 20) else 0)  # noqa: E731
    assert peak <= block(out_bytes) + block(scratch) < 4 * b * h * n * m
    rows = np.random.default_rng(2).choice(n, min(n, 40), replace=False)
    want, bound = ar.multi_head(q.cpu().numpy()[..., rows], k.cpu().numpy(), v.cpu().numpy())
    check(out[..., torch.from_numpy(rows).cuda()], want, bound, f"split {shape}")


# ---------------------------------------------------------------------------
# Modules.  Stand-ins with the reference's class names and attributes, written
# from the formulas (einsum / softmax / einsum; bmm / softmax / column sum / bmm).
# ---------------------------------------------------------------------------
class Cross_Attention(torch.nn.Module):                                      # noqa: N801 (the reference's name)
    def __init__(self, feat_dims, nhead):
        super().__init__()
        nn = torch.nn
        self.feats_dim, self.nhead = feat_dims, nhead
        self.conv = nn.Conv1d(feat_dims, feat_dims, 1)
        self.q_conv, self.k_conv, self.v_conv = (nn.Conv1d(feat_dims, feat_dims, 1) for _ in range(3))
        self.mlp = nn.Sequential(nn.Conv1d(feat_dims * 2, feat_dims * 2, 1), nn.InstanceNorm1d(feat_dims * 2),
                                 nn.ReLU(inplace=True), nn.Conv1d(feat_dims * 2, feat_dims, 1))

    def core(self, feats1, feats2):
        b, dims = feats1.size(0), self.feats_dim // self.nhead
        q = self.q_conv(feats1).reshape(b, dims, self.nhead, -1)
        k = self.k_conv(feats2).reshape(b, dims, self.nhead, -1)
        v = self.v_conv(feats2).reshape(b, dims, self.nhead, -1)
        w = torch.softmax(torch.einsum("bdhn,bdhm->bhnm", q, k) / dims ** 0.5, dim=-1)
        return (q, k, v), torch.einsum("bhnm,bdhm->bdhn", w, v)

    def forward(self, feats1, feats2):
        feats = self.core(feats1, feats2)[1].reshape(feats1.size(0), self.feats_dim, -1)
        return self.mlp(torch.cat([feats1, self.conv(feats)], dim=1))


class OverlapAttentionBlock(torch.nn.Module):
    def __init__(self, channels):
        super().__init__()
        nn = torch.nn
        self.q_conv = nn.Conv1d(channels, channels // 4, 1, bias=False)
        self.k_conv = nn.Conv1d(channels, channels // 4, 1, bias=False)
        self.q_conv.weight = self.k_conv.weight
        self.v_conv = nn.Conv1d(channels, channels, 1)
        self.trans_conv = nn.Conv1d(channels, channels, 1)
        self.after_norm = nn.GroupNorm(channels // 32, channels)
        self.act = nn.ReLU()

    def core(self, x, ol_score):
        q, k, v = self.q_conv(x), self.k_conv(x), self.v_conv(x)
        s = torch.bmm(q.transpose(1, 2), k)
        if ol_score is not None:
            s = ol_score[:, :, None] * s
        w = torch.softmax(s, dim=-1)
        w = w / (1e-9 + w.sum(dim=1, keepdim=True))
        return (q, k, v), torch.bmm(v, w)

    def forward(self, x, ol_score):
        x_r = self.core(x, ol_score)[1]
        return x + self.act(self.after_norm(self.trans_conv(x - x_r)))


class Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.cross = Cross_Attention(64, 4)
        self.blocks = torch.nn.ModuleList([OverlapAttentionBlock(64), OverlapAttentionBlock(64)])


def _conv_abs(conv, x_abs, cols=None):
    """|W| x + |b| of a 1x1 convolution in f64 (cols: the input channels it is applied to)."""
    w = conv.weight.detach().double().abs()[:, :, 0]
    w = w if cols is None else w[:, cols]
    b = 0.0 if conv.bias is None else conv.bias.detach().double().abs()[None, :, None]
    return torch.einsum("oc,bcn->bon", w, x_abs), b


def _conv_round(conv, x_abs):
    """The f32 rounding of a 1x1 convolution: (fan_in + 2) u (|W| |x| + |b|)."""
    wx, b = _conv_abs(conv, x_abs)
    return (conv.in_channels + 2) * ar.U * (wx + b)


def test_modules_state_dict_fuse_and_agreement():
    a = att()
    torch.manual_seed(5)
    net = Net().cuda().eval()
    with torch.no_grad():
        for p in net.parameters():
            p.add_(0.05 * torch.randn_like(p))
    # state dicts go into the fused modules key for key
    ours_c = a.CrossAttention(64, 4).cuda()
    ours_c.load_state_dict(net.cross.state_dict(), strict=True)
    ours_o = a.OverlapAttentionBlock(64).cuda()
    ours_o.load_state_dict(net.blocks[0].state_dict(), strict=True)
    assert ours_o.q_conv.weight is ours_o.k_conv.weight
    assert set(ours_c.state_dict()) == set(net.cross.state_dict())
    assert set(ours_o.state_dict()) == set(net.blocks[0].state_dict())

    g = torch.Generator(device="cuda").manual_seed(6)
    f1 = torch.randn((2, 64, 50), device="cuda", generator=g)
    f2 = torch.randn((2, 64, 70), device="cuda", generator=g)
    ol = torch.rand((2, 50), device="cuda", generator=g)
    # the norms out of the way: what follows the attention is then convolutions and ReLUs, through
    # which a difference propagates by |W| (ReLU being 1-Lipschitz); fuse() shares the submodules
    net.cross.mlp[1] = torch.nn.Identity()
    for blk in net.blocks:
        blk.after_norm = torch.nn.Identity()
    stand_c, stand_o = net.cross, net.blocks[0]
    with torch.no_grad():
        (q, k, v), core_c = stand_c.core(f1, f2)
        want_c = stand_c(f1, f2)
        (xq, xk, xv), core_o = stand_o.core(f1, ol)
        want_o = stand_o(f1, ol)
        want_o_none = stand_o(f1, None)
    params = {id(p) for p in net.parameters()}
    assert a.fuse(net) == (1, 2)
    assert isinstance(net.cross, a.CrossAttention) and isinstance(net.blocks[1], a.OverlapAttentionBlock)
    assert {id(p) for p in net.parameters()} == params and not net.training
    assert net.blocks[0].q_conv.weight is net.blocks[0].k_conv.weight
    assert net.cross.q_conv is stand_c.q_conv and net.blocks[0].trans_conv is stand_o.trans_conv
    assert a.fuse(net) == (0, 0)

    with torch.no_grad():
        got_c = net.cross(f1, f2)
        got_o = net.blocks[0](f1, ol)
        got_o_none = net.blocks[0](f1, None)
    # cross attention: both cores are within `bound` of the f64 restatement of the same q, k, v
    ref, bound = ar.multi_head(*(t.cpu().numpy() for t in (q, k, v)))
    check(core_c, ref, bound, "stand-in core")
    d0 = 2 * torch.from_numpy(bound).cuda().reshape(2, 64, -1)
    core_abs = core_c.double().abs().reshape(2, 64, -1) + d0
    z1 = _conv_abs(stand_c.conv, core_abs)
    r1 = _conv_round(stand_c.conv, core_abs)
    cat_abs = torch.cat([f1.double().abs(), z1[0] + z1[1] + r1], dim=1)
    second = list(range(64, 128))
    h1 = _conv_abs(stand_c.mlp[0], cat_abs)
    d1 = _conv_abs(stand_c.mlp[0], _conv_abs(stand_c.conv, d0)[0], second)[0]
    r2 = _conv_round(stand_c.mlp[0], cat_abs) + _conv_abs(stand_c.mlp[0], r1, second)[0]
    d2 = _conv_abs(stand_c.mlp[3], d1)[0]
    r3 = _conv_round(stand_c.mlp[3], h1[0] + h1[1] + r2) + _conv_abs(stand_c.mlp[3], r2)[0]
    tol = d2 + 2 * r3
    ratio = ((got_c - want_c).double().abs() / tol).max().item()
    print(f"CrossAttention: max diff / propagated bound = {ratio:.4f}")
    assert ratio <= 1.0

    # offset block: x + relu(trans_conv(x - x_r))
    for got, want, o in ((got_o, want_o, ol), (got_o_none, want_o_none, None)):
        ref, bound = ar.offset_batched(*(t.cpu().numpy() for t in (xq, xk, xv)), None if o is None else o.cpu().numpy())
        d0 = 2 * torch.from_numpy(bound).cuda()
        x_r_abs = torch.from_numpy(np.abs(ref)).cuda() + d0
        diff_abs = f1.double().abs() + x_r_abs
        d1 = _conv_abs(stand_o.trans_conv, d0 + 2 * ar.U * diff_abs)[0]     # x - x_r is rounded on both sides
        t1 = _conv_abs(stand_o.trans_conv, diff_abs)
        r1 = _conv_round(stand_o.trans_conv, diff_abs)
        tol = d1 + 2 * r1 + 2 * ar.U * (f1.double().abs() + t1[0] + t1[1] + r1)
        ratio = ((got - want).double().abs() / tol).max().item()
        print(f"OverlapAttentionBlock (ol={o is not None}): max diff / propagated bound = {ratio:.4f}")
        assert ratio <= 1.0


def test_error_paths():
    a = att()
    q = torch.zeros((2, 8, 4, 5), device="cuda")
    k = torch.zeros((2, 8, 4, 7), device="cuda")
    v = torch.zeros((2, 6, 4, 7), device="cuda")
    with torch.no_grad():
        assert tuple(a.multi_head_attention(q, k, v).shape) == (2, 6, 4, 5)
        with pytest.raises(ValueError, match="CUDA"):
            a.multi_head_attention(q.cpu(), k, v)
        with pytest.raises(ValueError, match="CUDA"):
            a.offset_attention(q[:, :, 0].cpu(), q[:, :, 0], q[:, :, 0])
        with pytest.raises(ValueError, match="CUDA"):
            a.overlap_scores(torch.zeros(8, 4), torch.zeros(8, 1), 3, 0.1)
        with pytest.raises(ValueError, match="float32"):
            a.multi_head_attention(q.double(), k, v)
        with pytest.raises(ValueError, match="float32"):
            a.offset_attention(q[:, :, 0].half(), q[:, :, 0], q[:, :, 0])
        with pytest.raises(TypeError):
            a.multi_head_attention(q.cpu().numpy(), k, v)
        for bad_k in (k[:, :7], k[:1], k[:, :, :3]):                      # d, B, nhead
            with pytest.raises(ValueError, match="key"):
                a.multi_head_attention(q, bad_k, v)
        for bad_v in (v[..., :6], v[:1], v[:, :, :3]):                    # m, B, nhead
            with pytest.raises(ValueError, match="value"):
                a.multi_head_attention(q, k, bad_v)
        for d in (0, 257):
            with pytest.raises(ValueError, match=f"dim={d}"):
                a.multi_head_attention(torch.zeros((1, d, 1, 4), device="cuda"),
                                       torch.zeros((1, d, 1, 4), device="cuda"), v[:1, :, :1, :4])
            with pytest.raises(ValueError, match=f"dv={d}"):
                a.multi_head_attention(q[:1, :, :1], k[:1, :, :1, :4], torch.zeros((1, d, 1, 4), device="cuda"))
            with pytest.raises(ValueError, match=f"d={d}"):
                a.offset_attention(torch.zeros((1, d, 4), device="cuda"), torch.zeros((1, d, 4), device="cuda"),
                                   torch.zeros((1, 3, 4), device="cuda"))
            with pytest.raises(ValueError, match=f"C={d}"):
                a.offset_attention(q[:1, :, 0], q[:1, :, 0], torch.zeros((1, d, 5), device="cuda"))
        with pytest.raises(ValueError, match="M = 0"):
            a.multi_head_attention(q, k[..., :0], v[..., :0])
        assert tuple(a.multi_head_attention(q[..., :0], k, v).shape) == (2, 6, 4, 0)
        assert tuple(a.offset_attention(q[:, :, 0, :0], q[:, :, 0, :0], v[:, :, 0, :0]).shape) == (2, 6, 0)
        with pytest.raises(ValueError, match="x_k"):
            a.offset_attention(q[:, :, 0], k[:, :, 0], v[:, :, 0, :5])
        with pytest.raises(ValueError, match="x_v"):
            a.offset_attention(q[:, :, 0], q[:, :, 0], v[:, :, 0])
        with pytest.raises(ValueError, match="ol_score"):
            a.offset_attention(q[:, :, 0], q[:, :, 0], v[:, :, 0, :5], torch.zeros((2, 4), device="cuda"))
        with pytest.raises(ValueError, match="len_src"):
            a.overlap_scores(torch.zeros((8, 4), device="cuda"), torch.zeros((8, 1), device="cuda"), 8, 0.1)
        with pytest.raises(ValueError, match="attn_scores"):
            a.overlap_scores(torch.zeros((8, 4), device="cuda"), torch.zeros((7, 1), device="cuda"), 3, 0.1)
    # an input that requires grad under grad mode raises; detached or under no_grad it runs
    qg = q.clone().requires_grad_(True)
    with pytest.raises(RuntimeError, match="forward-only"):
        a.multi_head_attention(qg, k, v)
    with pytest.raises(RuntimeError, match="forward-only"):
        a.offset_attention(qg[:, :, 0], q[:, :, 0], v[:, :, 0, :5])
    with pytest.raises(RuntimeError, match="forward-only"):
        a.overlap_scores(torch.zeros((8, 4), device="cuda", requires_grad=True), torch.zeros((8, 1), device="cuda"),
                         3, 0.1)
    with pytest.raises(RuntimeError, match="forward-only"):
        a.CrossAttention(8, 2).cuda()(torch.zeros((1, 8, 4), device="cuda"), torch.zeros((1, 8, 4), device="cuda"))
    with torch.no_grad():
        assert not a.multi_head_attention(qg, k, v).requires_grad
    assert not a.multi_head_attention(qg.detach(), k, v).requires_grad
