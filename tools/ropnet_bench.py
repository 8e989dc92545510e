#!/usr/bin/env python
"""Time ROPNet's dense stages on pointcloudregistration_amd.ropnet beside the
reference's formulas written as torch ops on the same GPU, parameters and data.

Shapes (ROPNet's own): B in {2, 8}, N = M = 2048, feat_dim 192.
  cg        CGModule.forward: encoder 3 -> 192 -> 192 -> 192 -> 384 -> 1536 with
            the max over points, decoder_qt, and the overlap decoder; torch
            builds the (B, 6144, N) ensembles, the library does not
  oa        OverlapAttention (five blocks and conv_fuse); torch: the blocks'
            Conv1d / bmm / softmax / GroupNorm and torch.cat of the five outputs
  pw_*      single calls: conv_fuse (960 -> 960 over five sources, GroupNorm(20),
            LeakyReLU), a block's tail (192 -> 192, sub, GroupNorm(6), ReLU,
            residual), the split decoder layer (1536 -> 1536 with a cloud bias)
            and the n = 1 cloud-bias product over 4608 inputs
  forward   ropnet.forward, num_iter = 2, on a network with random parameters
            (library only: N1 = 896, M1 = 1434, 64 neighbours, radius 0.3)

Both sides are compared before anything is timed (max abs difference, reported).
Method: warm-up calls, then the median of per-call HIP-event times, the Python
call included; peak memory is torch's allocator peak over one call (the
library's scratch is a torch byte tensor, so the peak contains it).  One JSON
line per row.

    python tools/ropnet_bench.py [--reps 20] [--warmup 5] [--batches 2 8] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pointcloudregistration_amd import ropnet  # noqa: E402

nn = torch.nn
F = torch.nn.functional


def conv_stack(in_dim, dims, relu):
    seq = nn.Sequential()
    for i, d in enumerate(dims):
        seq.add_module(f"pointnet_conv_{i}", nn.Conv1d(in_dim, d, 1))
        if relu and i != len(dims) - 1:
            seq.add_module(f"pointnet_relu_{i}", nn.ReLU(inplace=True))
        in_dim = d
    return seq


class Holder(nn.Module):
    def __init__(self, **mods):
        super().__init__()
        for k, v in mods.items():
            setattr(self, k, v)


class CGModule(nn.Module):
    """The reference's structure and, in forward, its formulas as torch ops."""

    def __init__(self):
        super().__init__()
        self.encoder = Holder(backbone=conv_stack(3, [192, 192, 192, 384, 1536], False), cls=False)
        self.decoder_ol = Holder(backbone=conv_stack(6144, [1536, 1536, 768, 2], True), cls=True)
        mlps = nn.Sequential()
        for i, (a, b) in enumerate(((3072, 1536), (1536, 1536), (1536, 768), (768, 7))):
            mlps.add_module(f"fc_{i}", nn.Linear(a, b))
            if i != 3:
                mlps.add_module(f"relu_{i}", nn.ReLU(inplace=True))
                mlps.add_module(f"dropout_{i}", nn.Dropout(0.2))
        self.decoder_qt = Holder(mlps=mlps)

    def forward(self, src, tgt):
        f_x, f_y = (self.encoder.backbone(t.permute(0, 2, 1).contiguous()) for t in (src, tgt))
        g_x, g_y = f_x.max(2)[0], f_y.max(2)[0]
        out = self.decoder_qt.mlps(torch.cat((g_x, g_y), dim=1))
        quat = out[:, 3:] / (torch.norm(out[:, 3:], dim=1, keepdim=True) + 1e-8)
        T = torch.cat([ropnet.batch_quat2mat(quat), out[:, :3, None]], dim=-1)
        ex, ey = g_x.unsqueeze(-1).expand_as(f_x), g_y.unsqueeze(-1).expand_as(f_y)
        x_ol = self.decoder_ol.backbone(torch.cat([f_x, ex, ey, ex - ey], dim=1))
        y_ol = self.decoder_ol.backbone(torch.cat([f_y, ey, ex, ey - ex], dim=1))
        return T, x_ol, y_ol


class Block(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.q_conv = nn.Conv1d(c, c // 4, 1, bias=False)
        self.k_conv = nn.Conv1d(c, c // 4, 1, bias=False)
        self.q_conv.weight = self.k_conv.weight
        self.v_conv, self.trans_conv = nn.Conv1d(c, c, 1), nn.Conv1d(c, c, 1)
        self.after_norm, self.act = nn.GroupNorm(c // 32, c), nn.ReLU()

    def forward(self, x, ol=None):
        att = torch.bmm(self.q_conv(x).permute(0, 2, 1).contiguous(), self.k_conv(x))
        att = torch.softmax(att if ol is None else ol.unsqueeze(-1) * att, dim=-1)
        att = att / (1e-9 + att.sum(dim=1, keepdims=True))
        x_r = torch.bmm(self.v_conv(x), att)
        return x + self.act(self.after_norm(self.trans_conv(x - x_r)))


class OverlapAttention(nn.Module):
    def __init__(self, dim):
        super().__init__()
        for i in range(1, 6):
            setattr(self, f"overlap_attention{i}", Block(dim))
        self.conv_fuse = nn.Sequential(nn.Conv1d(dim * 5, dim * 5, 1, bias=False), nn.GroupNorm(20, dim * 5),
                                       nn.LeakyReLU(0.2))

    def forward(self, x, ol=None):
        xs = []
        for i in range(1, 6):
            x = getattr(self, f"overlap_attention{i}")(x, ol)
            xs.append(x)
        return self.conv_fuse(torch.cat(xs, dim=1))


class LocalFeatue(nn.Module):
    def __init__(self, radius, K, in_dim, dims):
        super().__init__()
        self.radius, self.K = radius, K
        blocks = nn.Sequential()
        for i, d in enumerate(dims):
            blocks.add_module(f"conv2d_{i}", nn.Conv2d(in_dim, d, 1, bias=False))
            blocks.add_module(f"gn_{i}", nn.GroupNorm(d // 32, d))
            blocks.add_module(f"relu_{i}", nn.ReLU(inplace=True))
            in_dim = d
        self.local_feature_fused = Holder(blocks=blocks)


class ROPNet(nn.Module):
    def __init__(self, N1=896, M1=1434, feat_dim=192, K=64, radius=0.3):
        super().__init__()
        self.N1, self.use_ppf = N1, True
        self.cg = CGModule()
        self.tfmr = Holder(local_features=LocalFeatue(radius, K, 10, [256, 512, feat_dim]),
                           overlap_attention=OverlapAttention(feat_dim))
        self.tfmr.N1s, self.tfmr.M1s, self.tfmr.top_probs = [N1, N1], [M1, M1], [0.6, 0.4]
        self.tfmr.similarity_topks, self.tfmr.use_ppf = [3, 1], True


def measure(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    times.sort()
    return {"median_ms": statistics.median(times), "min_ms": times[0],
            "p90_ms": times[int(0.9 * (len(times) - 1))], "reps": reps, "peak_bytes": int(peak)}


def row(name, shape, ours, theirs, args):
    with torch.no_grad():
        r = {"op": name, **shape, "library": None}
        if theirs is not None:
            a, b = ours(), theirs()
            a, b = (a, b) if isinstance(a, (tuple, list)) else ((a,), (b,))
            r["max_abs_diff"] = max(float((x - y).abs().max()) for x, y in zip(a, b))
            del a, b
        r["library"] = measure(ours, args.reps, args.warmup)
        if theirs is not None:
            r["torch"] = measure(theirs, args.reps, args.warmup)
            r["speedup"] = r["torch"]["median_ms"] / r["library"]["median_ms"]
    print(json.dumps(r), flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batches", type=int, nargs="+", default=[2, 8])
    ap.add_argument("--points", type=int, default=2048)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ropnet_bench: no GPU (times are only meaningful on the device)")
    torch.manual_seed(1)
    torch.set_grad_enabled(False)
    gen = torch.Generator(device="cuda").manual_seed(1)
    randn = lambda *s: torch.randn(s, device="cuda", generator=gen)  # noqa: E731
    n, dim = args.points, 192
    t_cg, t_oa = CGModule().cuda().eval(), OverlapAttention(dim).cuda().eval()
    cg, oa = ropnet.CG(t_cg), ropnet.OverlapAttention(t_oa)
    net = ROPNet().cuda().eval()
    from pointcloudregistration_amd import groupmlp
    assert ropnet.fuse(net) == (1, 1) and groupmlp.fuse(net) == (0, 0, 1)
    rows = []
    for b in args.batches:
        shape = {"b": b, "n": n}
        src = torch.rand((b, n, 3), device="cuda", generator=gen) - 0.5
        tgt = torch.rand((b, n, 3), device="cuda", generator=gen) - 0.5
        rows.append(row("cg", shape, lambda: cg(src, tgt), lambda: t_cg(src, tgt), args))
        x = randn(b, dim, n)
        rows.append(row("oa", shape, lambda: oa(x, None), lambda: t_oa(x, None), args))
        xs = [randn(b, dim, n) for _ in range(5)]
        conv, norm = t_oa.conv_fuse[0], t_oa.conv_fuse[1]
        rows.append(row("pw_conv_fuse", shape,
                        lambda: ropnet.pointwise_forward(xs, conv.weight, groups=20, gamma=norm.weight, beta=norm.bias,
                                                         act=True, slope=0.2),
                        lambda: t_oa.conv_fuse(torch.cat(xs, dim=1)), args))
        blk = t_oa.overlap_attention1
        rows.append(row("pw_block_tail", shape,
                        lambda: ropnet.pointwise_forward(xs[0], blk.trans_conv.weight, sub=xs[1],
                                                         bias=blk.trans_conv.bias, groups=6,
                                                         gamma=blk.after_norm.weight, beta=blk.after_norm.bias,
                                                         act=True, residual=xs[0]),
                        lambda: xs[0] + blk.act(blk.after_norm(blk.trans_conv(xs[0] - xs[1]))), args))
        f, gx, gy = randn(b, 1536, n), randn(b, 1536, 1), randn(b, 1536, 1)
        w = t_cg.decoder_ol.backbone[0].weight[:, :, 0]
        bias = t_cg.decoder_ol.backbone[0].bias
        cb = lambda: ropnet.pointwise_forward((gx, gy, gx), w[:, 1536:], sub=(None, None, gy), bias=bias)  # noqa: E731
        rows.append(row("pw_cloud_bias_4608", {"b": b, "n": 1}, cb,
                        lambda: F.conv1d(torch.cat([gx, gy, gx - gy], 1), w[:, 1536:, None], bias), args))
        cbias = cb().squeeze(-1)
        rows.append(row("pw_split_layer", shape,
                        lambda: ropnet.pointwise_forward(f, w[:, :1536], cloud_bias=cbias, act=True),
                        lambda: F.relu(F.conv1d(torch.cat([f, gx.expand_as(f), gy.expand_as(f),
                                                           (gx - gy).expand_as(f)], 1), w[:, :, None], bias)), args))
        del f, xs, x
        s6 = torch.cat([src, F.normalize(randn(b, n, 3), dim=-1)], -1)
        t6 = torch.cat([tgt, F.normalize(randn(b, n, 3), dim=-1)], -1)
        rows.append(row("forward", dict(shape, num_iter=2),
                        lambda: ropnet.forward(net, s6, t6, num_iter=2)["pred_Ts"][-1], None, args))
    summary = {"device": torch.cuda.get_device_name(0), "rows": rows}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(summary, fh, indent=1)
    print(json.dumps({"ropnet_bench": "done", "rows": len(rows)}))


if __name__ == "__main__":
    main()
