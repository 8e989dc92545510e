#!/usr/bin/env python
"""Time the fused GCN / PPF / LocalFeatue blocks (pointcloudregistration_amd.groupmlp)
beside the path a user had before them, on the same GPU: grouping.graph_features
/ grouping.local_ppf_features feeding torch's Conv2d -> norm -> activation -> max
chain with the same weights.

Shapes: GCN at B=1, N in {512, 2048}, C=256, k=10 (NgeNet: gnn_feats_dim 256,
dgcnn_k 10); PPF at B=1, N in {512, 2048}, K=64, widths 256/512/256 (ppf_k 64);
ROPNet's LocalFeatue at B=8, N=1024, K=64, widths 256/512/192 (GroupNorm, affine).

Per shape and side: the whole block (front end included) and the fused op alone
beside the torch chain alone; the allocator's peak over one call; for the fused
op the achieved TFLOP/s, the recomputed layers counted as done work (pass l runs
layers 1..l).  With --errors the worst error / bound ratio (tests/groupmlp_ref.py)
of the fused result on the GPU and of the torch chain run on the CPU, at the
N = 512 shapes and one cloud of the LocalFeatue shape (the f64 restatement runs
on the host and takes a while).

Method: warm-up calls, then per-call HIP-event times: median, min and max.

    python tools/groupmlp_bench.py [--reps 50] [--warmup 10] [--errors] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pointcloudregistration_amd import grouping, groupmlp  # noqa: E402

nn = torch.nn


class Chain(nn.Module):
    """LocalFeatureFused: (Conv2d 1x1, norm, ReLU) per width, then the max over K."""

    def __init__(self, cin, widths, group_norm):
        super().__init__()
        self.blocks = nn.Sequential()
        for i, c in enumerate(widths):
            self.blocks.add_module(f"conv2d_{i}", nn.Conv2d(cin, c, 1, bias=False))
            self.blocks.add_module(f"n_{i}", nn.GroupNorm(c // 32, c) if group_norm else nn.InstanceNorm2d(c))
            self.blocks.add_module(f"relu_{i}", nn.ReLU(inplace=True))
            cin = c

    def forward(self, x):
        return torch.max(self.blocks(x), dim=2)[0]


class GCN(nn.Module):
    def __init__(self, c, k):
        super().__init__()
        self.conv1 = nn.Sequential(nn.Conv2d(2 * c, c, 1, bias=False), nn.InstanceNorm2d(c), nn.LeakyReLU(0.2))
        self.conv2 = nn.Sequential(nn.Conv2d(2 * c, 2 * c, 1, bias=False), nn.InstanceNorm2d(2 * c), nn.LeakyReLU(0.2))
        self.conv3 = nn.Sequential(nn.Conv1d(4 * c, c, 1, bias=False), nn.InstanceNorm1d(c), nn.LeakyReLU(0.2))
        self.k = k

    def edge(self, block, feats, inds):
        return block(grouping.graph_features(feats.permute(0, 2, 1), inds=inds, channels_first=True)).max(-1)[0]

    def forward(self, coords, feats):
        inds = grouping.knn_graph(coords.permute(0, 2, 1), self.k)
        f1 = self.edge(self.conv1, feats, inds)
        f2 = self.edge(self.conv2, f1, inds)
        return self.conv3(torch.cat([feats, f1, f2], dim=1))


class PPF(nn.Module):
    def __init__(self, widths, k, radius):
        super().__init__()
        self.k, self.radius = k, radius
        self.local_feature_fused = Chain(10, widths, False)

    def forward(self, coords, feats):
        return self.local_feature_fused(grouping.local_ppf_features(coords.permute(0, 2, 1), feats.permute(0, 2, 1),
                                                                    self.radius, self.k))


class LocalFeatue(nn.Module):
    def __init__(self, radius, K, cin, widths):
        super().__init__()
        self.radius, self.K = radius, K
        self.local_feature_fused = Chain(cin, widths, True)

    def forward(self, feature, xyz, permute=False, use_ppf=False):
        return self.local_feature_fused(grouping.local_ppf_features(xyz, feature, self.radius, self.K))


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
    return {"median_ms": statistics.median(times), "min_ms": min(times), "max_ms": max(times), "reps": reps,
            "peak_bytes": int(peak)}


def host(t):
    return t.detach().cpu().numpy()


def mlp_arrays(chain):
    mods = list(chain.blocks.children())
    gn = isinstance(mods[1], nn.GroupNorm)
    ws = [host(m.weight)[:, :, 0, 0] for m in mods[0::3]]
    gs = [host(m.weight) if gn else None for m in mods[1::3]]
    bs = [host(m.bias) if gn else None for m in mods[1::3]]
    return ws, gs, bs, 32 if gn else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--errors", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("groupmlp_bench: no GPU (times are only meaningful on the device)")
    if args.errors:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import groupmlp_ref as ref
        import knn_graph_ref as kr
    torch.manual_seed(0)
    rows = []

    def add(op, setting, ours, theirs, flops=None, extra=None):
        a, b = measure(ours, args.reps, args.warmup), measure(theirs, args.reps, args.warmup)
        row = {"op": op, "setting": setting, "fused": a, "torch": b, "speedup": b["median_ms"] / a["median_ms"],
               "not_slower_within_spread": a["median_ms"] - b["median_ms"] <=
               (a["max_ms"] - a["min_ms"]) + (b["max_ms"] - b["min_ms"])}
        if flops:
            row["flops"] = flops
            row["fused_tflops"] = flops / (a["median_ms"] * 1e-3) / 1e12
        row.update(extra or {})
        rows.append(row)
        print(json.dumps(row), flush=True)

    def cloud(b, n, seed):
        gen = torch.Generator().manual_seed(seed)
        xyz = (torch.rand(b, n, 3, generator=gen) * 2 - 1).cuda()
        nrm = nn.functional.normalize(torch.randn(b, n, 3, generator=gen), dim=-1).cuda()
        return xyz, nrm, gen

    with torch.no_grad():
        c, k = 256, 10
        for n in (512, 2048):
            xyz, _, gen = cloud(1, n, n)
            coords = xyz.permute(0, 2, 1).contiguous()
            feats = torch.randn(1, c, n, generator=gen).cuda()
            plain = GCN(c, k).cuda().eval()
            fused = groupmlp.GCN(plain)
            inds = grouping.knn_graph(xyz, k)
            s = f"GCN b=1 n={n} C={c} k={k}"
            err = {}
            if args.errors and n == 512:
                idx, _ = kr.knn_graph(host(xyz), k)
                w1 = host(plain.conv1[0].weight)[:, :, 0, 0]
                want, e = ref.edge_conv(w1, host(feats)[0].T, idx[0], 1e-5, 0.2)
                got = groupmlp.edge_conv(feats, inds, plain.conv1[0].weight, channels_first=True)
                cpu = GCN(c, k).eval()
                cpu.load_state_dict(plain.state_dict())
                g = torch.from_numpy(kr.edge_features(host(feats.permute(0, 2, 1)), idx, channels_first=True))
                err = {"fused_error_over_bound": ref.ratio(host(got)[0].T, want, e),
                       "torch_cpu_error_over_bound": ref.ratio(host(cpu.conv1(g).max(-1)[0])[0].T, want, e)}
            add("block", s, lambda: fused(coords, feats), lambda: plain(coords, feats))
            for name, blk, f_in in (("conv1", plain.conv1, feats), ("conv2", plain.conv2, plain.edge(plain.conv1, feats, inds))):
                co, ci = blk[0].weight.shape[:2]
                add(f"edge_conv {name} ({ci}->{co})", s,
                    lambda: groupmlp.edge_conv(f_in, inds, blk[0].weight, channels_first=True),
                    lambda: plain.edge(blk, f_in, inds), flops=2 * n * ci * co, extra=err if name == "conv1" else None)

        for kind, b, n, kk, radius, widths in (("PPF", 1, 512, 64, 0.8, (256, 512, 256)),
                                               ("PPF", 1, 2048, 64, 0.8, (256, 512, 256)),
                                               ("LocalFeatue", 8, 1024, 64, 0.3, (256, 512, 192))):
            xyz, nrm, _ = cloud(b, n, n + b)
            if kind == "PPF":
                xyz = xyz * (0.8 / 0.3)
                plain = PPF(list(widths), kk, radius).cuda().eval()
                fused = groupmlp.PPF(plain)
                coords, normals = xyz.permute(0, 2, 1).contiguous(), nrm.permute(0, 2, 1).contiguous()
                ours, theirs = (lambda: fused(coords, normals)), (lambda: plain(coords, normals))
            else:
                plain = LocalFeatue(radius, kk, 10, list(widths)).cuda().eval()
                for m in plain.modules():
                    if isinstance(m, nn.GroupNorm):
                        m.weight.uniform_(-1.5, 1.5)
                        m.bias.uniform_(-0.5, 0.5)
                fused = groupmlp.LocalFeature(plain)
                ours, theirs = (lambda: fused(nrm, xyz, use_ppf=True)), (lambda: plain(nrm, xyz, use_ppf=True))
            s = f"{kind} b={b} n={n} K={kk} widths={'/'.join(map(str, widths))}"
            chain = plain.local_feature_fused
            plan = groupmlp._mlp_plan(chain, kind)
            x_last = grouping.local_ppf_features(xyz, nrm, radius, kk, channels_first=False)
            x_first = grouping.local_ppf_features(xyz, nrm, radius, kk)
            c1, c2, c3 = widths
            flops = 2 * b * n * kk * (3 * 10 * c1 + 2 * c1 * c2 + c2 * c3)
            err = {}
            if args.errors and (n == 512 or kind == "LocalFeatue"):
                ws, gs, bs, group = mlp_arrays(chain)
                want, e, _ = ref.group_mlp(host(x_last)[0], ws, gs, bs, 1e-5, 0.0, group)
                got = groupmlp.group_mlp(x_last[:1], **plan)
                cpu = Chain(10, widths, group == 32).eval()
                cpu.load_state_dict(chain.state_dict())
                err = {"fused_error_over_bound": ref.ratio(host(got)[0].T, want, e),
                       "torch_cpu_error_over_bound": ref.ratio(host(cpu(x_first[:1].cpu()))[0].T, want, e)}
            add("block", s, ours, theirs)
            add("group_mlp", s, lambda: groupmlp.group_mlp(x_last, **plan), lambda: chain(x_first), flops=flops,
                extra=err)

    summary = {"device": torch.cuda.get_device_name(0), "rows": rows}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(summary, fh, indent=1)
    print(json.dumps({"groupmlp_bench": "done", "ops": len(rows)}))


if __name__ == "__main__":
    main()
