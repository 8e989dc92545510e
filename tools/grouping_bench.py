#!/usr/bin/env python
"""Time the grouping ops (pointcloudregistration_amd.grouping) beside a plain
torch composition of the same contract on the same GPU.

Shapes: fps at b=2, n=2048, m=512; ball_query and the fused point-pair group at
b=2, n=2048, K=64, r=0.3 (ROPNet's LocalFeatue), and at K=64, r=0.8 on the same
cloud scaled by 0.8 / 0.3 (NgeNet's PPF: ppf_k 64, radius 0.025 * 32).

Also the k-NN graph and edge features of NgeNet's GCN (knn_graph,
graph_features: dgcnn_k 10, gnn_feats_dim 256) at b=1, n in {512, 2048, 8192}
and b=8, n=2048, beside the reference's tensor program restated from torch ops:
the expanded-form (B,N,N) matrix, topk(k + 1, sorted), the gather, the repeat
and the cat.  Only the neighbour sets and the feature bytes of rows whose order
agrees are compared there (the reference ranks by the expanded form).  For
graph_features the achieved bandwidth over its algorithmic bytes
(B*N*kk*2C*4 written + B*N*C*4 read) is reported beside the time.

The torch side is this project's own wording of the contract the way a tensor
program has to do it: the (B,N,N) direct-form distance matrix, a (B,N,N) int64
index tensor that is sorted, and the element-wise ops of the point-pair
features; fps is a Python loop of m steps.  Its outputs are compared with the
library's before anything is timed (indices and channels 0-5 exactly).

Method: warm-up calls, then the median of per-call HIP-event times; peak memory
is torch's allocator peak over one call (the library's own scratch, which torch
does not see, is added from its size: the (b,n,k) int32 group when the fused op
is not asked for it).  One JSON line per op, and one summary line.

    python tools/grouping_bench.py [--reps 50] [--warmup 10] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pointcloudregistration_amd import grouping  # noqa: E402


# ----------------------------------------------------------- the torch composition
def t_sqdist(a, b):
    d = a[:, :, None, :] - b[:, None, :, :]
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def t_fps(xyz, m, start):
    B, N, _ = xyz.shape
    out = torch.zeros(B, m, dtype=torch.long, device=xyz.device)
    dist = torch.full((B, N), 1e10, device=xyz.device)
    cur = start.clone()
    rows = torch.arange(B, device=xyz.device)
    for i in range(m):
        out[:, i] = cur
        d = t_sqdist(xyz[rows, cur][:, None, :], xyz)[:, 0]
        dist = torch.minimum(dist, d)
        cur = torch.argmax(dist, dim=1)
    return out


def t_ball_query(xyz, query, radius, K):
    B, N, _ = xyz.shape
    inds = torch.arange(N, device=xyz.device).view(1, 1, N).repeat(B, query.shape[1], 1)
    inds[t_sqdist(query, xyz) > radius * radius] = N
    inds = torch.sort(inds, dim=-1)[0][:, :, :K]
    first = inds[:, :, :1].expand(-1, -1, inds.shape[2])
    return torch.where(inds == N, first, inds)


def t_angle(a, c):
    cr = torch.stack([a[..., 1] * c[..., 2] - a[..., 2] * c[..., 1],
                      a[..., 2] * c[..., 0] - a[..., 0] * c[..., 2],
                      a[..., 0] * c[..., 1] - a[..., 1] * c[..., 0]], dim=-1)
    return torch.atan2(torch.norm(cr, dim=-1), torch.sum(a * c, dim=-1))


def t_group_ppf(xyz, normals, radius, K):
    B, N, _ = xyz.shape
    inds = t_ball_query(xyz, xyz, radius, K)
    rows = torch.arange(B, device=xyz.device).view(B, 1, 1)
    g = xyz[rows, inds] - xyz[:, :, None, :]
    ni = normals[:, :, None, :].expand(-1, -1, K, -1)
    nj = normals[rows, inds]
    ppf = torch.stack([t_angle(ni, g), t_angle(nj, g), t_angle(ni, nj), torch.norm(g, dim=-1)], dim=-1)
    feat = torch.cat([xyz[:, :, None, :].expand(-1, -1, K, -1), g, ppf], dim=-1)
    return feat.permute(0, 3, 2, 1).contiguous(), inds


def t_square_dists(a, b):
    # the expanded form |a|^2 + |b|^2 - 2 a.b, as the reference's tensor program forms it
    # (the same ops: two squared norms, one matmul, the clamp at 1e-8)
    d = (a * a).sum(-1)[:, :, None] + (b * b).sum(-1)[:, None, :]
    d -= 2 * torch.matmul(a, b.transpose(1, 2))
    return d.clamp_(min=1e-8)


def t_knn(coords, k):
    n = coords.shape[1]
    inds = torch.topk(t_square_dists(coords, coords), min(n, k + 1), dim=-1, largest=False, sorted=True)[1]
    return inds[:, :, 1:]


def t_edge_features(feats, inds, channels_first):
    B = feats.shape[0]
    rows = torch.arange(B, device=feats.device).view(B, 1, 1)
    fj = feats[rows, inds]
    fi = feats.unsqueeze(2).repeat(1, 1, inds.shape[2], 1)
    out = torch.cat([fi, fj - fi], dim=-1)
    return out.permute(0, 3, 1, 2).contiguous() if channels_first else out


def t_graph_features(feats, coords, k, channels_first):
    return t_edge_features(feats, t_knn(coords, k), channels_first)


# ------------------------------------------------------------------- measurement
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--torch-fps-reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("grouping_bench: no GPU (times are only meaningful on the device)")

    B, N, M, K = 2, 2048, 512, 64
    gen = torch.Generator().manual_seed(0)
    xyz = (torch.rand(B, N, 3, generator=gen) * 2 - 1).cuda()
    nrm = torch.nn.functional.normalize(torch.randn(B, N, 3, generator=gen), dim=-1).cuda()
    start = torch.zeros(B, dtype=torch.long)
    start_d = start.cuda()
    settings = {"ropnet": (xyz, 0.3), "ngenet": ((xyz * (0.8 / 0.3)).contiguous(), 0.8)}

    # same results first
    assert torch.equal(grouping.fps(xyz, M, start=start), t_fps(xyz, M, start_d)), "fps differs"
    for name, (x, r) in settings.items():
        assert torch.equal(grouping.ball_query(x, x, r, K), t_ball_query(x, x, r, K)), name
        f, i = grouping.local_ppf_features(x, nrm, r, K, return_inds=True)
        tf, ti = t_group_ppf(x, nrm, r, K)
        assert torch.equal(i, ti) and torch.equal(f[:, :6], tf[:, :6]), name
        print(json.dumps({"check": name, "max_abs_diff_channels_6_9": float((f[:, 6:] - tf[:, 6:]).abs().max())}))

    rows = []

    def add(op, setting, ours, theirs, theirs_reps, scratch=0):
        a = measure(ours, args.reps, args.warmup)
        a["peak_bytes"] += scratch
        b = measure(theirs, theirs_reps, max(1, args.warmup // 5))
        row = {"op": op, "setting": setting, "library": a, "torch": b,
               "speedup": b["median_ms"] / a["median_ms"]}
        rows.append(row)
        print(json.dumps(row), flush=True)

    add("fps", f"b={B} n={N} m={M}", lambda: grouping.fps(xyz, M, start=start),
        lambda: t_fps(xyz, M, start_d), args.torch_fps_reps)
    for name, (x, r) in settings.items():
        s = f"{name} b={B} n={N} K={K} r={r}"
        add("ball_query", s, lambda: grouping.ball_query(x, x, r, K),
            lambda: t_ball_query(x, x, r, K), args.reps)
        add("ball_query+density", s, lambda: grouping.ball_query(x, x, r, K, rt_density=True),
            lambda: t_ball_query(x, x, r, K), args.reps)
        add("local_ppf_features", s, lambda: grouping.local_ppf_features(x, nrm, r, K),
            lambda: t_group_ppf(x, nrm, r, K)[0], args.reps, scratch=4 * B * N * K)
        add("local_ppf_features channels_last", s,
            lambda: grouping.local_ppf_features(x, nrm, r, K, channels_first=False),
            lambda: t_group_ppf(x, nrm, r, K)[0], args.reps, scratch=4 * B * N * K)
    # the k-NN graph and edge features of NgeNet's GCN
    C, k = 256, 10
    for B, N in ((1, 512), (1, 2048), (1, 8192), (8, 2048)):
        gen = torch.Generator().manual_seed(N + B)
        x = (torch.rand(B, N, 3, generator=gen) * 2 - 1).cuda()
        f = torch.randn(B, N, C, generator=gen).cuda()
        inds, tinds = grouping.knn_graph(x, k), t_knn(x, k)
        same_set = (inds.sort(-1)[0] == tinds.sort(-1)[0]).all(-1)
        same_row = (inds == tinds).all(-1)
        for cf in (False, True):
            assert torch.equal(grouping.graph_features(f, inds=inds, channels_first=cf),
                               t_edge_features(f, inds, cf)), "graph_features differs"
        print(json.dumps({"check": f"knn b={B} n={N}", "rows": B * N,
                          "rows_with_other_set": int((~same_set).sum()),
                          "rows_with_other_order": int((~same_row).sum())}))
        s = f"b={B} n={N} C={C} k={k}"
        kk = min(k, N - 1)
        algo_bytes = 4 * B * N * kk * 2 * C + 4 * B * N * C
        add("knn_graph", s, lambda: grouping.knn_graph(x, k), lambda: t_knn(x, k), args.reps)
        for cf in (False, True):
            name = "channels_first" if cf else "channels_last"
            add(f"edge features ({name}, inds given)", s,
                lambda: grouping.graph_features(f, inds=inds, channels_first=cf),
                lambda: t_edge_features(f, inds, cf), args.reps)
            rows[-1]["algorithmic_bytes"] = algo_bytes
            rows[-1]["library_bytes_per_s"] = algo_bytes / (rows[-1]["library"]["median_ms"] * 1e-3)
            add(f"graph_features ({name}, from coords)", s,
                lambda: grouping.graph_features(f, coords=x, k=k, channels_first=cf),
                lambda: t_graph_features(f, x, k, cf), args.reps)
            rows[-1]["algorithmic_bytes"] = algo_bytes
            rows[-1]["library_bytes_per_s"] = algo_bytes / (rows[-1]["library"]["median_ms"] * 1e-3)
            print(json.dumps({"op": rows[-1]["op"], "setting": s, "algorithmic_bytes": algo_bytes,
                              "edge_only_bytes_per_s": rows[-2]["library_bytes_per_s"],
                              "with_knn_bytes_per_s": rows[-1]["library_bytes_per_s"]}), flush=True)
    summary = {"device": torch.cuda.get_device_name(0), "rows": rows}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(summary, fh, indent=1)
    print(json.dumps({"grouping_bench": "done", "ops": len(rows)}))


if __name__ == "__main__":
    main()
