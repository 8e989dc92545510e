#!/usr/bin/env python
"""Time the fused attention (pointcloudregistration_amd.attention) beside the
reference's formulas written as torch ops on the same GPU and data.

Shapes:
  cross     NgeNet's Cross_Attention (MRI.yaml: 256 features, 4 heads): h = 4,
            d = dv = 64, n = m in {256, 1024, 3000}; torch: einsum, softmax, einsum
  overlap   NgeNet's overlap scores at the same n (n1 = n2 = n, C = 256, the
            temperature's scale of about 27): torch: matmul, two softmaxes, two matmuls
  offset    ROPNet's OverlapAttentionBlock: b in {2, 8}, n = 1024, d = 48,
            dv = 192, with ol_score; torch: bmm, softmax, column sum, bmm

Both sides are compared before anything is timed (max abs difference, reported).
Method: warm-up calls, then the median of per-call HIP-event times, the Python
call included; peak memory is torch's allocator peak over one call (the
library's scratch is a torch byte tensor, so the peak contains it).  One JSON
line per shape.

    python tools/attention_bench.py [--reps 50] [--warmup 10] [--out FILE]
"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pointcloudregistration_amd import attention  # noqa: E402


def t_mha(query, key, value):
    scores = torch.einsum("bdhn,bdhm->bhnm", query, key) / query.size(1) ** 0.5
    return torch.einsum("bhnm,bdhm->bdhn", torch.softmax(scores, dim=-1), value)


def t_overlap(fn, sc, n1, temperature):
    """Both softmax-weighted sums of the overlap scores from one dense (n1, n2) product."""
    inner = fn[:n1] @ fn[n1:].t() / temperature
    return torch.cat([inner.softmax(1) @ sc[n1:], inner.t().softmax(1) @ sc[:n1]])


def t_offset(x_q, x_k, x_v, ol):
    """Row softmax of the scaled (B, N, N) product, columns normalised by 1e-9 + their sums."""
    w = (ol.unsqueeze(-1) * (x_q.transpose(1, 2) @ x_k)).softmax(-1)
    return x_v @ (w / (w.sum(1, keepdim=True) + 1e-9))


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


def row(name, shape, ours, theirs, flops, args):
    with torch.no_grad():
        diff = float((ours() - theirs()).abs().max())
        a = measure(ours, args.reps, args.warmup)
        b = measure(theirs, args.reps, args.warmup)
    r = {"op": name, **shape, "library": a, "torch": b, "speedup": b["median_ms"] / a["median_ms"],
         "max_abs_diff": diff, "gflop": flops / 1e9, "library_tflops": flops / a["median_ms"] / 1e9}
    print(json.dumps(r), flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("attention_bench: no GPU (times are only meaningful on the device)")
    gen = torch.Generator(device="cuda").manual_seed(1)
    randn = lambda *s: torch.randn(s, device="cuda", generator=gen)  # noqa: E731
    rows = []
    temperature = math.exp(-5.0) + 0.03
    for n in (256, 1024, 3000):
        # the network's layout: (1, 256, n) conv outputs viewed as (1, 64, 4, n)
        q, k, v = (randn(1, 256, n).reshape(1, 64, 4, n) for _ in range(3))
        rows.append(row("cross", {"b": 1, "h": 4, "n": n, "m": n, "d": 64, "dv": 64},
                        lambda: attention.multi_head_attention(q, k, v), lambda: t_mha(q, k, v),
                        4 * n * n * (2 * 64 + 2 * 64), args))
        feats = torch.nn.functional.normalize(randn(1, 256, 2 * n), dim=1)
        fn = feats.squeeze(0).transpose(0, 1)
        sc = torch.rand((1, 2 * n), device="cuda", generator=gen).transpose(0, 1)
        rows.append(row("overlap", {"n1": n, "n2": n, "C": 256},
                        lambda: attention.overlap_scores(fn, sc, n, temperature),
                        lambda: t_overlap(fn, sc, n, temperature), 2 * n * n * (2 * 256 + 2), args))
    for b in (2, 8):
        n, d, dv = 1024, 48, 192
        xq, xk = randn(b, d, n) / d ** 0.25, randn(b, d, n) / d ** 0.25
        xv = randn(b, dv, n)
        ol = torch.rand((b, n), device="cuda", generator=gen)
        rows.append(row("offset", {"b": b, "n": n, "d": d, "dv": dv},
                        lambda: attention.offset_attention(xq, xk, xv, ol), lambda: t_offset(xq, xk, xv, ol),
                        b * n * n * (2 * 2 * d + 2 * dv), args))
    summary = {"device": torch.cuda.get_device_name(0), "rows": rows}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(summary, fh, indent=1)
    print(json.dumps({"attention_bench": "done", "shapes": len(rows)}))


if __name__ == "__main__":
    main()
