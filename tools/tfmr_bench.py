#!/usr/bin/env python
"""Time the TFMR matching (pointcloudregistration_amd.matching.tfmr_match) beside
the same contract written as a torch tensor program on the same GPU.

Shapes: ROPNet's (configs/arguments.py:26-36): N1 = 896, M1 = 1434, C = 960,
B in {2, 8}, (k, top_prob) in {(1, 0.4), (3, 0.6)} (test and train).

The torch side is the reference's wording of TFMR.py:226-257: bmm similarity,
row maxima, sort, gather, topk, a zeros_like mask written by index_put, the
normalisation and a second bmm -- three (B,N1,M1) f32 tensors.  Its selection
is compared with the library's before anything is timed (rows whose maxima
differ by under an ulp may swap places under bmm's summation order: the count
of differing places is reported, not asserted).

Method: warm-up calls, then the median of per-call HIP-event times, the Python
call included; peak memory is torch's allocator peak over one call (the
library's scratch is a torch byte tensor, so the peak contains it; its size is
also reported).  similarity_topk alone is timed too: the sweep and its merge
are two of the call's three launches.  One JSON line per configuration.

    python tools/tfmr_bench.py [--reps 50] [--warmup 10] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pointcloudregistration_amd import _lib, matching  # noqa: E402


def t_match(fx, fy, src, tgt, x_ol, top_prob, k):
    B, N1, _ = fx.shape
    dev = fx.device
    similarity = torch.bmm(fx, fy.permute(0, 2, 1).contiguous())
    N2 = int(top_prob * N1)
    similarity_max = torch.max(similarity, dim=-1)[0]
    inds = torch.sort(similarity_max, dim=-1, descending=True)[1][:, :N2]
    bi = torch.arange(B, device=dev).view(B, 1)
    src = src[bi, inds]
    similarity = similarity[bi, inds]
    x_ol = x_ol[bi, inds]
    topk_inds = torch.topk(similarity, k=k, dim=-1)[1]
    mask = torch.zeros_like(similarity)
    inds1 = torch.arange(B, dtype=torch.long, device=dev).reshape((B, 1, 1)).repeat((1, N2, k))
    inds2 = torch.arange(N2, dtype=torch.long, device=dev).reshape((1, N2, 1)).repeat((B, 1, k))
    mask[inds1, inds2, topk_inds] = 1
    similarity = similarity * mask
    weights = similarity / (torch.sum(similarity, dim=-1, keepdim=True) + 1e-8)
    return src, torch.bmm(weights, tgt), x_ol, inds


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
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tfmr_bench: no GPU (times are only meaningful on the device)")

    N1, M1, C = 896, 1434, 960
    rows = []
    for B in (2, 8):
        gen = torch.Generator().manual_seed(B)
        fx = torch.nn.functional.normalize(torch.randn(B, N1, C, generator=gen), dim=-1)
        fy = torch.nn.functional.normalize(torch.randn(B, M1, C, generator=gen), dim=-1)
        fy[:, :M1 // 2] = torch.nn.functional.normalize(
            fx[:, :M1 // 2] + torch.linspace(0.05, 1.5, M1 // 2)[None, :, None]
            * torch.randn(B, M1 // 2, C, generator=gen), dim=-1)
        fx, fy = fx.cuda(), fy.cuda()
        src, tgt = torch.rand(B, N1, 3, generator=gen).cuda(), torch.rand(B, M1, 3, generator=gen).cuda()
        x_ol = torch.rand(B, N1, generator=gen).cuda()
        for k, p in ((1, 0.4), (3, 0.6)):
            ours = matching.tfmr_match(fx, fy, src, tgt, x_ol, p, k)
            theirs = t_match(fx, fy, src, tgt, x_ol, p, k)
            differ = int((ours[3] != theirs[3]).sum())
            same = ours[3] == theirs[3]
            corr_diff = float((ours[1] - theirs[1])[same].abs().max())
            a = measure(lambda: matching.tfmr_match(fx, fy, src, tgt, x_ol, p, k), args.reps, args.warmup)
            t = measure(lambda: matching.similarity_topk(fx, fy, k), args.reps, args.warmup)
            b = measure(lambda: t_match(fx, fy, src, tgt, x_ol, p, k), args.reps, args.warmup)
            row = {"B": B, "N1": N1, "M1": M1, "C": C, "k": k, "top_prob": p, "library": a,
                   "library_similarity_topk_only": t, "torch": b,
                   "scratch_bytes": int(_lib.load().pcr_tfmr_scratch_bytes(B, N1, M1, C, k)),
                   "speedup": b["median_ms"] / a["median_ms"],
                   "selection_places_that_differ": differ, "max_abs_tgt_corr_diff_on_equal_rows": corr_diff}
            rows.append(row)
            print(json.dumps(row), flush=True)
    summary = {"device": torch.cuda.get_device_name(0), "rows": rows}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(summary, fh, indent=1)
    print(json.dumps({"tfmr_bench": "done", "configurations": len(rows)}))


if __name__ == "__main__":
    main()
