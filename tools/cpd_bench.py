#!/usr/bin/env python
"""Time the CPD E-step (pointcloudregistration_amd.cpd.expectation_step) and the
full rigid + scale registration (cpd.register_batch) beside probreg's wording
of the same steps as a torch tensor program on the same GPU and the same data.

E-step shapes (P, M, N): (1, 1024, 1024), (1, 8192, 8192), (64, 1024, 1024),
(256, 1024, 1024); registration: P = 64 at 1024 x 1024, 50 fixed iterations.

The torch side forms the dense (P, M, N) matrix as probreg does: squared
distances, exp, column sums, the FLT_EPSILON rule, one divide, two reductions
and a bmm, in f32.  Before anything is timed both are compared with the same
program in f64 on the contract's f32 distances: the library may be at most 4 times as far from
f64 as the f32 torch program, floored at 4 * 2^-24 (the rule of
tests/test_cpd_gpu.py); the errors are reported, a row that misses the rule is
flagged ("outputs_agree": false) and the tool then exits with status 1: a time
beside outputs that disagree is not a result.  The registration row is held to
the loop rule of the tests in the same way (the library at most 4 times as far
from the f64 torch loop as the f32 torch loop is, floored at 2^-20).

Method: warm-up calls, then the median of per-call HIP-event times, the Python
call included; peak memory is torch's allocator peak over one call (the
library's scratch is a torch byte tensor, so the peak contains it; its size is
also reported).  The sweeps' rate is 2 P M N exponentials over the E-step time,
set against the vector-issue bound of the kernels' own instruction count:
per pair evaluation the column sweep issues 10.75 plain f32 instructions, one
v_exp_f32 and 0.5 f64 instructions (a conversion and an add per group of four),
the row sweep 15.75, one and 2.5 (csrc/cpd.hip), at 4 issue cycles a wave for
plain f32 and 8 for v_exp_f32 and for f64 (half rate; the f32 -> f64 conversion
is counted at that rate too): 146 cycles per wave for two exponentials of 64
lanes.
One JSON line per configuration.

    python tools/cpd_bench.py [--reps 50] [--warmup 10] [--out FILE]
"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pointcloudregistration_amd import _lib, cpd  # noqa: E402

FLT_EPSILON = 2.0 ** -23
ISSUE_CYCLES_PER_PAIR = (10.75 + 15.75) * 4 + 2 * 8 + (0.5 + 2.5) * 8      # both sweeps, one wave
SIMDS, CLOCK_HZ, WAVE = 256 * 4, 2.4e9, 64
ISSUE_BOUND_EXPS = 2 * SIMDS * CLOCK_HZ * WAVE / ISSUE_CYCLES_PER_PAIR


def sqdist(ts, tgt, dtype):
    """The contract's f32 squared distances (P, M, N), then cast to `dtype`."""
    dx = ts[:, :, None, 0] - tgt[:, None, :, 0]
    dy = ts[:, :, None, 1] - tgt[:, None, :, 1]
    dz = ts[:, :, None, 2] - tgt[:, None, :, 2]
    return ((dx * dx + dy * dy) + dz * dz).to(dtype)


def t_estep(ts, tgt, sigma2, w, dtype=torch.float32):
    """probreg's dense E-step on f32 (P, M, 3), (P, N, 3), every array after the
    distances in `dtype`."""
    M, N = ts.shape[1], tgt.shape[1]
    pmat = torch.exp(-sqdist(ts, tgt, dtype) / (2.0 * sigma2))
    tgt = tgt.to(dtype)
    den = pmat.sum(1)
    den = torch.where(den == 0, torch.full_like(den, FLT_EPSILON), den)
    r = den + (2.0 * math.pi * sigma2) ** 1.5 * w / (1.0 - w) * M / N
    pmat = pmat / r[:, None, :]
    p1 = pmat.sum(2)
    return den / r, p1, torch.bmm(pmat, tgt), p1.sum(1)


def t_register(src, tgt, w, iters, dtype=torch.float32):
    """Rigid + scale CPD of P pairs: the dense E-step above in `dtype` and the M-step
    of the contract in f64 (batched SVD), `iters` fixed iterations, no host reads."""
    P, M, _ = src.shape
    N = tgt.shape[1]
    Y, X = src.double(), tgt.double()
    xc, yc = X - X[:, :1], Y - X[:, :1]
    sigma2 = (M * (xc * xc).sum((1, 2)) + N * (yc * yc).sum((1, 2)) - 2.0 * (xc.sum(1) * yc.sum(1)).sum(1)) / (3.0 * M * N)
    B = torch.eye(3, dtype=torch.float64, device=src.device).repeat(P, 1, 1)
    t = torch.zeros(P, 3, dtype=torch.float64, device=src.device)
    for _ in range(iters):
        ts = (Y @ B.transpose(1, 2) + t[:, None, :]).float()
        s2 = sigma2.to(dtype)[:, None, None]
        pmat = torch.exp(-sqdist(ts, tgt, dtype) / (2.0 * s2))
        den = pmat.sum(1)
        den = torch.where(den == 0, torch.full_like(den, FLT_EPSILON), den)
        r = den + ((2.0 * math.pi * sigma2) ** 1.5 * w / (1.0 - w) * M / N).to(dtype)[:, None]
        pmat = pmat / r[:, None, :]
        pt1, p1, px = (den / r).double(), pmat.sum(2).double(), torch.bmm(pmat, tgt.to(dtype)).double()
        n_p = p1.sum(1)
        mux, muy = px.sum(1) / n_p[:, None], (Y * p1[:, :, None]).sum(1) / n_p[:, None]
        Yc, Xc = Y - muy[:, None, :], X - mux[:, None, :]
        A = px.transpose(1, 2) @ Yc - mux[:, :, None] * (p1[:, :, None] * Yc).sum(1)[:, None, :]
        U, _, Vt = torch.linalg.svd(A)
        C = torch.ones(P, 3, dtype=torch.float64, device=src.device)
        C[:, 2] = torch.linalg.det(U @ Vt)
        R = U @ torch.diag_embed(C) @ Vt
        tr_ar = (A * R).sum((1, 2))
        tr_g = (p1 * (Yc * Yc).sum(2)).sum(1)
        scale = tr_ar / tr_g
        sigma2 = ((pt1 * (Xc * Xc).sum(2)).sum(1) - scale * tr_ar) / (3.0 * n_p)
        sigma2 = torch.clamp(sigma2, min=FLT_EPSILON)
        B = scale[:, None, None] * R
        t = mux - (B @ muy[:, :, None])[:, :, 0]
    return B, t, sigma2


def rel_err(a, b):
    return float((a.double() - b).abs().max() / b.abs().max())


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


def make(P, M, N, seed):
    gen = torch.Generator().manual_seed(seed)
    src = torch.rand(P, M, 3, generator=gen)
    pick = torch.randint(0, M, (P, N), generator=gen)
    tgt = torch.gather(src, 1, pick[:, :, None].expand(P, N, 3)) + 0.02 * torch.randn(P, N, 3, generator=gen)
    return src.cuda(), tgt.cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("cpd_bench: no GPU (times are only meaningful on the device)")
    lib = _lib.load()
    sigma2, w = 0.01, 0.1
    rows = []
    for P, M, N in ((1, 1024, 1024), (1, 8192, 8192), (64, 1024, 1024), (256, 1024, 1024)):
        src, tgt = make(P, M, N, P + M)
        ours = cpd.expectation_step(src, tgt, sigma2, w)
        theirs = t_estep(src, tgt, sigma2, w)
        want = t_estep(src, tgt, sigma2, w, torch.float64)
        errs = {}
        for name, o, t, r in zip(("pt1", "p1", "px", "n_p"), ours, theirs, want):
            e_lib, e_torch = rel_err(o, r), rel_err(t, r)
            errs[name] = {"library": e_lib, "torch_f32": e_torch, "within": e_lib <= max(4 * e_torch, 4 * 2.0 ** -24)}
        agree = all(e["within"] for e in errs.values())
        del want, theirs, ours
        torch.cuda.empty_cache()
        a = measure(lambda: cpd.expectation_step(src, tgt, sigma2, w), args.reps, args.warmup)
        b = measure(lambda: t_estep(src, tgt, sigma2, w), args.reps, args.warmup)
        rate = 2.0 * P * M * N / (a["median_ms"] * 1e-3)
        row = {"what": "estep", "P": P, "M": M, "N": N, "library": a, "torch": b,
               "scratch_bytes": int(lib.pcr_cpd_scratch_bytes(P, M, N)), "speedup": b["median_ms"] / a["median_ms"],
               "exps_per_s": rate, "issue_bound_exps_per_s": ISSUE_BOUND_EXPS,
               "issue_cycles_per_pair_evaluation": ISSUE_CYCLES_PER_PAIR,
               "share_of_issue_bound": rate / ISSUE_BOUND_EXPS, "outputs_agree": agree, "errors_vs_f64": errs}
        rows.append(row)
        print(json.dumps(row), flush=True)

    P, M, N, iters = 64, 1024, 1024, 50
    src, tgt = make(P, M, N, 7)
    ours = cpd.register_batch(src, tgt, kind="rigid_scale", w=w, maxiter=iters, tol=0.0)
    Bt, tt, s2t = t_register(src, tgt, w, iters)
    Bw, tw, s2w = t_register(src, tgt, w, iters, torch.float64)
    ob, ot = ours.transformation[:, :3, :3], ours.transformation[:, :3, 3]
    errs = {"T": {"library": float(max((ob - Bw).abs().max(), (ot - tw).abs().max())),
                  "torch_f32": float(max((Bt - Bw).abs().max(), (tt - tw).abs().max()))},
            "sigma2_rel": {"library": float(((ours.sigma2 - s2w) / s2w).abs().max()),
                           "torch_f32": float(((s2t - s2w) / s2w).abs().max())}}
    for e in errs.values():
        e["within"] = e["library"] <= max(4 * e["torch_f32"], 2.0 ** -20)
    agree = all(e["within"] for e in errs.values())
    del Bw, tw, s2w
    torch.cuda.empty_cache()
    a = measure(lambda: cpd.register_batch(src, tgt, kind="rigid_scale", w=w, maxiter=iters, tol=0.0), args.reps, args.warmup)
    b = measure(lambda: t_register(src, tgt, w, iters), args.reps, args.warmup)
    row = {"what": "register rigid+scale", "P": P, "M": M, "N": N, "iterations": iters, "library": a, "torch": b,
           "scratch_bytes": int(lib.pcr_cpd_scratch_bytes(P, M, N)), "speedup": b["median_ms"] / a["median_ms"],
           "exps_per_s": 2.0 * P * M * N * iters / (a["median_ms"] * 1e-3), "issue_bound_exps_per_s": ISSUE_BOUND_EXPS,
           "outputs_agree": agree, "errors_vs_f64_loop": errs}
    rows.append(row)
    print(json.dumps(row), flush=True)
    summary = {"device": torch.cuda.get_device_name(0), "rows": rows}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(summary, fh, indent=1)
    bad = [(r["what"], r["P"], r["M"], r["N"]) for r in rows if not r["outputs_agree"]]
    print(json.dumps({"cpd_bench": "done", "configurations": len(rows), "rows_whose_outputs_disagree": bad}))
    if bad:
        sys.exit(1)


if __name__ == "__main__":
    main()
