"""Chamfer-stage (a1) microbenchmark: nnd_with_index on P pairs of N points, at
256 / 64 / 32 pairs by default, device events around the calls and the
library's profile slots for the kernels inside.  Prints one JSON line per pair
count and query kernel.  PCR_LIB selects the library (tools/ab.sh custom);
--query l2 lds times both query kernels in one process (PCR_NND_QUERY is read
per call), without it the environment's choice stands."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pointcloudregistration_amd import _lib, nndistance as nd, synth  # noqa: E402


def make_clouds(pairs, n, seed, data):
    """surface: the bench's synthetic pairs (synth.make_pair) with the source
    moved by the ground-truth motion, which is what the step's Chamfer sees
    after ICP -- two samplings of one surface, most answers certified within a
    ring or two; 32 distinct pairs, tiled.  uniform: two independent uniform
    clouds in the unit cube, where nearly every query walks to ring 2."""
    if data == "uniform":
        g = torch.Generator(device="cuda").manual_seed(seed)
        return (torch.rand(pairs, n, 3, device="cuda", generator=g),
                torch.rand(pairs, n, 3, device="cuda", generator=g))
    distinct = min(pairs, 32)
    b = synth.make_batch(distinct, n=n, m=n, d=1, base_seed=1000 + seed)
    src = torch.from_numpy(b.src).cuda().double()
    R, t = torch.from_numpy(b.R).cuda(), torch.from_numpy(b.t).cuda()
    x1 = (src @ R.transpose(1, 2) + t[:, None, :]).float()
    x2 = torch.from_numpy(b.tgt).cuda()
    rep = -(-pairs // distinct)
    return x1.repeat(rep, 1, 1)[:pairs].contiguous(), x2.repeat(rep, 1, 1)[:pairs].contiguous()


def run_one(x1, x2, iters, data):
    out = nd.nnd_with_index(x1, x2)   # warm-up: workspace, code objects
    torch.cuda.synchronize()
    _lib.profile_enable(True)
    for pid in range(_lib.PROF_SLOTS):
        _lib.profile_read(pid, reset=True)
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record()
    for _ in range(iters):
        out = nd.nnd_with_index(x1, x2)
    ev1.record()
    torch.cuda.synchronize()
    prof = {name: _lib.profile_read(pid)[0] / iters for name, pid in
            (("nnd_forward", _lib.PROF_NND_FWD), ("nnd_grid_query", _lib.PROF_NND_GRID))}
    _lib.profile_enable(False)
    d1, d2, i1, i2 = out
    return {"pairs": x1.shape[0], "n": x1.shape[1], "data": data, "iters": iters,
            "ms_total": ev0.elapsed_time(ev1) / iters, "ms": prof,
            "query": os.environ.get("PCR_NND_QUERY", "auto"), "lib": os.path.basename(_lib.LIB_PATH),
            # a fingerprint of the results, equal between libraries and kernels that compute the same
            "checksum": [float(d1.double().sum()), float(d2.double().sum()), int(i1.long().sum()), int(i2.long().sum())]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, nargs="+", default=[256, 64, 32])
    ap.add_argument("--n", type=int, default=8192)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--data", choices=("surface", "uniform"), default="surface")
    ap.add_argument("--query", nargs="+", choices=("auto", "l2", "lds"), default=None)
    a = ap.parse_args()
    for p in a.pairs:
        x1, x2 = make_clouds(p, a.n, a.seed, a.data)
        for q in a.query or [None]:
            if q is not None:
                os.environ["PCR_NND_QUERY"] = q
            print(json.dumps(run_one(x1, x2, a.iters, a.data)), flush=True)


if __name__ == "__main__":
    main()
