#!/usr/bin/env python3
"""CPU replay of the RANSAC sweep's grid walk on the benchmark's own workload
(synth.make_batch(.., base_seed=1000), d = 0.04): candidates a query examines
under the hashed 2.01 r grid and under r-wide cells, with and without hash
collisions ("Round 7: dense r-cell grid").  numpy only.

  python3 tools/grid_candidates_replay.py [--pairs 4] [--identity]

Per layout: mean candidates per query (c_bar), their 99th percentile, the mean
over 64-query chunks (queries in cell order) of the chunk's maximum -- a wave
runs as long as its longest lane -- and the cells tested / non-empty per query.
--identity replays a wrong hypothesis (the identity) instead of the true transform.
"""
import argparse
import itertools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pointcloudregistration_amd import synth  # noqa: E402


def murmur_slot(cx, cy, cz, S):
    k = ((cx & 1023) | ((cy & 1023) << 10) | ((cz & 1023) << 20)).astype(np.uint64)
    m32 = np.uint64(0xFFFFFFFF)
    k ^= k >> np.uint64(16)
    k = (k * np.uint64(0x85EBCA6B)) & m32
    k ^= k >> np.uint64(13)
    k = (k * np.uint64(0xC2B2AE35)) & m32
    k ^= k >> np.uint64(16)
    return ((k * np.uint64(S)) >> np.uint64(32)).astype(np.int64)


def walk(q, tgt, r, factor, S):
    """per query: candidates, cells tested, cells non-empty.  S: hash slots, or None
    for a collision-free table."""
    cell = factor * r
    thr = float(np.float32(r * r)) * (1 + 1e-6)
    ct = np.floor(tgt.astype(np.float64) / cell).astype(np.int64)
    if S is None:
        lo = ct.min(0)
        D = ct.max(0) - lo + 1
        pop = np.bincount(((ct[:, 2] - lo[2]) * D[1] + (ct[:, 1] - lo[1])) * D[0] + (ct[:, 0] - lo[0]),
                          minlength=int(D.prod()))
    else:
        pop = np.bincount(murmur_slot(ct[:, 0], ct[:, 1], ct[:, 2], S), minlength=S)
    u, w = q / cell, 1.001 * r / cell
    c0, c1 = np.floor(u - w).astype(np.int64), np.floor(u + w).astype(np.int64)
    span = int((c1 - c0).max()) + 1
    cand = np.zeros(len(q), np.int64)
    tested = np.zeros(len(q), np.int64)
    full = np.zeros(len(q), np.int64)
    for off in itertools.product(range(span), repeat=3):
        c = c0 + np.array(off)
        gap = np.maximum(np.maximum(c * cell - q, q - (c + 1) * cell), 0.0)
        keep = (c <= c1).all(1) & ((gap * gap).sum(1) <= thr)
        if S is None:
            rel = c - lo
            inside = keep & (rel >= 0).all(1) & (rel < D).all(1)
            rel = np.where(inside[:, None], rel, 0)
            n = np.where(inside, pop[(rel[:, 2] * D[1] + rel[:, 1]) * D[0] + rel[:, 0]], 0)
        else:
            n = np.where(keep, pop[murmur_slot(c[:, 0], c[:, 1], c[:, 2], S)], 0)
        cand += n
        tested += keep
        full += n > 0
    return cand, tested, full


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=4)
    ap.add_argument("--points", type=int, default=8192)
    ap.add_argument("--identity", action="store_true")
    a = ap.parse_args()
    r = 0.04
    B = synth.make_batch(a.pairs, n=a.points, m=a.points, d=32, base_seed=1000, feat_noise=1.0)
    layouts = [("2.01 r cells, murmur hash, S = 12288", 2.01, 12288),
               ("2.01 r cells, no collisions", 2.01, None),
               ("1.005 r cells, culled, hashed S = 12288", 1.005, 12288),
               ("1.005 r cells, culled, hashed S = 16384", 1.005, 16384),
               ("1.005 r cells, culled, no collisions", 1.005, None)]
    for p in range(a.pairs):
        src, tgt = B.src[p].astype(np.float64), B.tgt[p]
        q = src if a.identity else src @ B.R[p].T + B.t[p]
        # the sweep's order: queries of neighbouring cells share a wave
        key = np.floor(q / (2.01 * r)).astype(np.int64)
        q = q[np.lexsort((key[:, 0], key[:, 1], key[:, 2]))]
        print(f"pair {p} ({'identity' if a.identity else 'true transform'})")
        print(f"  {'layout':42s} {'c_bar':>6s} {'p99':>5s} {'max/64':>7s} {'cells':>6s} {'non-empty':>9s}")
        for name, f, S in layouts:
            c, t, n = walk(q, tgt, r, f, S)
            pad = (-len(c)) % 64
            wmax = np.pad(c, (0, pad)).reshape(-1, 64).max(1).mean()
            print(f"  {name:42s} {c.mean():6.1f} {np.percentile(c, 99):5.0f} {wmax:7.1f} {t.mean():6.1f} {n.mean():9.1f}")


if __name__ == "__main__":
    main()
