#!/usr/bin/env python
"""Time the fused unary family (pointcloudregistration_amd.ngenet) beside the path a
user had before it, on the same GPU: the torch composite of the reference's blocks
(Linear -> unsqueeze / permute / contiguous -> InstanceNorm1d -> permute /
contiguous -> (+ residual) -> LeakyReLU, and index + torch.cat in front of it in
the decoder) with the same weights.

Shapes: every distinct unary shape of the MRI architecture (first_feats_dim 128,
levels 128 .. 1024, gnn_feats_dim 256, decoder 770 -> 129, 385 -> 64, 192 -> 34)
at a pair of 2 x 10k points, the pyramid's levels taken as 20000, 5000, 1250 and
320 stacked points (a quarter per stride).

Per shape: median, min and max of per-call HIP-event times of both sides, the
allocator's peak over one call, the bytes the fused passes move (pass 1 reads the
operand and writes y, pass 3 reads and writes out; the weight and the partials
are small beside them), the achieved fraction of the f32-MFMA rate (256 flop per
cycle and CU on v_mfma_f32_32x32x2_f32), and whether the two sides agree.

Then the whole forward: a network with the architecture's real widths -- the
KPConv blocks on a synthetic pyramid of those sizes, the interaction block a stub
of two Conv1ds (it is not part of this family and has its own benchmarks) --
through ngenet.forward after ngenet.fuse, beside the torch forward of the same
network; kpconv.fuse is applied to both, so the convolutions are the fused ones
on either side.

Method: warm-up calls, then per-call HIP-event times in one process: median, min
and max.

    python tools/unary_bench.py [--reps 30] [--warmup 5] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
from pointcloudregistration_amd import kpconv, ngenet  # noqa: E402
import unary_blocks as ub  # noqa: E402  (reference-shaped composites)
import unary_cases as uc  # noqa: E402

F = torch.nn.functional
LEVELS = (20000, 5000, 1250, 320)
FIRST, GNN, FINAL = 128, 256, 32
ARCH = ["simple", "resnetb", "resnetb_strided", "resnetb", "resnetb", "resnetb_strided", "resnetb", "resnetb",
        "resnetb_strided", "resnetb", "resnetb"]
MFMA_FLOPS = 256 * 256 * 2.4e9     # 256 CUs x 256 flop / cycle x 2.4 GHz


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
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return {"median_ms": statistics.median(times), "min_ms": min(times), "max_ms": max(times), "reps": reps,
            "peak_bytes": int(peak)}


def composite(x0, w, gather, x1, bias, norm, act, res):
    """The reference's blocks one by one (blocks.py:145-174, 191-199, 290)."""
    x = x0 if gather is None else x0[gather]
    if x1 is not None:
        x = torch.cat([x, x1], dim=1)
    y = F.linear(x, w) if w is not None else x
    if norm:
        y = torch.unsqueeze(y, 0).permute(0, 2, 1).contiguous()
        y = F.instance_norm(y, eps=1e-5)
        y = torch.squeeze(y.permute(0, 2, 1), 0).contiguous()
    elif bias is not None:
        y = y + bias
    if res is not None:
        y = y + res
    return F.leaky_relu(y, 0.1) if act else y


def shapes():
    """(label, n, m0, c0, c1, cout, weight, norm, act, res): the distinct calls of one forward."""
    out = []
    width = FIRST // 2
    out.append(("simple bn+lrelu", LEVELS[0], None, width, 0, width, False, True, True, False))
    level, in_dim, out_dim = 0, width, FIRST
    for name in ARCH[1:]:
        n_in = LEVELS[level]
        n_out = LEVELS[level + 1] if "strided" in name else n_in
        mid = out_dim // 4
        tag = f"L{level} {name} {in_dim}->{out_dim}"
        if in_dim != mid:
            out.append((f"{tag} unary1", n_in, None, in_dim, 0, mid, True, True, True, False))
        out.append((f"{tag} bn+lrelu", n_out, None, mid, 0, mid, False, True, True, False))
        out.append((f"{tag} unary2+res+lrelu", n_out, None, mid, 0, out_dim, True, True, True, True))
        if in_dim != out_dim:
            out.append((f"{tag} shortcut", n_out, None, in_dim, 0, out_dim, True, True, False, False))
        in_dim = out_dim
        if "strided" in name:
            level, out_dim = level + 1, out_dim * 2
    for branch, plan in zip("hml", uc.decoder_plan(FIRST, GNN)):
        lvl = 3 if branch == "h" else None
        pend = False
        for name, cin, cout, layer in plan:
            if name == "nearest_upsample":
                pend, lvl = True, layer
                continue
            if lvl is None or not pend:
                lvl = layer
            co = cout if name == "unary" else FINAL + (0 if cout == -1 else 2)
            n = LEVELS[lvl]
            last = name == "last_unary"
            if pend:
                c1 = [FIRST, 2 * FIRST, 4 * FIRST][lvl]
                out.append((f"dec {branch} up+cat+{name} {cin}->{co}", n, LEVELS[lvl + 1], cin - c1, c1, co, True,
                            not last, not last, False))
            else:
                out.append((f"dec {branch} {name} {cin}->{co}", n, None, cin, 0, co, True, not last, not last, False))
            pend = False
    seen, uniq = set(), []
    for s in out:
        if s[1:] not in seen:
            seen.add(s[1:])
            uniq.append(s)
    return uniq


class Net(torch.nn.Module):
    """NgeNet's submodules at the architecture's widths on reference-shaped blocks, the interaction a stub."""

    def __init__(self):
        super().__init__()
        nn = torch.nn
        blocks, self.encoder_skips = [], []
        in_dim, out_dim, level = 1, FIRST, 0
        for i, name in enumerate(ARCH):
            if "strided" in name:
                self.encoder_skips.append(i)
            cls = ub.SimpleBlock if name == "simple" else ub.ResnetBottleneckBlock
            blocks.append(cls(name, in_dim, out_dim, 1.0, True, 0.02, level, 15, 0.1))
            in_dim = out_dim // 2 if name == "simple" else out_dim
            if "strided" in name:
                level, out_dim = level + 1, out_dim * 2
        self.encoder_blocks = nn.ModuleList(blocks)
        self.decoder_skips = [12, 14, 16]
        self.bottleneck = nn.Conv1d(in_dim, GNN, 1)
        self.info_interative = ub.Interact(GNN)
        self.pro_gnn, self.attn_score = nn.Conv1d(GNN, GNN, 1), nn.Conv1d(GNN, 1, 1)
        self.epsilon = nn.Parameter(torch.tensor(-5.0))
        mk = lambda b: ub.decider(*b, final=FINAL)  # noqa: E731
        h, m, lo = uc.decoder_plan(FIRST, GNN)
        self.decoder_blocks = nn.ModuleList(mk(b) for b in h)
        self.decoder_blocks_m = nn.ModuleList(mk(b) for b in m)
        self.decoder_blocks_l = nn.ModuleList(mk(b) for b in lo)
        for mod in self.modules():
            if isinstance(mod, ub.KPConv):
                nn.init.kaiming_uniform_(mod.weights, a=5 ** 0.5)
                mod.kernel_points.data = 0.03 * torch.randn(15, 3)

    def forward(self, inputs):
        """NgeNet.forward's data flow on torch ops (the decoder's three branches written out)."""
        feats, skips = inputs["feats"], []
        for i, block in enumerate(self.encoder_blocks):
            if i in self.encoder_skips:
                skips.append(feats)
            feats = block(feats, inputs)
        n_src = int(inputs["stacked_lengths"][-1][0])
        feats = self.bottleneck(feats.t().unsqueeze(0))
        cf = lambda t: t.t().unsqueeze(0)  # noqa: E731
        pts, nrm = inputs["points"][-1], inputs["normals"][-1]
        a, b = self.info_interative(cf(pts[:n_src]), feats[..., :n_src], cf(pts[n_src:]), feats[..., n_src:],
                                    cf(nrm[:n_src]), cf(nrm[n_src:]))
        feats = self.pro_gnn(torch.cat([a, b], -1))
        attn = self.attn_score(feats).squeeze(0).t()
        temp = torch.exp(self.epsilon) + 0.03
        fn = (feats / (feats.norm(dim=1, keepdim=True) + 1e-8)).squeeze(0).t()
        inner = fn[:n_src] @ fn[n_src:].t()
        ol = torch.cat([torch.softmax(inner / temp, 1) @ attn[n_src:],
                        torch.softmax(inner.t() / temp, 1) @ attn[:n_src]])
        x = torch.cat([feats.squeeze(0).t(), attn, ol], 1)
        hb, mb, lb = self.decoder_blocks, self.decoder_blocks_m, self.decoder_blocks_l
        s0, s1, s2 = skips
        x = hb[1](torch.cat([hb[0](x, inputs), s2], 1))
        x = hb[3](torch.cat([hb[2](x, inputs), s1], 1))
        x = hb[5](torch.cat([hb[4](x, inputs), s0], 1))
        m = mb[0](s2)
        m = mb[2](torch.cat([mb[1](m, inputs), s1], 1))
        m = mb[4](torch.cat([mb[3](m, inputs), s0], 1))
        lo = lb[0](s1)
        lo = lb[2](torch.cat([lb[1](lo, inputs), s0], 1))
        out_h = torch.cat([x[:, :-2] / x[:, :-2].norm(dim=1, keepdim=True), torch.sigmoid(x[:, -2:-1]),
                           torch.sigmoid(x[:, -1:])], 1)
        return out_h, m / m.norm(dim=1, keepdim=True), lo / lo.norm(dim=1, keepdim=True)


def pyramid(gen, k=32):
    """A synthetic pyramid of LEVELS stacked points: neighbour tables of k random rows of the same cloud."""
    inp = {"points": [], "normals": [], "stacked_lengths": [], "neighbors": [], "pools": [], "upsamples": []}
    for n in LEVELS:
        inp["points"].append((0.05 * torch.rand(n, 3, generator=gen)).cuda())
        inp["normals"].append(F.normalize(torch.randn(n, 3, generator=gen), dim=-1).cuda())
        inp["stacked_lengths"].append(torch.tensor([n // 2, n - n // 2]))
        inp["neighbors"].append(torch.randint(0, n, (n, k), generator=gen).cuda())
    for l in range(3):
        inp["pools"].append(torch.randint(0, LEVELS[l], (LEVELS[l + 1], k), generator=gen).cuda())
        inp["upsamples"].append(torch.randint(0, LEVELS[l + 1], (LEVELS[l], k), generator=gen).cuda())
    inp["feats"] = torch.ones(LEVELS[0], 1).cuda()
    return inp


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("unary_bench: no GPU (times are only meaningful on the device)")
    torch.manual_seed(0)
    gen = torch.Generator().manual_seed(0)
    rows = []
    with torch.no_grad():
        for label, n, m0, c0, c1, cout, weight, norm, act, res in shapes():
            x0 = torch.randn(m0 or n, c0, generator=gen).cuda()
            g = torch.randint(0, m0, (n,), generator=gen).cuda() if m0 else None
            x1 = torch.randn(n, c1, generator=gen).cuda() if c1 else None
            w = (torch.randn(cout, c0 + c1, generator=gen) / (c0 + c1) ** 0.5).cuda() if weight else None
            bias = None if norm else torch.randn(cout, generator=gen).cuda()
            r = torch.randn(n, cout, generator=gen).cuda() if res else None
            kw = dict(gather=g, x1=x1, bias=bias, norm=norm, act=act, residual=r)
            ours = (lambda: ngenet.unary_forward(x0, w, **kw)) if weight else (lambda: ngenet.norm_act(x0, **kw))
            theirs = lambda: composite(x0, w, g, x1, bias, norm, act, r)  # noqa: E731
            diff = float((ours() - theirs()).abs().max())
            a, b = measure(ours, args.reps, args.warmup), measure(theirs, args.reps, args.warmup)
            flops = 2 * n * (c0 + c1) * cout if weight else 0
            moved = 4 * n * ((c0 + c1) + cout + (2 * cout if norm else 0) + (cout if res else 0))
            row = {"op": label, "n": n, "cin": c0 + c1, "cout": cout, "fused": a, "torch": b,
                   "speedup": b["median_ms"] / a["median_ms"], "max_abs_diff": diff, "fused_bytes": moved,
                   "fused_gbps": moved / (a["median_ms"] * 1e-3) / 1e9,
                   "mfma_fraction": flops / (a["median_ms"] * 1e-3) / MFMA_FLOPS,
                   "slower": a["median_ms"] > b["median_ms"]}
            rows.append(row)
            print(json.dumps(row), flush=True)

        net = Net().cuda().eval()
        inputs = pyramid(gen)
        kpconv.fuse(net)
        plain = measure(lambda: net(inputs), args.reps, args.warmup)
        want = net(inputs)
        counts = ngenet.fuse(net)
        fused = measure(lambda: ngenet.forward(net, inputs), args.reps, args.warmup)
        got = ngenet.forward(net, inputs)
        row = {"op": "whole forward (stub interaction, synthetic pyramid)", "swapped": counts, "fused": fused,
               "torch": plain, "speedup": plain["median_ms"] / fused["median_ms"],
               "max_abs_diff": max(float((a - b).abs().max()) for a, b in zip(got, want))}
        rows.append(row)
        print(json.dumps(row), flush=True)

    summary = {"device": torch.cuda.get_device_name(0), "rows": rows}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(summary, fh, indent=1)
    print(json.dumps({"unary_bench": "done", "ops": len(rows)}))


if __name__ == "__main__":
    main()
