"""Generate tests/golden/unary_golden.npz by IMPORTING the reference's own Python
code (read-only, no bytecode written) in the build container.  The file holds
only what the reference returned; the inputs come from unary_cases.py.

  UnaryBlock, BatchNormBlock, NearestUpsampleBlock, MaxPoolBlock, block_decider
      c2p-net/ngenet/models/KPConv/blocks.py:135-199, 293-327 (instantiated: they read no files)
  SimpleBlock.forward, ResnetBottleneckBlock.forward, KPConv.forward
      blocks.py:222-233, 271-290, 73-128, called UNBOUND on a types.SimpleNamespace: KPConv's
      constructor (load_kernels) would create a directory inside the reference tree
  NgeNet.forward   c2p-net/ngenet/models/NgeNet.py:132-221, unbound on the tiny network
      (unary_blocks.TinyNet) built from the reference's blocks

`open3d` is not installed: an EMPTY placeholder module satisfies the top-level
`import open3d` (nothing used here calls into it).

Keys:
  unary/<case>            (n, cout)   UnaryBlock.forward
  upcat/<case>            (n, cout)   UnaryBlock(cat([NearestUpsampleBlock(x0), x1]))
  block/<case>/conv_in    (m, mid)    what the block handed its KPConv (blocks with a unary1)
  block/<case>/conv_out   (n, mid)    what KPConv.forward returned
  block/<case>/out        (n, out)    the block's forward
  net/h, net/m, net/l     NgeNet.forward's three outputs on the tiny network
  net/deviation           max |f32 - f64| of the same forward run in f64 (the wiring test allows 8 x)

Every single-block output is asserted to lie within the restatement's bound
(tests/unary_ref.py).

    python tests/golden/make_golden_unary.py
"""
import os
import sys
import types

sys.dont_write_bytecode = True
os.environ["PYTHONDONTWRITEBYTECODE"] = "1"
import numpy as np  # noqa: E402
import torch  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.modules.setdefault("open3d", types.ModuleType("open3d"))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import unary_blocks as ub  # noqa: E402
import unary_cases as uc  # noqa: E402
import unary_ref as ur  # noqa: E402

WIRING_FACTOR = 8


def _imp_reference():
    sys.path.insert(0, f"{REF}/c2p-net")
    from ngenet.models.KPConv import blocks
    from ngenet.models.NgeNet import NgeNet
    return blocks, NgeNet


def _t(a):
    return None if a is None else torch.from_numpy(a)


def _unary(blocks, w, bias, relu):
    blk = blocks.UnaryBlock(w.shape[1], w.shape[0], bias is None, 0.02, relu=relu)
    sd = {"mlp.weight": _t(w)}
    if bias is not None:
        sd["bn.bias"] = _t(bias)
    blk.load_state_dict(sd, strict=True)
    return blk.eval()


def _bn(blocks, dim, bias):
    bn = blocks.BatchNormBlock(dim, bias is None, 0.02)
    if bias is not None:
        bn.load_state_dict({"bias": _t(bias)}, strict=True)
    return bn.eval()


def reference_block(blocks, name, rec):
    """The block's forward, unbound on a namespace whose KPConv records what goes through it."""
    kind, in_dim, out_dim, use_bn = uc.BLOCKS[name]
    c = uc.make_block(name)
    p = c["params"]
    conv = types.SimpleNamespace(kernel_points=_t(p["KPConv.kernel_points"]), weights=_t(p["KPConv.weights"]),
                                 KP_extent=c["extent"], KP_influence="linear", aggregation_mode="sum",
                                 K=p["KPConv.kernel_points"].shape[0])

    def kpconv(q, s, f, idx):
        out = blocks.KPConv.forward(conv, q, s, f, idx)
        rec["conv_in"], rec["conv_out"] = f.numpy().copy(), out.numpy().copy()
        return out

    mid = p["KPConv.weights"].shape[2]
    ns = types.SimpleNamespace(block_name=kind, layer_ind=0, KPConv=kpconv, bn=_bn(blocks, mid, p.get("bn.bias")),
                               leaky_relu=torch.nn.LeakyReLU(0.1))
    batch = {k: [_t(a) for a in v] for k, v in c["batch"].items()}
    if kind == "simple":
        return blocks.SimpleBlock.forward(ns, _t(c["f"]), batch).numpy(), c
    for u, relu in (("unary1", True), ("unary2", False), ("unary_shortcut", False)):
        w = p.get(f"{u}.mlp.weight")
        setattr(ns, u, torch.nn.Identity() if w is None else _unary(blocks, w, None, relu))
    ns.max_pool = blocks.MaxPoolBlock(0)
    return blocks.ResnetBottleneckBlock.forward(ns, _t(c["f"]), batch).numpy(), c


def main():
    blocks, NgeNet = _imp_reference()
    out, worst = {}, 0.0

    def check(key, got, want, bound):
        nonlocal worst
        r = ur.ratio(got, want, bound)
        worst = max(worst, r)
        print(f"{key}: shape {got.shape}, max err / bound = {r:.4f}")
        assert r <= 1, (key, r)

    with torch.no_grad():
        for name, (n, cin, cout, use_bn, relu) in uc.UNARY.items():
            c = uc.make_unary(name)
            ref = _unary(blocks, c["w"], c["bias"], relu)(_t(c["x"])).numpy()
            want, bound, _ = ur.unary(c["w"], c["x"], bias=c["bias"], norm=use_bn, eps=uc.EPS, slope=uc.SLOPE, act=relu)
            check(f"unary/{name}", ref, want, bound)
            out[f"unary/{name}"] = ref
        for name, (m0, n, c0, c1, cout, use_bn, relu) in uc.UPCAT.items():
            c = uc.make_upcat(name)
            up = blocks.NearestUpsampleBlock(0)(_t(c["x0"]), {"upsamples": [_t(c["up"])]})
            ref = _unary(blocks, c["w"], c["bias"], relu)(torch.cat([up, _t(c["x1"])], dim=1)).numpy()
            want, bound, _ = ur.unary(c["w"], c["x0"], c["up"][:, 0], c["x1"], bias=c["bias"], norm=use_bn,
                                      eps=uc.EPS, slope=uc.SLOPE, act=relu)
            check(f"upcat/{name}", ref, want, bound)
            out[f"upcat/{name}"] = ref
        for name in uc.BLOCKS:
            rec = {}
            ref, c = reference_block(blocks, name, rec)
            st = ur.block_stages(uc.BLOCKS[name][0], c, rec["conv_in"], rec["conv_out"], uc.EPS, uc.SLOPE)
            if st["conv_in"] is not None:
                check(f"block/{name}/conv_in", rec["conv_in"], *st["conv_in"])
                out[f"block/{name}/conv_in"] = rec["conv_in"]
            check(f"block/{name}/conv_out", rec["conv_out"], *st["conv_out"])
            check(f"block/{name}/out", ref, *st["out"])
            out[f"block/{name}/conv_out"], out[f"block/{name}/out"] = rec["conv_out"], ref

        # the tiny network: the reference's forward on the reference's blocks, in f32 and in f64
        cfg = types.SimpleNamespace(final_feats_dim=uc.NET["final"])
        decider = lambda name, cin, cout, layer: blocks.block_decider(name, 1.0, cin, cout, True, 0.02, layer, cfg)  # noqa: E731
        case = uc.make_net()
        net = ub.load_net(ub.TinyNet(decider, unary=blocks.UnaryBlock, pool=blocks.MaxPoolBlock), case["params"])
        h, m, lo = (t.numpy() for t in NgeNet.forward(net, ub.net_inputs(case["inputs"])))
        twin = NgeNet.forward(net.double(), ub.net_inputs(case["inputs"], dtype=torch.float64))
        dev = max(float(np.abs(a - b.numpy()).max()) for a, b in zip((h, m, lo), twin))
    out.update({"net/h": h, "net/m": m, "net/l": lo, "net/deviation": np.float64(dev)})
    print(f"net: h {h.shape}, m {m.shape}, l {lo.shape}; f32 composite vs its f64 twin: max deviation {dev:.3e}, "
          f"wiring tolerance {WIRING_FACTOR} x = {WIRING_FACTOR * dev:.3e}")
    path = os.path.join(HERE, "unary_golden.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < 512 * 1024, size
    print(f"unary: {size} bytes, {len(out)} arrays, worst err / bound {worst:.4f}")


if __name__ == "__main__":
    main()
