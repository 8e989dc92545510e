"""Generate tests/golden/groupmlp_golden.npz by IMPORTING the reference's own
Python code (read-only, no bytecode written) in the build container.  The file
holds only what the reference returned; inputs and weights are regenerated from
seeds by groupmlp_cases.py.

  GCN, PPF, GGE, LocalFeatureFused   c2p-net/ngenet/models/information_interactive.py
  LocalFeatue, LocalFeatureFused     ROPNet/src/models/TFMR.py

`open3d` is not installed: an EMPTY placeholder module satisfies the top-level
`import open3d` (nothing used here calls into it).

GCN cases run the reference's whole GCN.forward; feats1 and feats2 are taken
from inside the call by forward hooks on conv1 and conv2 (the max over k is
the reference's own next line, redone here).  The k-NN sets of the float
clouds equal the library order's: asserted below, change the seed if not.
MLP cases build the reference's PPF / LocalFeatue, load the case weights into
`local_feature_fused` and run that module on the case's group.  GGE is built
once to check that it is made of these very classes.

Nothing is written unless every reference output lies within the carried bound
of the f64 restatement (tests/groupmlp_ref.py).

Keys:  gcn/<case>/feats1 (B, C, N), feats2 (B, 2C, N), out (B, C, N);
       mlp/<case>/out (B, c_L, N).

    python tests/golden/make_golden_groupmlp.py
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
import groupmlp_cases as cases  # noqa: E402
import groupmlp_ref as ref  # noqa: E402
import knn_graph_ref as kr  # noqa: E402


def _imp_ngenet():
    sys.path.insert(0, f"{REF}/c2p-net")
    from ngenet.models import information_interactive as ii
    return ii


def _imp_ropnet():
    """ROPNet's TFMR imports `utils` and `models` as top-level names that c2p-net's tree would
    shadow: it is loaded with ROPNet/src first on the path and those names dropped afterwards."""
    saved = list(sys.path)
    stale = {k: sys.modules.pop(k) for k in list(sys.modules) if k.split(".")[0] in ("utils", "models")}
    sys.path.insert(0, f"{REF}/ROPNet/src")
    try:
        from models import TFMR
    finally:
        sys.path[:] = saved
        for k in list(sys.modules):
            if k.split(".")[0] in ("utils", "models"):
                sys.modules.pop(k)
        sys.modules.update(stale)
    return TFMR


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def load_mlp(fused, case):
    blocks = list(fused.blocks.children())
    with torch.no_grad():
        for i, w in enumerate(case["weights"]):
            conv, norm = blocks[3 * i], blocks[3 * i + 1]
            assert conv.weight.shape[:2] == w.shape and conv.bias is None
            conv.weight.copy_(t(w)[:, :, None, None])
            if case["gammas"][i] is not None:
                norm.weight.copy_(t(case["gammas"][i]))
                norm.bias.copy_(t(case["betas"][i]))


def check(name, got, want, bound):
    ratio = ref.ratio(got, want, bound)
    print(f"{name}: reference within {ratio:.3g} of the restatement's bound")
    assert ratio <= 1.0, f"{name}: the reference leaves the bound; nothing written"


def main():
    ii = _imp_ngenet()
    out = {}
    gge = ii.GGE(feats_dim=32, gcn_k=10, ppf_k=16, radius=0.6, bottleneck=True)
    assert any(isinstance(m, ii.GCN) for m in gge.modules()) and any(isinstance(m, ii.PPF) for m in gge.modules())

    for name in cases.GCN_CASES:
        c = cases.gcn_case(name)
        b, ch, n = c["feats"].shape
        gcn = ii.GCN(ch, c["k"]).eval()
        with torch.no_grad():
            gcn.conv1[0].weight.copy_(t(c["conv1"])[:, :, None, None])
            gcn.conv2[0].weight.copy_(t(c["conv2"])[:, :, None, None])
            gcn.conv3[0].weight.copy_(t(c["conv3"])[:, :, None])
        taps, picks = {}, []
        hooks = [gcn.conv1.register_forward_hook(lambda m, i, o: taps.__setitem__("feats1", o.max(-1)[0])),
                 gcn.conv2.register_forward_hook(lambda m, i, o: taps.__setitem__("feats2", o.max(-1)[0]))]
        topk = torch.topk

        def tap(*a, **kw):
            res = topk(*a, **kw)
            picks.append(res[1].numpy())
            return res
        torch.topk = tap
        try:
            with torch.no_grad():
                res = gcn(t(c["coords"]), t(c["feats"])).numpy()
        finally:
            torch.topk = topk
            for h in hooks:
                h.remove()
        xyz = np.ascontiguousarray(c["coords"].transpose(0, 2, 1))
        idx, _ = kr.knn_graph(xyz, c["k"])
        for p in picks:   # float clouds: the reference's neighbour sets are the library order's
            assert (np.sort(p[..., 1:], -1) == np.sort(idx, -1)).all(), (name, "k-NN sets differ: change the seed")
        f1 = taps["feats1"].numpy()
        f2 = taps["feats2"].numpy()
        for i in range(b):
            w1, e1 = ref.edge_conv(c["conv1"], c["feats"][i].T, idx[i], cases.EPS, cases.GCN_SLOPE)
            check(f"gcn/{name}/feats1[{i}]", f1[i].T, w1, e1)
            w2, e2 = ref.edge_conv(c["conv2"], f1[i].T, idx[i], cases.EPS, cases.GCN_SLOPE)
            check(f"gcn/{name}/feats2[{i}]", f2[i].T, w2, e2)
        out[f"gcn/{name}/feats1"], out[f"gcn/{name}/feats2"], out[f"gcn/{name}/out"] = f1, f2, res

    tfmr = _imp_ropnet()
    for name, (kind, b, n, k, radius, widths) in cases.MLP_CASES.items():
        c = cases.mlp_case(name)
        cin = c["x"].shape[-1]
        if kind == "ppf":
            mod = ii.PPF(list(widths), k, radius)
        else:
            mod = tfmr.LocalFeatue(radius, k, cin, list(widths))
        fused = mod.local_feature_fused.eval()
        load_mlp(fused, c)
        with torch.no_grad():
            res = fused(t(c["x"].transpose(0, 3, 2, 1))).numpy()   # (B, C, K, N) -> (B, c_L, N)
        for i in range(b):
            want, bound, _ = ref.group_mlp(c["x"][i], c["weights"], c["gammas"], c["betas"], cases.EPS, 0.0,
                                           1 if c["norm"] == "instance" else 32)
            check(f"mlp/{name}[{i}]", res[i].T, want, bound)
        out[f"mlp/{name}/out"] = res

    path = os.path.join(HERE, "groupmlp_golden.npz")
    np.savez_compressed(path, **out)
    print("groupmlp", os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
