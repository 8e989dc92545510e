"""Generate tests/golden/pointnet_golden.npz by driving the reference's OWN
PointNetFeature (dip/network.py), imported read-only (no bytecode written), with
its trained checkpoint dip/chkpts/final_dip.pt (dim = 32) in eval mode on the
CPU.  The file holds data only: the checkpoint's arrays and what the reference's
modules returned at every stage boundary for the eight patches of
pointnet_cases.golden_patches().

  sd/<key>            the state dict (keys without DataParallel's "module.")
  <patch>/x           the patch (3, P) f32, as pointnet_cases makes it
  <patch>/stn_mx      T-net: max over points of conv2(conv1(x))          (256,)
  <patch>/stn_hid     T-net: fc1 of that                                   (128,)
  <patch>/trans       stn3d(x)                                             (9,)
  <patch>/xtrans      bmm(trans, x)                                        (3, P)
  <patch>/mx, /amx    max and argmax over points of conv2(conv1(xtrans))   (256,) f32, int64
  <patch>/fc1         fc1(mx)                                              (128,)
  <patch>/fc2         fc2 of that                                          (32,)
  <patch>/f           the network's output (l2-normalised)                 (32,)

The script refuses to write unless every stage lies within the f64 restatement's
bound from the reference's own previous stage (tests/pointnet_ref.py), as
tests/test_pointnet_cpu.py checks again from the file.

    python tests/golden/make_golden_pointnet.py --reference <checkout of the reference>
"""
import argparse
import os
import sys

sys.dont_write_bytecode = True
os.environ["PYTHONDONTWRITEBYTECODE"] = "1"
import numpy as np  # noqa: E402
import torch  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import pointnet_cases as pc  # noqa: E402
import pointnet_ref as pr  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("PCR_REFERENCE"),
                    help="checkout of the reference project (or PCR_REFERENCE)")
    a = ap.parse_args()
    if not a.reference:
        ap.error("--reference (or PCR_REFERENCE) is required")
    dip_dir = os.path.join(a.reference, "dip")
    sys.path.insert(0, dip_dir)
    try:
        network = __import__("network")
    finally:
        sys.path.remove(dip_dir)
    sd = torch.load(os.path.join(dip_dir, "chkpts", "final_dip.pt"), map_location="cpu")
    sd = {k[len("module."):] if k.startswith("module.") else k: v for k, v in sd.items()}
    net = network.PointNetFeature(dim=32, l2norm=True, tnet=True)
    net.load_state_dict(sd)
    net.eval()

    out = {f"sd/{k}": v.numpy() for k, v in sd.items()}
    with torch.no_grad():
        for name, x in pc.golden_patches().items():
            xt = torch.from_numpy(x)[None]
            stn = net.stn3d
            stn_mx = torch.max(stn.conv2(stn.conv1(xt)), 2)[0]
            stn_hid = stn.fc1(stn_mx)
            f, xtrans, trans, mx, amx = net._forward(xt)
            h = net.fc1(mx.view(-1, 256))
            g = {"x": x, "stn_mx": stn_mx[0], "stn_hid": stn_hid[0], "trans": trans.reshape(9), "xtrans": xtrans[0],
                 "mx": mx.reshape(256), "amx": amx.reshape(256), "fc1": h[0], "fc2": net.fc2(h)[0], "f": f[0]}
            for k, v in g.items():
                out[f"{name}/{k}"] = np.ascontiguousarray(v.numpy() if isinstance(v, torch.Tensor) else v)

    folded = pr.folded_layers(pr.net_from_arrays({k[3:]: v for k, v in out.items() if k.startswith("sd/")}))
    ok = True
    for name in pc.GOLDEN_PATCHES:
        for stage, ratio in pr.stage_ratios(folded, {k.split("/", 1)[1]: v for k, v in out.items()
                                                     if k.startswith(name + "/")}).items():
            print(f"{name:8s} {stage:12s} max err / bound = {ratio:.4f}")
            ok &= ratio <= 1.0
    if not ok:
        print("nothing written: a reference output lies outside the restatement's bound")
        sys.exit(1)
    path = os.path.join(HERE, "pointnet_golden.npz")
    np.savez_compressed(path, **out)
    print("pointnet", os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
