"""Generate tests/golden/kpconv_conv_golden.npz by IMPORTING the reference's own
Python code (read-only, no bytecode written) in the build container.  The file
holds only what the reference returned; the inputs come from
kpconv_conv_cases.py.

  KPConv.forward        c2p-net/ngenet/models/KPConv/blocks.py:73-128
  MaxPoolBlock.forward  c2p-net/ngenet/models/KPConv/blocks.py:182-188

`open3d` is not installed: an EMPTY placeholder module satisfies the top-level
`import open3d` (nothing used here calls into it).  KPConv is not instantiated
(its constructor's load_kernels creates a directory inside the reference tree):
`KPConv.forward` is called unbound on a types.SimpleNamespace that carries
kernel_points, weights, KP_extent, KP_influence, aggregation_mode and K.

Keys:
  linear/<case>     (n,C_out) f32  KPConv.forward, KP_influence 'linear', 'sum'
  constant/<case>   (n,C_out) f32  the same with 'constant' (CONSTANT_CASE)
  pool/<case>       (n,C_in) f32   MaxPoolBlock.forward(feats, {'pools': [idx]})

    python tests/golden/make_golden_kpconv_conv.py
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
import kpconv_conv_cases as kc  # noqa: E402
import kpconv_conv_ref as kr  # noqa: E402


def _imp_reference():
    sys.path.insert(0, f"{REF}/c2p-net")
    from ngenet.models.KPConv.blocks import KPConv, MaxPoolBlock
    return KPConv, MaxPoolBlock


def reference_conv(KPConv, c, influence):
    ns = types.SimpleNamespace(kernel_points=torch.from_numpy(c["kp"]), weights=torch.from_numpy(c["W"]),
                               KP_extent=c["extent"], KP_influence=influence, aggregation_mode="sum",
                               K=c["kp"].shape[0])
    with torch.no_grad():
        out = KPConv.forward(ns, torch.from_numpy(c["q"]), torch.from_numpy(c["s"]), torch.from_numpy(c["f"]),
                             torch.from_numpy(c["idx"]))
    return out.numpy().astype(np.float32)


def main():
    KPConv, MaxPoolBlock = _imp_reference()
    out = {}
    worst = 0.0
    for name in kc.CASES:
        c = kc.make(name)
        for infl in ("linear",) + (("constant",) if name == kc.CONSTANT_CASE else ()):
            ref = reference_conv(KPConv, c, infl)
            want, bound, allpad = kr.kpconv(c["q"], c["s"], c["f"], c["idx"], c["kp"], c["W"], c["extent"], infl)
            err = np.abs(ref - want)
            assert (err <= bound).all(), (name, infl)
            assert allpad.any() and not ref[allpad].any(), (name, infl)
            ratio = float((err[bound > 0] / bound[bound > 0]).max())
            worst = max(worst, ratio)
            print(f"{infl}/{name}: shape {ref.shape}, max err / bound = {ratio:.4f}, "
                  f"pads {100 * (c['idx'] == c['s'].shape[0]).mean():.0f} %")
            out[f"{infl}/{name}"] = ref
        if name in kc.POOL_CASES:
            with torch.no_grad():
                pool = MaxPoolBlock.forward(types.SimpleNamespace(layer_ind=0), torch.from_numpy(c["f"]),
                                            {"pools": [torch.from_numpy(c["idx"])]}).numpy()
            assert pool.tobytes() == kr.neighbor_max(c["f"], c["idx"]).tobytes(), name
            out[f"pool/{name}"] = pool
    path = os.path.join(HERE, "kpconv_conv_golden.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < 512 * 1024, size
    print(f"kpconv_conv: {size} bytes, {len(out)} arrays, worst err / bound {worst:.4f}")


if __name__ == "__main__":
    main()
