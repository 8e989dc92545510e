"""Generate tests/golden/attention_golden.npz by driving the reference's OWN
multi_head_attention (c2p-net/ngenet/models/information_interactive.py:165-177)
and OverlapAttentionBlock.forward (ROPNet/src/models/TFMR.py:76-106), imported
read-only (no bytecode written).  The file holds data only: what the
reference's functions returned.  Inputs are regenerated from
attention_cases.py by the tests, not stored.

`open3d` is not installed: an EMPTY placeholder module satisfies the top-level
imports.

  mha/<case>          multi_head_attention(query, key, value)          (B,dv,h,N) f32
  overlap/src, /tgt   multi_head_attention with one head, value width 1 and the
                      query pre-scaled by sqrt(C) / temperature: the softmax
                      matmul of NgeNet.py:175-178 for either cloud   (n1,), (n2,) f32
  offset/<case>/ol, /none
                      OverlapAttentionBlock.forward(x, ol_score or None) with the
                      case's selection weights in q/k/v_conv, trans_conv the
                      identity, after_norm and act nn.Identity: 2 x - x_r, f32

The script refuses to write unless every reference output lies within the f64
restatement's bound (tests/attention_ref.py); the block's x_r is recovered as
2 x - output, for which one ulp of |2 x| is added.

    python tests/golden/make_golden_attention.py --reference <checkout of the reference>
"""
import argparse
import os
import sys
import types

sys.dont_write_bytecode = True
os.environ["PYTHONDONTWRITEBYTECODE"] = "1"
import numpy as np  # noqa: E402
import torch  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
sys.modules.setdefault("open3d", types.ModuleType("open3d"))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import attention_cases as ac  # noqa: E402
import attention_ref as ar  # noqa: E402


def _import(path, module):
    """Import `module` with `path` first on sys.path."""
    sys.path.insert(0, path)
    try:
        return __import__(module, fromlist=["_"])
    finally:
        sys.path.remove(path)


def _check(name, ref, want, bound, extra=0.0):
    err = np.abs(ref.astype(np.float64) - want)
    ratio = float((err / (bound + extra)).max())
    print(f"{name:24s} {tuple(ref.shape)} max err / bound = {ratio:.4f}")
    return ratio <= 1.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("PCR_REFERENCE"),
                    help="checkout of the reference project (or PCR_REFERENCE)")
    a = ap.parse_args()
    if not a.reference:
        ap.error("--reference (or PCR_REFERENCE) is required")
    out, ok = {}, True
    torch.manual_seed(0)

    ii = _import(os.path.join(a.reference, "c2p-net"), "ngenet.models.information_interactive")
    with torch.no_grad():
        for name in ac.MHA_CASES:
            c = ac.make_mha(name)
            ref = ii.multi_head_attention(*(torch.from_numpy(c[k]) for k in ("query", "key", "value"))).numpy()
            want, bound = ar.multi_head(c["query"], c["key"], c["value"])
            ok &= _check(f"mha/{name}", ref, want, bound)
            out[f"mha/{name}"] = ref
        c = ac.make_overlap()
        f, s, n1, temp = c["feats_norm"], c["attn_scores"], c["len_src"], c["temperature"]
        C = f.shape[1]
        want, bound = ar.overlap_scores(f, s, n1, temp)
        pre = np.float32(np.sqrt(C) / temp)
        for key, qs, ks in (("src", slice(0, n1), slice(n1, None)), ("tgt", slice(n1, None), slice(0, n1))):
            q = torch.from_numpy(f[qs].T.copy()).reshape(1, C, 1, -1) * pre
            k = torch.from_numpy(f[ks].T.copy()).reshape(1, C, 1, -1)
            v = torch.from_numpy(s[ks].T.copy()).reshape(1, 1, 1, -1)
            ref = ii.multi_head_attention(q, k, v).numpy().reshape(-1)
            ok &= _check(f"overlap/{key}", ref, want[qs, 0], bound[qs, 0])
            out[f"overlap/{key}"] = ref

    tf = _import(os.path.join(a.reference, "ROPNet", "src"), "models.TFMR")
    with torch.no_grad():
        for name in ac.OFFSET_CASES:
            c = ac.make_offset(name)
            C = c["x"].shape[1]
            blk = tf.OverlapAttentionBlock(C)
            blk.k_conv.weight.copy_(torch.from_numpy(c["w_qk"])[:, :, None])   # q_conv shares it
            blk.v_conv.weight.copy_(torch.from_numpy(c["w_v"])[:, :, None])
            blk.v_conv.bias.zero_()
            blk.trans_conv.weight.copy_(torch.eye(C)[:, :, None])
            blk.trans_conv.bias.zero_()
            blk.after_norm, blk.act = torch.nn.Identity(), torch.nn.Identity()
            q, v = ac.offset_qkv(c)
            x = torch.from_numpy(c["x"])
            for key, ol in (("ol", c["ol"]), ("none", None)):
                ref = blk(x, None if ol is None else torch.from_numpy(ol)).numpy()
                want, bound = ar.offset_batched(q, q, v, ol)
                x_r = 2.0 * c["x"].astype(np.float64) - ref.astype(np.float64)
                ulp = np.spacing(np.abs(2.0 * c["x"]).astype(np.float32)).astype(np.float64)
                ok &= _check(f"offset/{name}/{key}", x_r, want, bound, ulp)
                out[f"offset/{name}/{key}"] = ref

    if not ok:
        print("nothing written: a reference output lies outside the restatement's bound")
        sys.exit(1)
    path = os.path.join(HERE, "attention_golden.npz")
    np.savez_compressed(path, **out)
    print("attention", os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
