"""Generate tests/golden/tfmr_golden.npz by driving the reference's OWN
TFMRModule.forward (ROPNet/src/models/TFMR.py:154-257, train=False, iter=0),
imported read-only (no bytecode written) in the build container.  The file
holds data only: what the reference returned.

`open3d` is not installed: an EMPTY placeholder module satisfies the top-level
`import open3d`.  The module's two networks (local_features, overlap_attention)
are replaced by small nn.Module stubs that return prescribed tensors -- the
raw features of tests/tfmr_ref.py's generator -- so that forward runs its own
normalise / sort / gather lines and its whole matching on them.

Inputs are regenerated from tfmr_ref.GOLDEN_SEED by the tests, not stored.
Per case (tfmr_ref.GOLDEN_CASES):
  <case>/similarity_max_inds   (B,N2) int16
  <case>/tgt_corr              (B,N2,3) f32
  <case>/icp_weights           (B,N2) f32
  <case>/spread                max |reference tgt_corr - restatement|

The fma-chain restatement has to equal the reference outright on every index
and on icp_weights: rows whose maxima differ by under an ulp can swap places
under the reference's bmm, so if a regenerated fixture breaks
tests/test_tfmr_cpu.py, change GOLDEN_SEED, not the test.  This script checks
the same and refuses to write otherwise.

    python tests/golden/make_golden_tfmr.py
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
REF = "/root/reference"
sys.modules.setdefault("open3d", types.ModuleType("open3d"))
sys.path.insert(0, os.path.dirname(HERE))
import tfmr_ref  # noqa: E402


class _Pass(torch.nn.Module):
    """local_features stand-in: hands the cloud on as the 'features'."""

    def forward(self, feature, xyz, permute=False, use_ppf=False):
        return xyz


class _Prescribed(torch.nn.Module):
    """overlap_attention stand-in: the prescribed (B,C,N) tensor of the cloud
    it is called for (the source first, then the target)."""

    def __init__(self, tensors):
        super().__init__()
        self.tensors = list(tensors)

    def forward(self, x, ol):
        return self.tensors.pop(0)


def run_reference(TFMRModule, case, k, top_prob):
    B, N1, _ = case["src"].shape
    M1 = case["tgt"].shape[1]
    args = types.SimpleNamespace(train_N1=N1, test_N1=N1, train_M1=M1, test_M1=M1, train_top_prob=top_prob,
                                 test_top_prob=top_prob, train_similarity_topk=k, test_similarity_topk=k,
                                 use_ppf=False, radius=0.3, num_neighbors=8, feat_dim=32)
    mod = TFMRModule(args)
    mod.local_features = _Pass()
    t = {n: torch.from_numpy(v) for n, v in case.items()}
    mod.overlap_attention = _Prescribed([t["f_x_attn"].permute(0, 2, 1), t["f_y_attn"].permute(0, 2, 1)])
    with torch.no_grad():
        src, tgt_corr, icp_w, inds = mod(t["src"], t["tgt"], t["x_ol_score"], t["y_ol_score"], train=False,
                                         iter=0)
    return src.numpy(), tgt_corr.numpy(), icp_w.numpy(), inds.numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=None, help="probe another seed (nothing is written)")
    a = ap.parse_args()
    if a.seed is not None:
        tfmr_ref.GOLDEN_SEED = a.seed
    sys.path.insert(0, f"{REF}/ROPNet/src")
    from models.TFMR import TFMRModule
    out, ok = {}, True
    for name, (B, N1, M1, C, k, p) in tfmr_ref.GOLDEN_CASES.items():
        case = tfmr_ref.golden_case(name)
        src, tgt_corr, icp_w, inds = run_reference(TFMRModule, case, k, p)
        (fx, fy, src_g, tgt_g, x_ol), S = tfmr_ref.golden_similarity((B, N1, M1, C))
        n_keep = int(p * N1)
        r = tfmr_ref.restate(fx, fy, tgt_g, k, n_keep, S=S)
        bi = np.arange(B)[:, None]
        same = (np.array_equal(inds, r["sel"]) and icp_w.tobytes() == x_ol[bi, r["sel"]].tobytes()
                and src.tobytes() == src_g[bi, r["sel"]].tobytes())
        spread = float(np.abs(tgt_corr.astype(np.float64) - r["tgt_corr"]).max())
        print(name, "equal" if same else f"DIFFERS in {(inds != r['sel']).sum()} places", "spread", spread)
        ok &= same and spread < 1e-6
        assert inds.min() >= 0 and inds.max() < 2 ** 15
        out[f"{name}/similarity_max_inds"] = inds.astype(np.int16)
        out[f"{name}/tgt_corr"] = tgt_corr
        out[f"{name}/icp_weights"] = icp_w
        out[f"{name}/spread"] = np.array(spread)
    if a.seed is not None or not ok:
        print("nothing written" + ("" if ok else ": the restatement differs, choose another GOLDEN_SEED"))
        sys.exit(0 if ok else 1)
    path = os.path.join(HERE, "tfmr_golden.npz")
    np.savez_compressed(path, **out)
    print("tfmr", os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
