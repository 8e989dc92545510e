"""Generate tests/golden/procrustes_edges_golden.npz by IMPORTING the reference's
own Python code (read-only, no bytecode written) in the build container, in the
manner of make_golden_py.py.  Outputs are data (inputs + the reference's
outputs); the reference itself never travels.

  weighted_icp     ROPNet/src/models/model_utils.py:105-139
  rigid_fit        c2p-net/deformationpyramid/model/geometry.py:8-34

For every named case of tests/procrustes_ref.py with a unique optimum
(cases(np.float32): the tails, the angles, the conditioning cases; B = 3):
  <case>/src, tgt, w            the f32 inputs
  <case>/wicp64/R, t            weighted_icp on those inputs cast to f64
  <case>/wicp32/R, t            weighted_icp on the f32 inputs
  <case>/rfit32/R, t            rigid_fit on the f32 inputs
The cases without a unique optimum are not stored: the reference's answer
there is one of many (and its own determinant assertion may fire).

`open3d` is not installed: an EMPTY placeholder module satisfies the top-level
`import open3d` of geometry.py (neither function calls into it).

    python tests/golden/make_golden_procrustes_edges.py
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
sys.path.insert(0, os.path.dirname(HERE))
import procrustes_ref as pref  # noqa: E402


def _imp():
    sys.path.insert(0, f"{REF}/ROPNet/src")
    from models.model_utils import weighted_icp
    sys.path.insert(0, f"{REF}/c2p-net/deformationpyramid")
    from model.geometry import rigid_fit
    return weighted_icp, rigid_fit


def main():
    weighted_icp, rigid_fit = _imp()
    out = {}
    for name, (s, t, w, unique) in pref.cases(np.float32).items():
        if not unique:
            continue
        ts, tt, tw = torch.from_numpy(s), torch.from_numpy(t), torch.from_numpy(w)
        out[f"{name}/src"], out[f"{name}/tgt"], out[f"{name}/w"] = s, t, w
        R, tr, _ = weighted_icp(ts.double(), tt.double(), tw.double())
        out[f"{name}/wicp64/R"], out[f"{name}/wicp64/t"] = R.numpy(), tr.numpy()
        R32, t32, _ = weighted_icp(ts, tt, tw)
        out[f"{name}/wicp32/R"], out[f"{name}/wicp32/t"] = R32.numpy(), t32.numpy()
        R2, t2 = rigid_fit(ts, tt, tw[..., None])
        out[f"{name}/rfit32/R"], out[f"{name}/rfit32/t"] = R2.numpy(), t2.numpy()
        assert R.dtype == torch.float64 and R32.dtype == torch.float32 and R2.dtype == torch.float32
        # the reference's own f32 error against its f64 run, for the record
        dR = np.linalg.norm((R32.double() - R).numpy(), axis=(1, 2)).max()
        dt = np.linalg.norm((t32.double() - tr).numpy(), axis=1).max()
        print(f"{name:18s} N={s.shape[1]:4d}  wicp32 vs wicp64: dR {dR:.2e} dt {dt:.2e}")
    path = os.path.join(HERE, "procrustes_edges_golden.npz")
    np.savez_compressed(path, **out)
    print("procrustes_edges", os.path.getsize(path))


if __name__ == "__main__":
    main()
