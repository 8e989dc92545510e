"""Generate tests/golden/grouping_golden.npz by IMPORTING the reference's own
Python code (read-only, no bytecode written) in the build container.  The file
holds data only: the input clouds and what the reference returned for them.

  fps / ball_query / sample_and_group   ROPNet/src/models/model_utils.py:6-102
  LocalFeatue.forward (use_ppf)         ROPNet/src/models/TFMR.py:48-71
  ball_query with K > N                 c2p-net/ngenet/utils/process.py:57-79
                                        (ROPNet's raises there)

`open3d` is not installed: an EMPTY placeholder module satisfies the top-level
`import open3d` (nothing used here calls into it).

Clouds.  Lattice clouds have coordinates that are multiples of 1/16 in [-1, 1]
(duplicates allowed): with radii 0.25 and 0.5 both r^2 are exact, many pairs
sit exactly on them, and the FPS maximum has many exact ties.  Float clouds
are uniform in [-1, 1]^3.  On all of them the reference's expanded-form
distances select the same points as the direct form of the contract
(tests/test_grouping_cpu.py checks that on every array stored here; if a
regenerated fixture breaks it, change SEED, not the test).

FPS lengths are m in {1, 3, n, n + 3} on every cloud but f2048.  There the
reference's expanded form |a|^2 + |b|^2 - 2 a.b carries an absolute error of
about 1e-7 into distances that have shrunk to 1e-2 after some hundred picks,
and its argmax leaves the direct form's at a near tie: over twelve seeds the
first such pick fell between 404 and 1769, so no seed pins m = 2048.  f2048 is
therefore pinned to m in {1, 3, 512} (512 is the ROPNet-sized sample the
benchmark tool times; F2048_SEED is one whose first near tie comes later), and
the GPU tests run its m = n and m = n + 3 against the restatement instead.

Keys (indices are stored as int16; every one is < 2^15):
  cloud/<c>                      (b,n,3) f32
  fps/<c>/m<m>                   (b,m)   the reference's fps under torch seed
                                 FPS_SEED; its column 0 is the start it drew
  bq/<c>/r<r>/k<k>/idx, /count   ball_query(xyz, xyz, r, k, rt_density=True);
                                 count = density * n, the reference's integer sum
  sg/<c>/...                     sample_and_group with M > 0: new_xyz, idx, count
  ppf/<p>/...                    LocalFeatue's feature_local (B,C,K,N), the normals,
                                 and spread_angle / spread_norm: max |reference f32
                                 - f64 evaluation of the same formulas on the f32
                                 normals and the f32 g| over channels 6-8 / 9

    python tests/golden/make_golden_grouping.py
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
import grouping_ref  # noqa: E402

SEED = 20240611
F2048_SEED = (SEED, 2048, 0)
FPS_SEED = 77
F2048_FPS_M = (1, 3, 512)

# name -> (kind, b, n)
CLOUDS = {
    "l1": ("lattice", 1, 1), "l5": ("lattice", 3, 5), "l63": ("lattice", 1, 63),
    "l64": ("lattice", 3, 64), "l65": ("lattice", 1, 65), "l257": ("lattice", 3, 257),
    "l1025": ("lattice", 1, 1025),
    "f257": ("float", 2, 257), "f2048": ("float", 2, 2048),
}
KS = (1, 16, 64)


def radii(kind):
    return (0.25, 0.5) if kind == "lattice" else (0.3,)


def make_clouds():
    rng = np.random.default_rng(SEED)
    out = {}
    for name, (kind, b, n) in CLOUDS.items():
        if kind == "lattice":
            out[name] = (rng.integers(-16, 17, (b, n, 3)) / 16.0).astype(np.float32)
        elif name == "f2048":
            out[name] = np.random.default_rng(F2048_SEED).uniform(-1, 1, (b, n, 3)).astype(np.float32)
        else:
            out[name] = rng.uniform(-1, 1, (b, n, 3)).astype(np.float32)
    return out


def _imp_ropnet():
    sys.path.insert(0, f"{REF}/ROPNet/src")
    from models import model_utils
    from models.TFMR import LocalFeatue
    return model_utils, LocalFeatue


def _imp_ngenet_ball_query():
    import importlib.util
    spec = importlib.util.spec_from_file_location("_ngenet_process", f"{REF}/c2p-net/ngenet/utils/process.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.ball_query


def i16(t):
    a = t.numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    assert a.min() >= 0 and a.max() < 2 ** 15
    return a.astype(np.int16)


def main():
    mu, LocalFeatue = _imp_ropnet()
    ngenet_ball_query = _imp_ngenet_ball_query()
    clouds = make_clouds()
    out = {}
    for name, x in clouds.items():
        kind, b, n = CLOUDS[name]
        out[f"cloud/{name}"] = x
        xt = torch.from_numpy(x)
        for m in (F2048_FPS_M if name == "f2048" else sorted({1, 3, n, n + 3})):
            torch.manual_seed(FPS_SEED)
            out[f"fps/{name}/m{m}"] = i16(mu.fps(xt, m))
        for r in radii(kind):
            for k in KS:
                fn = mu.ball_query if k <= n else ngenet_ball_query
                idx, density = fn(xt, xt, r, k, rt_density=True)
                out[f"bq/{name}/r{r}/k{k}/idx"] = i16(idx)
                out[f"bq/{name}/r{r}/k{k}/count"] = i16(torch.round(density * n))
    # sample_and_group with M > 0 (fps inside, under the same seed rule)
    for name, M, r, k in (("l257", 32, 0.5, 16), ("f257", 64, 0.3, 16), ("f2048", 128, 0.3, 64)):
        xt = torch.from_numpy(clouds[name])
        torch.manual_seed(FPS_SEED)
        new_xyz, _, idx, _, density = mu.sample_and_group(xt, None, M, r, k, rt_density=True)
        out[f"sg/{name}/M"], out[f"sg/{name}/r"], out[f"sg/{name}/k"] = np.array(M), np.array(r), np.array(k)
        out[f"sg/{name}/new_xyz"] = new_xyz.numpy()
        out[f"sg/{name}/idx"] = i16(idx)
        out[f"sg/{name}/count"] = i16(torch.round(density * xt.shape[1]))
    # the fused group: LocalFeatue with its conv stack replaced by the identity
    rng = np.random.default_rng(SEED + 1)
    for pname, (name, r, k) in {"l65": ("l65", 0.5, 16), "l257": ("l257", 0.25, 16),
                                "f257": ("f257", 0.3, 16)}.items():
        x = clouds[name]
        nrm = rng.standard_normal(x.shape)
        nrm = (nrm / np.linalg.norm(nrm, axis=-1, keepdims=True)).astype(np.float32)
        nrm[:, ::17] = 0.0                         # angle(0, .) = 0
        nrm[:, 1::17] = -np.abs(nrm[:, 1::17])     # all-negative normals: the dot with g = 0 is -0 thrice
        lf = LocalFeatue(r, k, in_dim=10, out_dims=[32])
        lf.local_feature_fused = torch.nn.Identity()
        with torch.no_grad():
            f10 = lf(torch.from_numpy(nrm), torch.from_numpy(x), use_ppf=True).numpy()
            f6 = lf(None, torch.from_numpy(x)).numpy()
        assert f10.shape == (x.shape[0], 10, k, x.shape[1]) and f6.shape[1] == 6
        idx, _ = grouping_ref.ball_query(x, x, r, k)
        e64 = grouping_ref.group_ppf(x, nrm, idx, np.float64)
        ref = np.transpose(f10, (0, 3, 2, 1)).astype(np.float64)
        out[f"ppf/{pname}/cloud"], out[f"ppf/{pname}/r"], out[f"ppf/{pname}/k"] = np.array(name), np.array(r), np.array(k)
        out[f"ppf/{pname}/normals"] = nrm
        out[f"ppf/{pname}/feat10"], out[f"ppf/{pname}/feat6"] = f10, f6
        out[f"ppf/{pname}/spread_angle"] = np.abs(ref[..., 6:9] - e64[..., 6:9]).max()
        out[f"ppf/{pname}/spread_norm"] = np.abs(ref[..., 9] - e64[..., 9]).max()
        print(pname, "spread", out[f"ppf/{pname}/spread_angle"], out[f"ppf/{pname}/spread_norm"])
    path = os.path.join(HERE, "grouping_golden.npz")
    np.savez_compressed(path, **out)
    print("grouping", os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
