"""Generate tests/golden/knn_golden.npz by IMPORTING the reference's own Python
code (read-only, no bytecode written) in the build container.  The file holds
data only: the input clouds and features and what the reference returned.

  get_graph_features   c2p-net/ngenet/models/information_interactive.py:7-23

`open3d` is not installed: an EMPTY placeholder module satisfies the top-level
`import open3d` (nothing used here calls into it).

The reference's function returns the gathered features only.  Its neighbour
indices, column 0 included, are taken from inside the call: `torch.topk` is
wrapped for the duration of the call and the wrapper records what the
reference's own topk returned.

Clouds.  Lattice clouds have coordinates that are multiples of 1/16 in [-1, 1]
(duplicates allowed): the reference's expanded-form distances are exact there,
many rows are tied at the cut, and topk breaks the ties arbitrarily, so the
pinned quantity is the ranked direct-form distances of its k + 1 picks.  Float
clouds are uniform in [-1, 1]^3: no exact ties, and the pinned quantities are
every row's neighbour set and the dropped column (tests/test_knn_graph_cpu.py
checks both on every array stored here; main() asserts them too, so a seed
that breaks them never reaches the file: change the seed, not the test).  At
2048 points some seeds have one row whose expanded-form near tie at the cut
picks the other point; F2048_SEED has none for k in FLOAT_KS.

Keys (indices are stored as int16; every one is < 2^15):
  cloud/<c>              (b,n,3) f32
  topk/<c>/k<k>          (b,n,min(n,k+1)) the reference's topk indices, column 0
                         (the one get_graph_features drops) included
  feat/cloud, feat/feats, feat/k, feat/out
                         one full get_graph_features call: (2,65,3), (2,65,8),
                         10 and the reference's (2,65,10,16) output
  shape/n<n>/k10         the shape get_graph_features returned for (2,n,3)
                         coordinates and (2,n,8) features, n in {1, 5}

    python tests/golden/make_golden_knn.py
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
import knn_graph_ref as kr  # noqa: E402
from grouping_ref import sqdist  # noqa: E402

SEED = 20240611
F2048_SEED = (SEED, 2048, 0)
FEAT_SEED = (SEED, 65, 8)
LATTICE_KS = (1, 10, 32)
FLOAT_KS = (1, 10, 20, 32)

# name -> (kind, b, n)
CLOUDS = {
    "l5": ("lattice", 3, 5), "l64": ("lattice", 3, 64), "l65": ("lattice", 1, 65),
    "l257": ("lattice", 3, 257), "l1025": ("lattice", 1, 1025),
    "f257": ("float", 2, 257), "f1025": ("float", 2, 1025), "f2048": ("float", 2, 2048),
}


def make_clouds():
    rng = np.random.default_rng(SEED)
    out = {}
    for name, (kind, b, n) in CLOUDS.items():
        if kind == "lattice":
            out[name] = (rng.integers(-16, 17, (b, n, 3)) / 16.0).astype(np.float32)
        else:
            seed = F2048_SEED if n == 2048 else (SEED, n, 1)
            out[name] = np.random.default_rng(seed).uniform(-1, 1, (b, n, 3)).astype(np.float32)
    return out


def _imp_reference():
    sys.path.insert(0, f"{REF}/c2p-net")
    from ngenet.models.information_interactive import get_graph_features
    return get_graph_features


class TopkTap:
    """Records the indices every torch.topk call returns while it is active."""

    def __enter__(self):
        self.inds = []
        self._orig = torch.topk

        def tap(*args, **kwargs):
            res = self._orig(*args, **kwargs)
            self.inds.append(res[1])
            return res
        torch.topk = tap
        return self

    def __exit__(self, *exc):
        torch.topk = self._orig


def i16(t):
    a = t.numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    assert a.min() >= 0 and a.max() < 2 ** 15
    return a.astype(np.int16)


def reference_topk(ggf, x, k):
    """The indices of the reference's own topk (b,n,min(n,k+1)) for cloud x."""
    xt = torch.from_numpy(x)
    with TopkTap() as tap, torch.no_grad():
        out = ggf(torch.zeros(x.shape[0], x.shape[1], 1), xt, k)
    assert len(tap.inds) == 1
    picks = tap.inds[0]
    assert out.shape[2] == picks.shape[2] - 1
    return picks.numpy()


def main():
    ggf = _imp_reference()
    clouds = make_clouds()
    out = {}
    for name, x in clouds.items():
        kind, b, n = CLOUDS[name]
        out[f"cloud/{name}"] = x
        rows = np.arange(n)[None, :, None]
        for k in (LATTICE_KS if kind == "lattice" else FLOAT_KS):
            picks = reference_topk(ggf, x, k)
            idx, d2 = kr.ranked(x, k)
            assert picks.shape == idx.shape, (name, k)
            if kind == "lattice":
                dd = np.sort(sqdist(x[:, :, None, :], x[np.arange(b)[:, None, None], picks]), axis=-1)
                assert dd.tobytes() == d2.tobytes(), (name, k)
                same = (picks == idx).all(-1).mean()
            else:
                assert (picks[..., :1] == rows).all(), (name, k, "dropped column")
                assert (np.sort(picks[..., 1:], -1) == np.sort(idx[..., 1:], -1)).all(), (name, k, "sets")
                same = (picks == idx).all(-1).mean()
            print(f"{name} k={k}: rows equal index for index {100 * same:.1f} %")
            out[f"topk/{name}/k{k}"] = i16(picks)
    # one full call, and the shapes at n = 1 and n = 5
    rng = np.random.default_rng(FEAT_SEED)
    x = rng.uniform(-1, 1, (2, 65, 3)).astype(np.float32)
    f = rng.standard_normal((2, 65, 8)).astype(np.float32)
    with TopkTap() as tap, torch.no_grad():
        ref = ggf(torch.from_numpy(f), torch.from_numpy(x), 10).numpy()
    idx, _ = kr.knn_graph(x, 10)
    # ordered equality is needed to compare bytes: FEAT_SEED is one where it holds
    assert (tap.inds[0].numpy()[..., 1:] == idx).all(), "feat: change FEAT_SEED"
    assert ref.tobytes() == kr.edge_features(f, idx).tobytes()
    out["feat/cloud"], out["feat/feats"], out["feat/k"], out["feat/out"] = x, f, np.array(10), ref
    for n in (1, 5):
        with torch.no_grad():
            r = ggf(torch.zeros(2, n, 8), torch.from_numpy(rng.uniform(-1, 1, (2, n, 3)).astype(np.float32)), 10)
        out[f"shape/n{n}/k10"] = np.array(r.shape)
        print("shape", n, tuple(r.shape))
    path = os.path.join(HERE, "knn_golden.npz")
    np.savez_compressed(path, **out)
    print("knn", os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
