"""CPU: the numpy restatement of the k-NN graph contract (tests/knn_graph_ref.py:
direct-form distances, the cloud ranked by (d2, index), rank 0 dropped) meets
every quantity that tests/golden/knn_golden.npz pins to the reference's
get_graph_features.  That is what lets the GPU tests stand on the restatement.

Pinned quantities.  Lattice clouds (exact distances, topk's tie order is
arbitrary): the direct-form distances of the reference's k + 1 picks, column 0
included, ranked, equal the contract's ranks 0 .. kk bit for bit on every row.
Float clouds: the neighbour set of every row equals the contract's and the
dropped column is the row's own index.  No row is excluded: if a regenerated
fixture breaks this, change the generator's seed, not the test.  The recorded
get_graph_features output equals the restated features byte for byte.

Also: the two entry points are declared in the header, exported and bound, and
their argument errors and empty calls need no GPU."""
import os
import re

import numpy as np
import pytest

import knn_graph_ref as kr
from grouping_ref import sqdist
from pointcloudregistration_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, "tests", "golden", "knn_golden.npz"))
CLOUDS = sorted(k.split("/")[1] for k in G.files if k.startswith("cloud/"))
TOPK = sorted(k for k in G.files if k.startswith("topk/"))
LATTICE = [k for k in TOPK if k.split("/")[1].startswith("l")]
FLOAT = [k for k in TOPK if k.split("/")[1].startswith("f")]


def _picks(key):
    _, c, k = key.split("/")
    return G[f"cloud/{c}"], int(k[1:]), G[key].astype(np.int64)


def test_fixture_covers_the_cases():
    shapes = {c: G[f"cloud/{c}"].shape[:2] for c in CLOUDS}
    assert {shapes[c] for c in CLOUDS if c.startswith("l")} == {(3, 5), (3, 64), (1, 65), (3, 257), (1, 1025)}
    assert {shapes[c] for c in CLOUDS if c.startswith("f")} == {(2, 257), (2, 1025), (2, 2048)}
    for c in CLOUDS:
        ks = (1, 10, 32) if c.startswith("l") else (1, 10, 20, 32)
        assert all(f"topk/{c}/k{k}" in G.files for k in ks)
    tied_at_cut = coincident = False
    for c in CLOUDS:
        x = G[f"cloud/{c}"]
        for k in (1, 10, 32):
            if k + 1 >= x.shape[1]:
                continue
            _, d2 = kr.ranked(x, k + 1)          # ranks 0 .. k + 1
            tied_at_cut |= bool((d2[..., k] == d2[..., k + 1]).any())
        _, d2 = kr.ranked(x, 1)
        coincident |= bool((d2[..., 1] == 0).any())
        if c.startswith("f"):
            # float clouds: no coincident points, so rank 0 is the point itself
            assert (d2[..., 1] > 0).all()
    assert tied_at_cut and coincident
    assert G["feat/cloud"].shape == (2, 65, 3) and G["feat/feats"].shape == (2, 65, 8)
    assert int(G["feat/k"]) == 10 and G["feat/out"].shape == (2, 65, 10, 16)


@pytest.mark.parametrize("key", LATTICE)
def test_lattice_ranked_distances_equal_reference(key):
    x, k, picks = _picks(key)
    idx, d2 = kr.ranked(x, k)
    assert picks.shape == idx.shape                      # min(n, k + 1) columns
    b = x.shape[0]
    ref = np.sort(sqdist(x[:, :, None, :], x[np.arange(b)[:, None, None], picks]), axis=-1)
    assert ref.tobytes() == d2.tobytes()
    # the reference's picks are distinct points, like the contract's
    assert (np.diff(np.sort(picks, -1), axis=-1) > 0).all()
    assert (np.diff(np.sort(idx, -1), axis=-1) > 0).all()


@pytest.mark.parametrize("key", FLOAT)
def test_float_neighbour_sets_equal_reference(key):
    x, k, picks = _picks(key)
    idx, d2 = kr.knn_graph(x, k)
    n = x.shape[1]
    assert picks.shape == (x.shape[0], n, k + 1) and idx.shape == (x.shape[0], n, k)
    assert (picks[..., 0] == np.arange(n)[None, :]).all()            # the dropped column
    assert np.array_equal(np.sort(picks[..., 1:], -1), np.sort(idx, -1))
    assert (np.diff(d2, axis=-1) >= 0).all()


def test_restatement_order_and_drop_rule():
    """Ties go to the lowest index; with coincident points rank 0 is the
    lowest-index point at distance 0, so a row may contain its own index."""
    x = np.zeros((1, 4, 3), np.float32)
    x[0, 3, 0] = 1.0                      # points 0, 1, 2 coincide
    idx, d2 = kr.knn_graph(x, 2)
    assert idx[0].tolist() == [[1, 2], [1, 2], [1, 2], [0, 1]]
    assert d2[0].tolist() == [[0, 0], [0, 0], [0, 0], [1, 1]]
    full, _ = kr.ranked(x, 63)            # kk = n - 1: every point, once
    assert full.shape == (1, 4, 4) and (np.sort(full, -1) == np.arange(4)).all()


def test_restated_features_equal_reference_bytes():
    x, f, k = G["feat/cloud"], G["feat/feats"], int(G["feat/k"])
    idx, _ = kr.knn_graph(x, k)
    out = kr.edge_features(f, idx)
    assert out.dtype == np.float32 and out.shape == G["feat/out"].shape
    assert out.tobytes() == np.ascontiguousarray(G["feat/out"]).tobytes()
    cf = kr.edge_features(f, idx, channels_first=True)
    assert cf.tobytes() == np.ascontiguousarray(np.transpose(G["feat/out"], (0, 3, 1, 2))).tobytes()
    for n in (1, 5):                      # kk = 0 and kk = 4
        xs = np.zeros((2, n, 3), np.float32)
        xs[:, :, 0] = np.arange(n)
        i2, _ = kr.knn_graph(xs, 10)
        got = kr.edge_features(np.zeros((2, n, 8), np.float32), i2)
        assert got.shape == tuple(G[f"shape/n{n}/k10"])
    assert tuple(G["shape/n1/k10"]) == (2, 1, 0, 16) and tuple(G["shape/n5/k10"]) == (2, 5, 4, 16)


def test_entry_points_declared_and_bound():
    from pointcloudregistration_amd import grouping
    hdr = open(os.path.join(ROOT, "include", "pcr_api.h")).read()
    lib = _lib.load()
    for s in ("pcr_knn_graph", "pcr_edge_features"):
        assert s in _lib.SIGNATURES and s in _lib.exported_symbols()
        assert re.search(r"\bint\s+%s\s*\(" % s, hdr)
        assert hasattr(lib, s)
    assert len(_lib.SIGNATURES["pcr_knn_graph"]) == 7
    assert len(_lib.SIGNATURES["pcr_edge_features"]) == 9
    assert {"knn_graph", "graph_features"} <= set(grouping.__all__)
    assert callable(grouping.knn_graph) and callable(grouping.graph_features)


def test_argument_errors_without_gpu():
    lib = _lib.load()
    one = 0x1000   # a non-null address; validation never dereferences it

    def err():
        return lib.pcr_last_error().decode()

    # pcr_knn_graph(xyz, b, n, k, idx, d2, stream)
    assert lib.pcr_knn_graph(None, 1, 8, 4, None, None, None) == -1
    assert "knn_graph" in err() and "null" in err()
    assert lib.pcr_knn_graph(None, 1, 8, 4, one, None, None) == -1 and "null" in err()
    assert lib.pcr_knn_graph(one, 1, 8, 4, None, None, None) == -1 and "null" in err()
    assert lib.pcr_knn_graph(one, 1, 8, 0, one, None, None) == -1
    assert "k=0 outside 1..63" in err()
    assert lib.pcr_knn_graph(one, 1, 8, 64, one, None, None) == -1
    assert "k=64 outside 1..63" in err()
    assert lib.pcr_knn_graph(one, 1, 0, 4, one, None, None) == -1 and "n=0" in err()
    assert lib.pcr_knn_graph(one, -1, 8, 4, one, None, None) == -1 and "negative batch" in err()
    # pcr_edge_features(feats, idx, b, n, c, kk, channels_first, out, stream)
    for cf in (0, 1):
        assert lib.pcr_edge_features(None, None, 1, 8, 4, 4, cf, None, None) == -1
        assert "edge_features" in err() and "null" in err()
        for args in ((None, one, one), (one, None, one), (one, one, None)):
            assert lib.pcr_edge_features(args[0], args[1], 1, 8, 4, 4, cf, args[2], None) == -1
            assert "null" in err()
        assert lib.pcr_edge_features(one, one, 1, 0, 4, 4, cf, one, None) == -1 and "n=0" in err()
        assert lib.pcr_edge_features(one, one, 1, 8, 0, 4, cf, one, None) == -1 and "c=0" in err()
        assert lib.pcr_edge_features(one, one, -1, 8, 4, 4, cf, one, None) == -1
        assert "negative batch" in err()
        assert lib.pcr_edge_features(one, one, 1, 8, 4, -1, cf, one, None) == -1
        assert "kk=-1 outside 0..63" in err()
        assert lib.pcr_edge_features(one, one, 1, 8, 4, 64, cf, one, None) == -1
        assert "kk=64 outside 0..63" in err()


def test_empty_calls_return_ok_without_pointers():
    lib = _lib.load()
    assert lib.pcr_knn_graph(None, 0, 8, 4, None, None, None) == 0       # b = 0
    assert lib.pcr_knn_graph(None, 3, 1, 10, None, None, None) == 0      # n = 1: kk = 0
    assert lib.pcr_edge_features(None, None, 0, 8, 4, 4, 0, None, None) == 0
    assert lib.pcr_edge_features(None, None, 3, 1, 4, 0, 1, None, None) == 0
