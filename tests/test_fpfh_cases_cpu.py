"""CPU: the inputs of tests/fpfh_cases.py still reach the branches they are named for
(proved from brute-force in-radius counts, so an edit to a seed cannot quietly turn a
case back into an easy one), and on them the f1 oracle (oracle/fpfh_oracle.c) equals
the independent numpy references of tests/fpfh_ref.py: the search exactly, the
normals and FPFH at the bars test_oracle_fpfh.py already uses.  The GPU twin,
test_fpfh_edges_gpu.py, compares csrc/fpfh.hip with both on the same inputs."""
import numpy as np
import pytest

import fpfh_cases as fc
import fpfh_ref


# ---- each case meets the condition it is named for ---------------------------

def test_blob_overflows_the_lds_list_twice():
    _, _, cnt, full = fc.brute("blob", fc.K_LIMIT)
    # more than 2 * 512 in radius: the mid-stream sort-and-cut runs, and runs again
    # on a list that already holds the K kept entries
    assert (full > 2 * fc.LDS_CAP).sum() >= 1000
    # the cut to max_nn is taken at every K the GPU test uses
    for K in fc.SEARCH_K["blob"]:
        assert (full > K).sum() >= 1000, K
    assert (cnt == fc.K_LIMIT).sum() >= 1000


def test_clusters_have_exactly_the_nine_counts():
    _, _, notes = fc.get("clusters")
    _, _, cnt, full = fc.brute("clusters", fc.K_LIMIT)
    sizes = np.array(fc.CLUSTER_SIZES)
    assert np.array_equal(full, sizes[notes["label"]])
    assert np.array_equal(np.unique(full), sizes)
    # K - 1, K, K + 1; cap - 1, cap (the exactly-full sort), cap + 1 (the smallest
    # overflow); and one more full ballot of 64 on top of each of those
    assert set(sizes) == {fc.K_LIMIT + d for d in (-1, 0, 1)} | {fc.LDS_CAP + d for d in (-1, 0, 1)} | \
        {fc.LDS_CAP + fc.WAVE + d for d in (-1, 0, 1)}
    assert np.array_equal(cnt, np.minimum(full, fc.K_LIMIT))


def test_lattice_has_pairs_on_the_threshold_and_ties_across_the_cut():
    p, r, notes = fc.get("lattice")
    thr = float(np.float32(r * r))
    assert thr == 0.0625 == r * r
    P = p.astype(np.float64)
    on = 0
    for i0 in range(0, len(P), 512):
        d = P[i0:i0 + 512, None, :] - P[None, :, :]
        on += int((((d[..., 0] ** 2 + d[..., 1] ** 2) + d[..., 2] ** 2) == thr).sum())
    assert on == notes["on_thr_pairs"] == 9126
    idx, d2, cnt, full = fc.brute("lattice", 100)
    assert full.max() == 251 and (full > 100).sum() == 2033
    assert (d2 < thr).all()
    # a tie group straddles the cut: the last kept and the first dropped entry have the
    # same d2, so only the index decides which stays
    _, d2f, _, _ = fc.brute("lattice", fc.K_LIMIT)
    cut = full > 100
    assert (d2f[cut, 99] == d2f[cut, 100]).sum() > 500


def test_identical_is_one_600_way_tie():
    idx, d2, cnt, full = fc.brute("identical", fc.K_LIMIT)
    assert (full == 600).all() and 600 > fc.LDS_CAP
    assert (d2 == 0.0).all()
    assert np.array_equal(idx, np.tile(np.arange(fc.K_LIMIT, dtype=np.int32), (600, 1)))


def test_sparse_holds_the_short_lists_and_the_rank_deficient_ones():
    p, r, notes = fc.get("sparse")
    idx, d2, cnt, full = fc.brute("sparse", 100)
    rows = notes["rows"]
    for g, k in (("g1", 1), ("g2", 2), ("g3", 3), ("g4", 4)):
        a, b = rows[g]
        assert b - a == k and (full[a:b] == k).all(), g
    # the parts do not see each other: every list stays inside its own part
    for a, b in rows.values():
        j = idx[a:b][idx[a:b] >= 0]
        assert j.min() >= a and j.max() < b
    P = p.astype(np.float64)
    for part, rank in (("line", 1), ("plane", 2)):
        a, b = rows[part]
        assert b - a == 200 and (full[a:b] >= 3).all()
        q = P[a:b] - P[a:b].mean(0)
        s = np.linalg.svd(q, compute_uv=False)
        assert (s > 1e-12 * s[0]).sum() == rank, part
    assert (full > 30).any()      # the plane is cut at the normals' K = 30


def test_blob400_lists_are_longer_than_a_wave():
    _, _, cnt, full = fc.brute("blob400", 100)
    assert (full > fc.WAVE).sum() >= 250 and (cnt == 100).sum() >= 250


# ---- the oracle against the independent references ---------------------------

@pytest.mark.parametrize("name,K", [(n, K) for n in fc.CASES for K in fc.SEARCH_K[n]])
def test_oracle_search_equals_brute_force(oracle, name, K):
    idx, d2, cnt = fc.oracle_search(oracle, name, K)
    b_idx, b_d2, b_cnt, _ = fc.brute(name, K)
    assert np.array_equal(cnt, b_cnt)
    assert np.array_equal(idx, b_idx)
    assert np.array_equal(d2, b_d2)


@pytest.mark.parametrize("with_prior", [False, True])
@pytest.mark.parametrize("name", list(fc.NORMALS_K))
def test_oracle_normals_against_eigh(oracle, name, with_prior):
    p, r, notes = fc.get(name)
    idx, _, cnt, _ = fc.brute(name, fc.NORMALS_K[name])
    v0, ok = fpfh_ref.eigh_normals(p, idx, cnt)
    nm = fc.oracle_normals(oracle, name, with_prior)
    err = np.abs(np.abs(np.einsum("ij,ij->i", nm, v0)) - 1.0)
    print(f"{name}: ok {ok.sum()} of {(cnt >= 3).sum()} with cnt >= 3, worst |n.v0| error "
          f"{err[ok].max() if ok.any() else 0.0:.3g}")
    assert (err[ok] < 1e-7).all()
    if not (name == "identical" and with_prior):   # there the result is the prior, unnormalised
        assert np.allclose(np.linalg.norm(nm, axis=1), 1.0, atol=1e-12)
    if with_prior:
        assert (np.einsum("ij,ij->i", nm, fc.prior(name)) >= 0.0).all()
    if name in ("blob", "blob400"):
        assert ok.sum() > 0 and ((cnt >= 3) & ~ok).sum() <= 0.05 * (cnt >= 3).sum()
    if name == "clusters":
        assert ok.all()
    if name == "identical":
        # zero covariance: no eigenvector, so (0, 0, 1) or the prior itself
        assert not ok.any()
        assert np.array_equal(nm, fc.prior(name) if with_prior else np.tile([0.0, 0.0, 1.0], (len(p), 1)))
    if name == "sparse":
        rows = notes["rows"]
        a, b = rows["line"]
        assert not ok[a:b].any()          # rank 1: the eigenvector is not unique
        for g in ("plane", "g3", "g4"):
            a, b = rows[g]
            assert ok[a:b].all(), g
        a, b = rows["plane"]
        assert (np.abs(np.abs(nm[a:b] @ notes["plane_normal"]) - 1.0) < 1e-7).all()
        a, b = rows["g1"][0], rows["g2"][1]   # fewer than 3 neighbours: (0, 0, 1), prior's sign
        up = np.tile([0.0, 0.0, 1.0], (b - a, 1))
        want = np.where(fc.prior(name)[a:b, 2:] < 0.0, -up, up) if with_prior else up
        assert np.array_equal(nm[a:b], want)


def test_oracle_fpfh_against_numpy_on_blob400(oracle):
    sp, fp = fc.oracle_fpfh(oracle, "blob400", 100)
    sp2, fp2 = fc.blob400_numpy(oracle)
    s_sp, s_fp = np.mean(np.abs(sp - sp2) < 1e-9), np.mean(np.abs(fp - fp2) < 1e-6)
    print(f"blob400 K 100: SPFH share {s_sp}, FPFH share {s_fp}")
    # libm vs the det_* functions only matter within ulps of a bin edge
    assert s_sp > 0.999
    assert s_fp > 0.999


@pytest.mark.parametrize("name,K", [(n, K) for n in fc.FPFH_K for K in fc.FPFH_K[n]])
def test_oracle_fpfh_group_sums(oracle, name, K):
    sp, fp = fc.oracle_fpfh(oracle, name, K)
    _, _, cnt, _ = fc.brute(name, K)
    lv = fc.live(name, K)
    if K == 1:
        assert not lv.any() and (sp == 0).all() and (fp == 0).all()
        return
    assert (sp[cnt <= 1] == 0).all() and (fp[cnt <= 1] == 0).all()
    np.testing.assert_allclose(sp[cnt > 1].reshape(-1, 3, 11).sum(2), 100.0, rtol=1e-12)
    np.testing.assert_allclose(fp[lv].reshape(-1, 3, 11).sum(2), 200.0, rtol=1e-12)
    # every neighbour at d2 == 0 is skipped: the FPFH is the point's own SPFH
    rest = (cnt > 1) & ~lv
    assert np.array_equal(fp[rest], sp[rest])
    if name == "identical":
        assert rest.all()
        # a coincident pair has the zero feature: bins 5, 5, 5
        assert (sp[:, [5, 16, 27]] > 99.0).all()
    else:
        assert lv.any()
