"""CPU: the inputs of tests/registration_cases.py still reach the branches they are
named for, proved on the oracle alone (oracle/pcr_oracle.c: the sequential RANSAC loop
and icp_core), so an edit to a seed, a noise level or the oracle cannot quietly turn a
case back into an easy one.  The GPU twins, test_ransac_edges_gpu.py and
test_icp_edges_gpu.py, hold csrc/ransac.hip and csrc/icp.hip to the oracle bit for bit
on the same inputs."""
import numpy as np
import pytest

import registration_cases as rc

I4 = np.eye(4)


# ---- RANSAC ------------------------------------------------------------------

def test_tie_rmse_moves_the_best_at_unchanged_fitness(oracle):
    ups = rc.tie_updates(oracle, "tie_rmse")
    ties = [(u, a, b) for u, a, b in ups if a[0] == b[0] and b[1] < a[1]]
    print("tie_rmse updates", [(u, b) for u, _, b in ups], "validated",
          rc.oracle_ransac(oracle, "tie_rmse")["validated"])
    assert len(ties) >= 2
    assert all(b[0] == 1.0 for _, _, b in ties)
    # confidence 1: the bound never shrinks
    assert rc.oracle_ransac(oracle, "tie_rmse")["iters"] == 200


def test_tie_full_keeps_the_earliest_of_equal_hypotheses(oracle):
    ups = rc.tie_updates(oracle, "tie_full")
    top = [(u, b) for u, _, b in ups if b == (1.0, 0.0)]
    assert len(top) == 1 and ups[-1][0] == top[0][0]   # reached once, and never left
    u = top[0][0]
    full = rc.oracle_ransac(oracle, "tie_full")
    upto = rc.oracle_ransac(oracle, "tie_full", max_iteration=u + 1)
    assert full["best_itr"] == u and upto["best_itr"] == u
    assert full["validated"] - upto["validated"] > 10
    # the later ones do reach fitness 1.0: on the noisy twin the same stream moves the
    # best after u, here (rmse 0.0 each time) nothing may
    assert max(v for v, _, _ in rc.tie_updates(oracle, "tie_rmse")) > u


def test_perfect_collapses_the_bound_to_zero(oracle):
    r = rc.oracle_ransac(oracle, "perfect")
    c = rc.rcase("perfect")
    assert rc.corr_inliers(c, r["T"]) == len(c.corr)
    assert oracle.est_k(1.0, 3, c.prm["confidence"]) == 0.0
    assert r["found"] == 1 and r["validated"] == 1
    assert r["iters"] == r["best_itr"] + 1 < c.prm["max_iteration"]


def test_no_inliers_validates_everything_and_finds_nothing(oracle):
    r = rc.oracle_ransac(oracle, "no_inliers")
    assert (r["iters"], r["validated"], r["best_itr"], r["found"]) == (300, 300, -1, 0)
    assert np.array_equal(r["T"], I4) and r["fitness"] == 0.0 and r["inlier_rmse"] == 0.0
    assert len(r["correspondence_set"]) == 0


def test_none_pass_validates_nothing(oracle):
    r = rc.oracle_ransac(oracle, "none_pass")
    assert (r["iters"], r["validated"], r["best_itr"], r["found"]) == (300, 0, -1, 0)
    assert np.array_equal(r["T"], I4)


def test_minus_inf_bound_ends_the_loop(oracle):
    c = rc.rcase("minus_inf_bound")
    r = rc.oracle_ransac(oracle, "minus_inf_bound")
    cin = rc.corr_inliers(c, r["T"])
    print("minus_inf_bound: cin", cin, "iters", r["iters"], "best_itr", r["best_itr"])
    assert cin >= 1 and oracle.est_k(cin / len(c.corr), 8, c.prm["confidence"]) == -np.inf
    assert r["found"] == 1 and r["iters"] == r["best_itr"] + 1 < c.prm["max_iteration"]
    # an earlier hypothesis was accepted without ending it (cin = 0: no bound at all)
    assert rc.oracle_ransac(oracle, "minus_inf_bound", max_iteration=r["best_itr"])["found"] == 1
    # ransac_n = 3 on the same clouds has a finite bound beyond max_iteration
    r3 = rc.run_ransac(oracle, rc.minus_inf_bound(3))
    assert r3["iters"] == c.prm["max_iteration"]


def test_est_k_iters_is_defined_for_every_bound(oracle):
    f = oracle.est_k_iters
    assert [f(x) for x in (-np.inf, -3.5, -0.0, 0.0, 1e-300, 0.5, 1.0, 1.5, 45.0, 99999.01)] == \
        [0, 0, 0, 0, 1, 1, 1, 2, 45, 100000]


def test_round_edges_run_every_iteration(oracle):
    ks = rc.round_edge_iterations(oracle)
    assert set(rc.ROUND_EDGES) <= set(ks)
    ups = [u for u, _, _ in rc.tie_updates(oracle, "tie_rmse")]
    for u in ups:
        if u >= 1:
            # the winner is the last hypothesis of the run, and just outside the next
            assert rc.oracle_ransac(oracle, "tie_rmse", max_iteration=u + 1)["best_itr"] == u
            assert rc.oracle_ransac(oracle, "tie_rmse", max_iteration=u)["best_itr"] < u
    for k in ks:
        r = rc.oracle_ransac(oracle, "tie_rmse", max_iteration=k)
        assert r["iters"] == k, k
    # the long runs still move the best on rmse after the first round
    assert rc.oracle_ransac(oracle, "tie_rmse", max_iteration=5121)["best_itr"] >= 1024


@pytest.mark.parametrize("name", rc.SHAPES)
def test_shapes_are_as_named(oracle, name):
    c = rc.rcase(name)
    r = rc.oracle_ransac(oracle, name)
    n, m, K = len(c.src), len(c.tgt), len(c.corr)
    want = {"n3_m3_k3": (3, 3, 3), "k8_rn8": (65, 65, 8), "n1": (1, 5, 3), "m1": (33, 1, 33)}
    if name in want:
        assert (n, m, K) == want[name]
    else:
        assert n == m == K == int(name[1:])
    if name == "k8_rn8":
        assert c.prm["ransac_n"] == K == 8
    assert r["found"] == 1 and r["validated"] >= 1
    if name == "m1":
        assert len(r["correspondence_set"]) >= 1 and (r["correspondence_set"][:, 1] == 0).all()
    elif name != "n1":
        assert r["fitness"] == 1.0


def test_mixed_batch_holds_every_kind(oracle):
    b, ob = rc.batch(), rc.oracle_batch(oracle)
    assert len(ob) == rc.BATCH_P == 257 and len(set(b["pair_ids"].tolist())) == 257
    by = {k: [r for kk, r in zip(b["kinds"], ob) if kk == k] for k in rc.BATCH_KINDS}
    assert all(len(v) >= 17 for v in by.values())
    # ragged in all three counts
    assert len(set(b["n_src"].tolist())) >= 8 and len(set(b["n_tgt"].tolist())) >= 8
    assert b["n_src"].min() == 0 and b["n_src"].max() == b["src"].shape[1] == 512
    assert b["n_corres"].min() == 2 and b["n_corres"].max() == b["corr"].shape[1]
    assert all(r["fitness"] == 1.0 and r["iters"] == 300 for r in by["tie_rmse"])
    assert sum(r["best_itr"] > 50 for r in by["tie_rmse"]) >= 9   # the best moved late, on rmse
    assert all(r["fitness"] == 1.0 and r["inlier_rmse"] == 0.0 and r["iters"] == 300 for r in by["tie_full"])
    assert all(r["iters"] == r["best_itr"] + 1 <= 3 and r["fitness"] == 1.0 for r in by["perfect"])
    # found == 0 with validated > 0 (a triple draw of one correspondence finds a result)
    none = [r for r in by["no_inliers"] if r["found"] == 0]
    print("no_inliers kind:", len(none), "of", len(by["no_inliers"]), "pairs find nothing")
    assert len(none) >= 5 and all(r["validated"] == 300 for r in by["no_inliers"])
    assert sum((r["validated"], r["found"]) == (0, 0) for r in by["none_pass"]) >= 10
    assert all(r["found"] == -1 and r["iters"] == 0 for r in by["k2_invalid"] + by["n0_invalid"])
    assert all(r["found"] == 1 for k in ("n1", "n3", "n31", "n33", "n63", "n65", "n257") for r in by[k])
    assert any(r["found"] == 0 for r in by["m1"])


# ---- ICP ---------------------------------------------------------------------

def test_icp_cases_reach_their_counts(oracle):
    o = {n: {it: rc.oracle_icp(oracle, n, it) for it in rc.ICP_ITERS} for n in rc.ICP_CASES}
    for n in rc.ICP_CASES:
        print(n, [(r["iters"], r["n_corr"]) for r in o[n].values()])
        assert o[n][0]["iters"] == 0 and np.array_equal(o[n][0]["T"], rc.icase(n).init)
    for n in ("none_identity", "none_init"):
        for it in rc.ICP_ITERS:
            r = o[n][it]
            assert (r["iters"], r["n_corr"]) == (0, 0) and r["T"].tobytes() == rc.icase(n).init.tobytes()
            assert r["fitness"] == 0.0 and r["inlier_rmse"] == 0.0
    assert np.array_equal(rc.icase("none_identity").init, I4)
    assert not np.array_equal(rc.icase("none_init").init, I4)
    for n, k in (("one_corr", 1), ("two_corr", 2), ("n1", 1)):
        assert all(o[n][it]["n_corr"] == k for it in rc.ICP_ITERS), n
        assert o[n][30]["iters"] >= 2      # estimated from k points, and again
    assert len(rc.icase("n1").src) == 1 and len(rc.icase("m1").tgt) == 1
    assert o["m1"][30]["n_corr"] == 33
    for n in rc.ICP_CASES:
        if not n.startswith("none"):
            assert o[n][1]["iters"] == 1 and 2 <= o[n][30]["iters"] < 30, n


def test_icp_at_d_excludes_the_point_on_the_radius(oracle):
    c = rc.icase("at_d")
    assert float(np.float32(c.d * c.d)) == c.d * c.d
    d = c.tgt.astype(np.float64) - c.src.astype(np.float64)
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    assert d2[0] == c.d * c.d and (d2[1:] < c.d * c.d).all()
    assert rc.oracle_icp(oracle, "at_d", 0)["n_corr"] == len(c.src) - 1


def test_icp_float_thr_separates_the_two_thresholds(oracle):
    c = rc.icase("float_thr")
    thr, rr = float(np.float32(c.d * c.d)), c.d * c.d
    x2 = float(c.tgt[0, 0]) * float(c.tgt[0, 0])
    assert thr != rr and (x2 < thr) != (x2 < rr)
    assert (c.src[0] == 0).all() and (c.tgt[0, 1:] == 0).all()
    want = len(c.src) - 1 + int(x2 < thr)
    assert rc.oracle_icp(oracle, "float_thr", 0)["n_corr"] == want


def test_icp_degenerate_clouds(oracle):
    c = rc.icase("dup_targets")
    assert np.array_equal(c.tgt[0::2], c.tgt[1::2])
    c = rc.icase("collinear")
    for a in (c.src, c.tgt):
        s = np.linalg.svd(a.astype(np.float64) - a.astype(np.float64).mean(0), compute_uv=False)
        assert (s > 1e-6 * s[0]).sum() == 1
    c = rc.icase("identical")
    assert (c.src == c.src[0]).all() and (c.tgt == c.tgt[0]).all()
    # every copy's jittered init is a different run; copy 0 is the case itself
    its = {rc.oracle_icp(oracle, "ordinary", 30, k)["iters"] for k in range(40)}
    assert len(its) >= 2
