"""CPU: the f64 restatement of one NDP level step (tests/ndp_train_ref.py)
against f64 torch autograd of ndp_opt.NDPLayer -- every per-point quantity (the
Linear outputs through forward hooks, their gradients through
torch.autograd.grad) and every parameter gradient, to 1e-12 of each tensor's
largest entry (both sides f64, different summation order).  Then the ReLU-kink
guard and the recorded f32 floor (tests/golden/ndp_train_bounds.npz) over the
whole case list of the GPU tests, so a bad seed or a stale bounds file is caught
without a GPU."""
import os

import numpy as np
import pytest
import torch

import ndp_train_ref as ref

BOUNDS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ndp_train_bounds.npz")


@pytest.mark.parametrize("N", [2, 33, 257])
@pytest.mark.parametrize("bce", [False, True])
@pytest.mark.parametrize("level", [0, 2])
@pytest.mark.parametrize("depth", [1, 3, 5])
def test_restatement_matches_f64_autograd(depth, level, bce, N):
    c = dict(name="t", N=N, depth=depth, level=level, seed=7000 + 10 * N + depth, bce=bce, chunks=(128,), K=None)
    d = ref.make_case(c)
    assert (d["bce_scale"] > 0) == (bce and level > 0)
    want = ref.autograd_step(ref.make_layer(d["P"], torch.float64), torch.from_numpy(d["x"]).double(),
                             torch.from_numpy(d["g"]).double(), d["bce_scale"])
    got = ref.level_step(d["P"], d["x"], d["g"], d["bce_scale"])
    err = ref.group_errors(got, want)
    assert set(err) == set(ref.GROUPS) - ({"gw_hid", "gb_hid"} if depth == 1 else set())
    for g, e in err.items():
        assert e <= 1e-12, (g, e)
    assert abs(got["min_preact"] - want["min_preact"]) <= 1e-12
    assert not got["aux"][7].any() and not got["dO"][7].any()
    if level == 0:  # no nonrigidity branch: s, its gradient rows and row 6 of the branch gradients are 0
        assert not got["aux"][6].any() and not got["dO"][6].any()
        assert not got["grads"][-2][6].any() and got["grads"][-1][6] == 0


def test_restatement_handles_one_point():
    """N = 1 (NDPLayer.forward's squeeze() changes shape there, so autograd is
    not asked): the per-point quantities of a single point equal that point's
    column of a 5-point run with the same parameters and the same bce_scale."""
    c = dict(name="t", N=5, depth=3, level=1, seed=7001, bce=True, chunks=(128,), K=None)
    d = ref.make_case(c)
    full = ref.level_step(d["P"], d["x"], d["g"], 0.05)
    one = ref.level_step(d["P"], d["x"][3:4], d["g"][3:4], 0.05)
    for k in ("pe", "H", "aux", "dO", "D"):
        assert one[k].shape[-1] == 1
        np.testing.assert_allclose(one[k][..., 0], full[k][..., 3], rtol=1e-13, atol=0)
    np.testing.assert_allclose(one["x_out"][0], full["x_out"][3], rtol=1e-13, atol=0)
    np.testing.assert_allclose(one["grads"][1], one["D"][0][:, 0], rtol=0, atol=0)


def test_case_list_is_the_issue_list():
    by = {c["name"]: c for c in ref.CASES}
    assert [c["N"] for c in ref.CASES[:11]] == [1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 257]
    assert all(c["depth"] == 3 and c["level"] == 1 and c["bce"] and c["chunks"] == (128,) for c in ref.CASES[:11])
    assert {(c["depth"], c["level"]) for c in ref.CASES[11:19]} == {(d, lv) for d in (1, 2, 3, 5) for lv in (0, 2)}
    assert all(c["N"] == 129 for c in ref.CASES[11:19])
    assert not by["nobce"]["bce"] and by["nobce"]["level"] == 1
    assert by["chunks"]["N"] == 513 and by["chunks"]["depth"] == 2 and by["chunks"]["chunks"] == (64, 128, 192, 576)
    assert [-(-513 // ch) for ch in by["chunks"]["chunks"]] == [9, 5, 3, 1]
    for n, K in (("sub1", 1), ("sub23", 23)):
        d = ref.make_case(by[n])
        assert by[n]["N"] == 65 and len(d["inds"]) == K == len(np.unique(d["inds"]))
        assert np.array_equal(d["g"][d["inds"]], d["gsub"]) and np.count_nonzero(d["g"].any(1)) == K
    assert ref.make_case(by["sub23"])["inds"][-1] == 64  # a hit in the partial tile
    assert [(c["N"], c["depth"], c["level"]) for c in ref.BIG_CASES] == [(3000, 3, lv) for lv in (0, 1, 5)]


@pytest.mark.parametrize("c", ref.CASES + ref.BIG_CASES, ids=lambda c: c["name"])
def test_guard_holds(c):
    """The f64 minimum |pre-activation| of the case is >= GUARD (1e-5, about 100
    times the f32 forward error: no f32 ReLU mask can differ from the f64 one),
    and it is the one recorded with the floors."""
    d = ref.make_case(c)
    want = ref.level_step(d["P"], d["x"], d["g"], d["bce_scale"])
    assert want["min_preact"] >= ref.GUARD, want["min_preact"]
    z = np.load(BOUNDS)
    i = [str(n) for n in z["cases"]].index(c["name"])
    assert abs(float(z["min_preact"][i]) - want["min_preact"]) <= 1e-12
    assert np.isfinite(z["floor"][i]).all()


def test_recorded_floor_is_reproduced():
    """The committed floors are what f32 autograd gives here, to its run-to-run
    variation.  One case's largest error moves with the BLAS blocking and the
    thread count (a 3000-term f32 sum was seen to move by 6 x between two
    machines), so the comparison is on what the GPU tests use: each group's floor
    pooled over the case list, a factor 4 either way, plus 1 ulp."""
    z = np.load(BOUNDS)
    now = {}
    for c in ref.CASES + ref.BIG_CASES:
        d = ref.make_case(c)
        want = ref.level_step(d["P"], d["x"], d["g"], d["bce_scale"])
        L = ref.make_layer(d["P"], torch.float32)
        got = ref.autograd_step(L, torch.from_numpy(d["x"]), torch.from_numpy(d["g"]), d["bce_scale"])
        now[c["name"]] = ref.group_errors(got, want)
    ulp = 2.0 ** -23
    for big in (False, True):
        rec = ref.load_floors(BOUNDS, big=big)
        for g in ref.GROUPS:
            cur = max(e.get(g, 0.0) for n, e in now.items() if big or not n.startswith("big-"))
            assert cur <= 4 * rec[g] + ulp and rec[g] <= 4 * cur + ulp, (g, rec[g], cur)


def test_bounds_are_not_looser_than_before():
    """No group bound may be looser than what test_ndp_train_gpu.py always
    asserted: 2e-6 absolute on x' (|x'| < 1.1 for |x| <= 0.8 warped by these
    layers), 2e-4 of the largest entry on gradients."""
    assert [str(g) for g in np.load(BOUNDS)["groups"]] == list(ref.GROUPS)
    for big in (False, True):
        b = ref.bounds(ref.load_floors(BOUNDS, big=big))
        assert set(b) == set(ref.GROUPS)
        assert b["xy"] * 1.1 <= 2e-6 and b["s"] <= 2e-6
        for g in ref.GRAD_GROUPS:
            assert ref.ULP4 <= b[g] <= 2e-4, (g, b[g])
