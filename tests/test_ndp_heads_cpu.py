"""CPU: the nine (motion, rotation format) heads of the NDP level.

a. the f64 restatement (tests/ndp_heads_ref.py) against f64 torch autograd of
   ndp_opt.NDPLayer: every per-point tensor and every parameter gradient to
   1e-12 of the tensor's largest entry (the bar of test_ndp_train_ref_cpu.py);
b. the mirror ndp_opt.NDPLayer in f64 against what the reference's own NDPLayer
   gave (tests/golden/ndp_heads_reference.npz), to 1e-12;
c. an all-zero rotation branch: NaN for axis_angle and quaternion, R = I for
   euler, R = 0 (finite) for 6D, the same pattern in mirror and restatement;
d. the conditioning guards over the whole case list of the GPU tests;
e. the recorded f32 floor (tests/golden/ndp_heads_bounds.npz) is reproducible.
"""
import os

import numpy as np
import pytest
import torch

import ndp_heads_ref as ref
import ndp_train_ref as base
from pointcloudregistration_amd import ndp, ndp_opt

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BOUNDS = os.path.join(GOLDEN, "ndp_heads_bounds.npz")
REFERENCE = os.path.join(GOLDEN, "ndp_heads_reference.npz")
HEAD_IDS = [ref.head_name(*h) for h in ref.HEADS]


# ---- a ---------------------------------------------------------------------

@pytest.mark.parametrize("N", [2, 33])
@pytest.mark.parametrize("depth", [1, 3])
@pytest.mark.parametrize("level", [0, 1])
@pytest.mark.parametrize("head", ref.HEADS, ids=HEAD_IDS)
def test_restatement_matches_f64_autograd(head, level, depth, N):
    motion, fmt = head
    c = ref._case("t", motion, fmt, N, depth, level, 7000 + 10 * N + depth)
    d = ref.make_case(c)
    assert (d["bce_scale"] > 0) == (level > 0)
    want = ref.autograd_step(ref.make_layer(d["P"], torch.float64), torch.from_numpy(d["x"]).double(),
                             torch.from_numpy(d["g"]).double(), d["bce_scale"])
    got = ref.level_step(d["P"], d["x"], d["g"], d["bce_scale"])
    err = ref.group_errors(got, want, motion, fmt)
    assert set(err) == ref.groups_of(motion, fmt) - ({"gw_hid", "gb_hid"} if depth == 1 else set())
    for g, e in err.items():
        assert e <= 1e-12, (g, e)
    assert abs(got["min_preact"] - want["min_preact"]) <= 1e-12
    aux_z, do_z, gw_z = ref.unused_rows(motion, fmt)
    M = ref.row_map(motion, fmt)
    if level == 0:
        do_z, aux_z, gw_z = do_z + [M["nr"]], aux_z + [M["nr"]], gw_z + [M["nr"]]
    assert not got["aux"][aux_z].any() and not got["dO"][do_z].any()
    assert not got["grads"][-2][gw_z].any() and not got["grads"][-1][gw_z].any()


def test_head_zero_is_the_existing_restatement():
    """SE3 / axis_angle here and ndp_train_ref.level_step are the same step in the
    same 8-row layout (two derivations: to 1e-12)."""
    d = ref.make_case(ref._case("t", "SE3", "axis_angle", 33, 3, 1, 5))
    a = ref.level_step(d["P"], d["x"], d["g"], d["bce_scale"])
    b = base.level_step(d["P"], d["x"], d["g"], d["bce_scale"])
    assert a["aux"].shape == b["aux"].shape == (8, 33) and a["grads"][-2].shape == (7, ref.WIDTH)
    for k in ("pe", "H", "aux", "x_out", "dO", "D"):
        assert np.abs(a[k] - b[k]).max() <= 1e-12 * np.abs(b[k]).max(), k
    for ga, gb in zip(a["grads"], b["grads"]):
        assert np.abs(ga - gb).max() <= 1e-12 * np.abs(gb).max()


def test_row_map_is_the_librarys():
    """pcr_ndp_head_rows against the map this file's reference uses."""
    from pointcloudregistration_amd import _lib
    lib = _lib.load()
    for motion, fmt in ref.HEADS:
        M, h = ref.row_map(motion, fmt), ref.head_code(motion, fmt)
        assert h == ndp.head_code(motion, fmt)
        want = [M["rot"], M["n"], M["nw"], M["trn"], M["nr"],
                -1 if M["sc"] is None else M["sc"], -1 if M["rx"] is None else M["rx"]]
        assert [int(lib.pcr_ndp_head_rows(h, k)) for k in range(7)] == want, (motion, fmt)
    assert lib.pcr_ndp_head_rows(9, 0) == -1 and lib.pcr_ndp_head_rows(-1, 0) == -1
    assert lib.pcr_ndp_head_rows(0, 7) == -1
    assert lib.pcr_ndp_train_partial_floats_head(129, 128, 3, 128, 0) == \
        lib.pcr_ndp_train_partial_floats(129, 128, 3, 128)
    W = 128
    assert lib.pcr_ndp_train_partial_floats_head(129, W, 3, 128, 5) == 2 * ((W * 6 + W) + 2 * (W * W + W) + 11 * W + 11)


# ---- b ---------------------------------------------------------------------

@pytest.mark.parametrize("head", ref.HEADS, ids=HEAD_IDS)
def test_mirror_matches_the_reference_module(head):
    motion, fmt = head
    z = np.load(REFERENCE)
    i = [str(n) for n in z["heads"]].index(ref.head_name(motion, fmt))
    d = ref.make_case(ref.fixture_case(motion, fmt))
    L = ref.make_layer(d["P"], torch.float64)
    assert L.motion == motion and L.rotation_format == fmt
    with torch.no_grad():
        xo, nr = L(torch.from_numpy(d["x"]).double())
    want_x, want_s = z["x_out"][i], z["nonrigidity"][i]
    assert np.abs(xo.numpy() - want_x).max() <= 1e-12 * np.abs(want_x).max()
    assert np.abs(nr.numpy() - want_s).max() <= 1e-12 * np.abs(want_s).max()
    # and the restatement's forward is the same map
    rx, rs = ref.forward_only(d["P"], d["x"])
    assert np.abs(rx - want_x).max() <= 1e-12 * np.abs(want_x).max()
    assert np.abs(rs - want_s).max() <= 1e-12 * np.abs(want_s).max()


def test_parameter_names_are_the_references():
    L = ndp_opt.NDPLayer(3, 32, -8, 2, nonrigidity_est=True, rotation_format="quaternion", motion="Sim3")
    names = set(dict(L.named_parameters()))
    assert {"rot_brach.weight", "s_branch.weight", "trn_branch.weight", "nr_branch.weight"} <= names
    assert tuple(L.rot_brach.weight.shape) == (4, 32) and tuple(L.s_branch.weight.shape) == (1, 32)
    assert tuple(ndp_opt.NDPLayer(1, 32, -8, 1, rotation_format="6D").rot_brach.weight.shape) == (6, 32)
    assert not hasattr(ndp_opt.NDPLayer(1, 32, -8, 1, motion="sflow"), "rot_brach")
    P = ndp_opt.DeformationPyramid(2, 32, "cpu", -8, 3, True, rotation_format="euler", motion="Sim3")
    assert [(l.motion, l.rotation_format, l.nonrigidity_est) for l in P.pyramid] == \
        [("Sim3", "euler", False), ("Sim3", "euler", True), ("Sim3", "euler", True)]


def test_unknown_heads_are_refused_with_the_choices():
    with pytest.raises(ValueError, match="SE3.*Sim3.*sflow"):
        ndp_opt.NDPLayer(1, 32, -8, 1, motion="foo")
    with pytest.raises(ValueError, match="axis_angle.*euler.*quaternion.*6D"):
        ndp_opt.NDPLayer(1, 32, -8, 1, rotation_format="rpy")
    with pytest.raises(ValueError, match="SE3.*Sim3.*sflow"):
        ndp.head_code("foo", "euler")


# ---- c ---------------------------------------------------------------------

def zero_rotation_case(motion, fmt, N=33, level=1):
    """A case whose rotation branch is exactly 0 (weights and bias)."""
    d = ref.make_case(ref._case("z", motion, fmt, N, 3, level, 8000 + ref.head_code(motion, fmt)))
    d["P"]["w_rot"] = np.zeros_like(d["P"]["w_rot"])
    d["P"]["b_rot"] = np.zeros_like(d["P"]["b_rot"])
    return d


@pytest.mark.parametrize("head", [h for h in ref.HEADS if h[0] != "sflow"], ids=HEAD_IDS[:8])
def test_zero_rotation_branch(head):
    motion, fmt = head
    d = zero_rotation_case(motion, fmt)
    P, x = d["P"], d["x"].astype(np.float64)
    with torch.no_grad():
        mx, ms = ref.make_layer(P, torch.float64)(torch.from_numpy(x))
    mx, ms = mx.numpy(), ms.numpy()
    rx, rs = ref.forward_only(P, x)
    assert np.array_equal(np.isnan(mx), np.isnan(rx))
    assert np.isfinite(ms).all() and np.isfinite(rs).all()   # s does not depend on the rotation
    if fmt in ("axis_angle", "quaternion"):
        assert np.isnan(mx).all()
        return
    assert np.isfinite(mx).all()
    assert np.abs(mx - rx).max() <= 1e-12
    # what the finite formats must give: R = I (euler), R = 0 (6D)
    one = dict(P, motion="sflow", w_rot=None, b_rot=None, w_s=None, b_s=None)
    t = ref.forward_only(dict(one, w_nr=None, b_nr=None), x)[0] - x        # sflow without blend: y = x + t
    Rx = x if fmt == "euler" else np.zeros_like(x)
    if motion == "Sim3":
        M = ref.row_map(motion, fmt)
        Rx = ref.level_step(P, x, np.zeros_like(x), 0.0)["aux"][M["sc"]][:, None] * Rx
    want = x + rs[:, None] * (Rx + t - x)
    assert np.abs(mx - want).max() <= 1e-12


# ---- d ---------------------------------------------------------------------

def test_case_list_is_the_issue_list():
    assert len(ref.NEW_HEADS) == 8 and ("SE3", "axis_angle") not in ref.NEW_HEADS
    for motion, fmt in ref.NEW_HEADS:
        cs = [c for c in ref.CASES if (c["motion"], c["rotation_format"]) == (motion, fmt)]
        assert [c["N"] for c in cs[:6]] == [1, 31, 32, 33, 65, 129]
        assert all(c["depth"] == 3 and c["level"] == 1 for c in cs[:6])
        assert {(c["depth"], c["level"]) for c in cs} == {(1, 0), (1, 1), (3, 0), (3, 1)}
        sub = [c for c in cs if c["K"] is not None]
        assert len(sub) == 1 and sub[0]["K"] == 23 and sub[0]["N"] == 65
        d = ref.make_case(sub[0])
        assert d["inds"][-1] == 64 and len(np.unique(d["inds"])) == 23   # a hit in the partial tile
        assert np.count_nonzero(d["g"].any(1)) == 23
    assert len({c["name"] for c in ref.CASES}) == len(ref.CASES) == 80
    for i, c in enumerate(ref.CASES):  # the seed rule
        assert c["seed"] == 100 * i + ref.SEED_BUMP.get(c["name"], 0) and 0 <= c["seed"] - 100 * i < 100


@pytest.mark.parametrize("c", ref.CASES, ids=lambda c: c["name"])
def test_guards_hold(c):
    """min |pre-activation| >= 1e-5 (no f32 ReLU mask can differ from the f64 one)
    and every norm a normalising format divides by >= 1e-6, on the restatement
    alone; both are the ones recorded with the floors."""
    d = ref.make_case(c)
    want = ref.level_step(d["P"], d["x"], d["g"], d["bce_scale"])
    assert want["min_preact"] >= ref.GUARD, want["min_preact"]
    fmt, motion = c["rotation_format"], c["motion"]
    expect = set() if motion == "sflow" or fmt == "euler" else \
        {"o_rot", "a1", "resid"} if fmt == "6D" else {"o_rot"}
    assert set(want["norms"]) == expect
    for k, v in want["norms"].items():
        assert v >= ref.NORM_GUARD, (k, v)
    z = np.load(BOUNDS)
    i = [str(n) for n in z["cases"]].index(c["name"])
    assert abs(float(z["min_preact"][i]) - want["min_preact"]) <= 1e-12
    assert float(z["min_norm"][i]) == min(want["norms"].values(), default=np.inf)
    assert np.isfinite(z["floor"][i]).all()


# ---- e ---------------------------------------------------------------------

def test_recorded_floor_is_reproduced():
    """As test_ndp_train_ref_cpu.test_recorded_floor_is_reproduced: each group's
    floor pooled over the case list, a factor 4 either way, plus 1 ulp."""
    z = np.load(BOUNDS)
    assert [str(g) for g in z["groups"]] == list(ref.GROUPS)
    assert [str(n) for n in z["cases"]] == [c["name"] for c in ref.CASES]
    now = []
    for c in ref.CASES:
        d = ref.make_case(c)
        want = ref.level_step(d["P"], d["x"], d["g"], d["bce_scale"])
        L = ref.make_layer(d["P"], torch.float32)
        got = ref.autograd_step(L, torch.from_numpy(d["x"]), torch.from_numpy(d["g"]), d["bce_scale"])
        now.append(ref.group_errors(got, want, c["motion"], c["rotation_format"]))
    ulp = 2.0 ** -23
    rec = ref.load_floors(BOUNDS)
    for g in ref.GROUPS:
        cur = max(e.get(g, 0.0) for e in now)
        assert cur <= 4 * rec[g] + ulp and rec[g] <= 4 * cur + ulp, (g, rec[g], cur)
    b = ref.bounds(rec)
    assert set(b) == set(ref.GROUPS) and all(v >= ref.ULP4 for v in b.values())
