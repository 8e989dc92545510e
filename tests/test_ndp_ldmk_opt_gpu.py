"""GPU: the landmark branch of the NDP level optimisation
(ndp_opt.optimize_deformation_pyramid(..., landmarks=...), fused and torch paths)
against the reference's own Deformation_Pyramid run through the landmark branch
of registration.py's loop on the CPU (tests/golden/ndp_ldmk_golden.npz,
make_golden_ndp_ldmk.py): mode A (landmark term + w_cd truncated Chamfer + BCE)
and mode B (the landmark term alone, as config/LNDP.yaml ships).

Tolerances: those of tests/test_ndp_opt_gpu.py for this loop, with its
reasoning -- the first loss of every level depends only on the inputs and the
initial weights (f32 forward, different summation orders): 2e-6 relative; later
iterations follow Adam trajectories whose normalised steps amplify f32 rounding
of near-zero gradients: 2e-3 relative on the losses, 2e-3 absolute on points
(clouds of radius 0.6, blobs at 2.5).  The fixture's truncation is clean by
construction (no distance within a factor 3 of trunc_cd at any iteration of the
generator), so no trajectory crosses the cut.

Observed on an MI355X against these tolerances: fused loop 2.0e-7 (first
losses), 3.0e-7 (all losses), 1.4e-6 (points); torch path 1.7e-7, 2.6e-7, 1.4e-6.
The landmark trajectories did not need more than the existing tolerances, so
none was derived from a measured spread.
"""
import os

import numpy as np
import pytest
import torch

from pointcloudregistration_amd import c2p, ndp_opt, synth
from pointcloudregistration_amd.ndp_opt import NDPConfig

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "ndp_ldmk_golden.npz")
INIT = os.path.join(HERE, "golden", "ndp_opt_golden.npz")   # the initial weights (make_golden_ndp_ldmk.py)
CFG = dict(iters=15, lr=0.01, max_break_count=15, break_threshold_ratio=0.001, m=3, k0=-8, depth=3, width=128,
           trunc_cd=0.25)
RUNS = {"A": dict(w_cd=0.5, w_reg=0.05), "B": dict(w_cd=0.0, w_reg=0.0)}


def _pyramid(cfg):
    init = np.load(INIT)
    P = ndp_opt.DeformationPyramid(cfg["depth"], cfg["width"], torch.device("cuda"), cfg["k0"], cfg["m"],
                                   cfg["w_reg"] > 0)
    for lvl, layer in enumerate(P.pyramid):
        layer.load_state_dict({k: torch.from_numpy(init[f"init/l{lvl}/{k}"]) for k in layer.state_dict()})
    return P


def _run(tag, **kw):
    g = np.load(GOLD)
    cfg = dict(CFG, **RUNS[tag])
    return g, ndp_opt.optimize_deformation_pyramid(
        torch.from_numpy(g["src"]).cuda(), torch.from_numpy(g["tgt"]).cuda(), None, cfg, NDP=_pyramid(cfg),
        landmarks=(g["src_ldmk"], g["tgt_ldmk"]), **kw)


def _check_against_golden(tag, g, out, fused):
    warped, hist, _, info = out
    worst = dict(first=0.0, loss=0.0, pts=0.0)
    for lvl in range(3):
        want, got = g[f"{tag}/loss/l{lvl}"], info[lvl]["losses"]
        assert info[lvl]["mode"] == tag and info[lvl]["mlp"] == ("fused" if fused else "torch")
        assert info[lvl]["chamfer"] == ("none" if tag == "B" else "fused" if fused else "nnd")
        assert info[lvl]["evaluated"] == len(want), (lvl, info[lvl]["evaluated"], len(want))
        worst["first"] = max(worst["first"], abs(got[0] - want[0]) / abs(want[0]))
        worst["loss"] = max(worst["loss"], float(np.abs(got / want - 1).max()))
        pts = [(info[lvl]["ldmk"], g[f"{tag}/ldmk/l{lvl}"])]
        if tag == "A":
            pts.append((hist[lvl], g[f"{tag}/hist/l{lvl}"]))
        for a, b in pts:
            assert a.shape == b.shape
            worst["pts"] = max(worst["pts"], float(np.abs(a - b).max()))
    assert hist.shape == ((4, 1300, 3) if tag == "A" else (1, 1300, 3))
    w = warped.cpu().numpy()
    assert np.array_equal(hist[-1], w)
    worst["pts"] = max(worst["pts"], float(np.abs(w - g[f"{tag}/warped"]).max()))
    print(f"ldmk loop mode {tag}, fused={fused}: first loss {worst['first']:.2e} (2e-6), "
          f"losses {worst['loss']:.2e} (2e-3), points {worst['pts']:.2e} (2e-3)")
    assert worst["first"] <= 2e-6 and worst["loss"] <= 2e-3 and worst["pts"] <= 2e-3, worst


@pytest.mark.parametrize("use_graph", [True, False])
@pytest.mark.parametrize("tag", ["A", "B"])
def test_fused_loop_matches_reference_loop(tag, use_graph):
    g, out = _run(tag, use_graph=use_graph)
    _check_against_golden(tag, g, out, True)


@pytest.mark.parametrize("tag", ["A", "B"])
def test_torch_path_matches_reference_loop(tag):
    g, out = _run(tag, fused=False)
    _check_against_golden(tag, g, out, False)


@pytest.mark.parametrize("tag", ["A", "B"])
def test_graph_eager_and_repeat_are_bit_equal(tag):
    """Same kernels, same order: the replayed graph is the eager loop, and a
    second run repeats the first (fixed reduction orders, no float atomics)."""
    _, a = _run(tag, use_graph=True)
    _, b = _run(tag, use_graph=False)
    _, c = _run(tag, use_graph=True)
    for o in (b, c):
        assert torch.equal(a[0], o[0]) and np.array_equal(a[1], o[1])
        for x, y in zip(a[3], o[3]):
            assert np.array_equal(x["losses"], y["losses"]) and np.array_equal(x["ldmk"], y["ldmk"])


def test_without_landmarks_nothing_changed():
    """landmarks=None is the code path of tests/test_ndp_opt_gpu.py: its golden,
    its tolerances, and no landmark entries beyond mode None."""
    g = np.load(INIT)
    cfg = dict(CFG, w_reg=0.05)
    a, b = (ndp_opt.optimize_deformation_pyramid(torch.from_numpy(g["src"]).cuda(), torch.from_numpy(g["tgt"]).cuda(),
                                                 g["inds"], cfg, NDP=_pyramid(cfg), landmarks=None) for _ in range(2))
    warped, hist, _, info = a
    for lvl in range(3):
        want, got = g[f"loss/l{lvl}"], info[lvl]["losses"]
        assert info[lvl]["mode"] is None and "ldmk" not in info[lvl] and info[lvl]["chamfer"] == "fused"
        assert info[lvl]["evaluated"] == len(want)
        assert abs(got[0] - want[0]) <= 2e-6 * abs(want[0])
        np.testing.assert_allclose(got, want, rtol=2e-3)
        np.testing.assert_allclose(hist[lvl], g[f"hist/l{lvl}"], atol=2e-3)
    np.testing.assert_allclose(warped.cpu().numpy(), g["warped"], atol=2e-3)
    assert torch.equal(a[0], b[0])


def test_mode_a_above_the_fused_chamfer_limit_takes_nnd_path():
    """K = N or M above pcr_ndp_chamfer_max_points(): the Chamfer part runs on the
    nnd kernels and cd_scale applies to gsub; same loss on a problem cut to the
    limit's fused pass at the first iteration."""
    from pointcloudregistration_amd import _lib
    lim = int(_lib.load().pcr_ndp_chamfer_max_points())
    rng = np.random.default_rng(5)
    tgt = rng.uniform(-0.5, 0.5, (lim + 500, 3)).astype(np.float32)
    src = (tgt[:2000] + rng.normal(0, 0.01, (2000, 3))).astype(np.float32)
    ld = (src[:40], tgt[:40])
    cfg = dict(CFG, iters=3, m=1, w_cd=0.5, w_reg=0.05)
    _, _, _, info = ndp_opt.optimize_deformation_pyramid(src, tgt, None, cfg, NDP=_pyramid(cfg), landmarks=ld)
    assert info[0]["chamfer"] == "nnd" and info[0]["mlp"] == "fused" and info[0]["mode"] == "A"
    losses = info[0]["losses"]
    assert len(losses) == 3 and np.isfinite(losses).all() and losses[-1] < losses[0]
    _, _, _, ref = ndp_opt.optimize_deformation_pyramid(src, tgt, None, cfg, NDP=_pyramid(cfg), landmarks=ld,
                                                        fused=False)
    np.testing.assert_allclose(losses, ref[0]["losses"], rtol=2e-3)
    assert abs(losses[0] - ref[0]["losses"][0]) <= 2e-6 * abs(losses[0])


def test_landmark_value_errors():
    src, tgt = np.zeros((10, 3), np.float32), np.ones((12, 3), np.float32)
    ok = np.zeros((4, 3), np.float32)
    for bad in ((np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32)),      # L = 0
                (ok, np.zeros((5, 3), np.float32)),                                 # shape mismatch
                (np.zeros((4, 2), np.float32), np.zeros((4, 2), np.float32)),      # not (L, 3)
                (np.zeros(12, np.float32), np.zeros(12, np.float32)),
                (ok,), ok[0, 0]):
        with pytest.raises(ValueError):
            ndp_opt.optimize_deformation_pyramid(src, tgt, None, dict(CFG, m=1, iters=1), landmarks=bad)
    with pytest.raises(ValueError):
        c2p.register_c2p(src, tgt, [], [], 0.05, landmarks="lepard")


def _c5_case(seed, n=3000):
    """The fixture of tests/test_c2p_gpu.py::test_c5_composed_flow_vs_oracle_chain."""
    B = synth.make_batch(1, n=n, m=n, d=32, base_seed=seed)
    rng = np.random.default_rng(seed)
    fs = [B.src_feat[0]] + [(B.src_feat[0] + rng.normal(0, 0.6, B.src_feat[0].shape)).astype(np.float32)
                            for _ in range(2)]
    ft = [B.tgt_feat[0]] + [(B.tgt_feat[0] + rng.normal(0, 0.6, B.tgt_feat[0].shape)).astype(np.float32)
                            for _ in range(2)]
    return B, fs, ft


@pytest.mark.parametrize("w_cd,w_reg,mode", [(0.5, 0.05, "A"), (0.0, 0.0, "B")])
def test_register_c2p_with_ransac_landmarks(w_cd, w_reg, mode):
    """The RANSAC inlier correspondences as landmarks, on the fixture of the
    existing C2P test; mode B with the weights config/LNDP.yaml ships.  The
    residual the NDP stage starts with is that of its own output before any
    optimisation: the reference cancels the global translation (both clouds and
    their landmarks are centred by the clouds' means, the result is shifted by
    the target's), so an identity warp returns estimate - mean(estimate) +
    mean(target), and the landmarks' mean squared residual there is the start.
    The figure in the frame of `estimate` is printed next to it."""
    B, fs, ft = _c5_case(41)
    cfg = NDPConfig(iters=15, m=3, width=128, w_cd=w_cd, w_reg=w_reg, trunc_cd=0.25)
    torch.manual_seed(0)
    res = c2p.register_c2p(B.src[0], B.tgt[0], fs, ft, 0.04, ndp_config=cfg, seed=9, pair_id=4, landmarks="ransac")
    info, corrs = res["info"], res["corrs"]
    assert [i["mode"] for i in info] == [mode] * 3 and info[0]["mlp"] == "fused"
    # the landmarks are the inlier correspondences the call holds
    sl, tl = res["landmarks"]
    L = corrs.numel()
    assert L >= 1 and sl.shape == tl.shape == (L, 3) and torch.equal(sl, res["estimate"][corrs])
    w = res["warped"]
    assert w.shape == (B.src.shape[1], 3) and bool(torch.isfinite(w).all())
    assert res["hist"].shape[0] == (4 if mode == "A" else 1) and np.array_equal(res["hist"][-1], w.cpu().numpy())
    shift = torch.from_numpy(B.tgt[0]).cuda().mean(0) - res["estimate"].mean(0)
    start = float(((sl + shift - tl) ** 2).sum(-1).mean())
    end = float(((torch.from_numpy(info[-1]["ldmk"]).cuda() - tl) ** 2).sum(-1).mean())
    raw = float(((sl - tl) ** 2).sum(-1).mean())
    print(f"register_c2p landmarks=ransac mode {mode}: L = {L}, residual {start:.3e} -> {end:.3e} "
          f"(in the frame of estimate: {raw:.3e})")
    assert end < start, (start, end)
