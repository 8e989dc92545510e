"""Golden vectors for the landmark branch of f4 (the NDP level optimisation),
generated in the build container by running the reference's own
Deformation_Pyramid (c2p-net/deformationpyramid/model/nets.py, imported from
/root/reference) through the landmark branch of
Registration.optimize_deformation_pyramid (model/registration.py:185-273) on the
CPU in f32.

registration.py itself cannot be imported here (its loss module needs pytorch3d,
absent), so the loop below restates :185-273 line for line, as
make_golden_ndp_opt.py restates the no-landmark branch; the truncated Chamfer
(model/loss.py:60-218) is restated as squared 1-NN distances by brute force.

Two runs at m = 3, iters = 15, N = 1300, M = 1200, L = 97:
  A: w_cd = 0.5, trunc_cd = 0.25, w_reg = 0.05 (registration.py:213-221);
  B: w_cd = 0, w_reg = 0, as config/LNDP.yaml ships (:224-227).  The reference
     raises NameError at :264 in this mode (s_sample_warped is never bound): the
     hist line is left out, nothing else.
Both pyramids start from the initial weights stored in ndp_opt_golden.npz (the
same architecture; make_golden_ndp_opt.py drew them from the reference's own
initialiser), run B's without the nonrigidity branch (w_reg = 0 builds none), so
no weights are stored here.

Clean truncation.  d' jumps at d == trunc, so an f32 trajectory that drifts
across the cut would leave the tolerance of any comparison.  The clouds are
built so that it cannot: both main bodies are the same sphere of radius 0.6 (the
target's mildly deformed, every nearest distance far below sqrt(trunc / 3)),
and each cloud carries two far blobs, mirror images about the centre (so the
means, and with them the centring, stay put) on an axis of its own, several
sqrt(trunc) away from every point of the other cloud.  At every recorded
iteration and in both directions the generator asserts that no distance lies in
[trunc / 3, 3 trunc] and that each side of the cut holds at least 5 % of the
points; it fails otherwise.

Stored: inputs, landmarks, the loss of every iteration, per
level the warped samples (A) and the warped landmarks, and the final warp.
Nothing from the reference is stored except these numbers.

Usage: PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_ndp_ldmk.py
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

CFG = dict(iters=15, lr=0.01, max_break_count=15, break_threshold_ratio=0.001, m=3, k0=-8, depth=3, width=128,
           trunc_cd=0.25)
RUNS = {"A": dict(w_cd=0.5, w_reg=0.05), "B": dict(w_cd=0.0, w_reg=0.0)}
N, M, L, BLOB = 1300, 1200, 97, 70      # BLOB points in each of a cloud's two far blobs (> 5 % each side)


def trunc_chamfer(x, y, trunc, check):
    """loss.py:60-218 for (1, P1, 3) / (1, P2, 3), point mean over the full length."""
    d = ((x[0][:, None, :] - y[0][None, :, :]) ** 2).sum(-1)
    cx, cy = d.min(1)[0], d.min(0)[0]
    for c in (cx, cy):      # the clean cut, both directions, every iteration
        c = c.detach().numpy()
        assert not ((c >= trunc / 3) & (c <= 3 * trunc)).any(), (check, c[(c >= trunc / 3) & (c <= 3 * trunc)])
        assert (c < trunc).mean() >= 0.05 and (c >= trunc).mean() >= 0.05, check
    cx = torch.where(cx >= trunc, torch.zeros_like(cx), cx)
    cy = torch.where(cy >= trunc, torch.zeros_like(cy), cy)
    return cx.sum() / x.shape[1] + cy.sum() / y.shape[1]


def deform(w):
    return w + 0.04 * np.sin(3 * w[:, [1, 2, 0]])


def clouds(rng):
    def sphere(n):
        u = rng.uniform(-1, 1, (n, 3))
        return u / np.linalg.norm(u, axis=1, keepdims=True) * 0.6

    def blobs(axis):
        b = rng.normal(0, 0.05, (BLOB, 3))
        c = np.zeros(3)
        c[axis] = 2.5
        return np.concatenate([b + c, -b - c])     # mirror images: their mean is the origin
    body = sphere(N - 2 * BLOB)
    src = np.concatenate([body, blobs(0)])
    shift = np.array([0.3, -0.1, 0.2])
    tgt = np.concatenate([deform(sphere(M - 2 * BLOB)), blobs(1)]) + shift
    # landmarks: L points of the source body and where the deformation takes them
    pick = np.sort(rng.choice(N - 2 * BLOB, L, replace=False))
    return (src.astype(np.float32), tgt.astype(np.float32), body[pick].astype(np.float32),
            (deform(body[pick]) + shift).astype(np.float32))


def run(NDP, c, src_t, tgt_t, landmarks, out, tag):
    """registration.py:171-287 with self.landmarks set."""
    src_mean = src_t.mean(dim=0, keepdims=True)
    tgt_mean = tgt_t.mean(dim=0, keepdims=True)
    src_pcd, tgt_pcd = src_t - src_mean, tgt_t - tgt_mean
    s_sample, t_sample = src_pcd, tgt_pcd
    src_ldmk = landmarks[0] - src_mean
    tgt_ldmk = landmarks[1] - tgt_mean
    BCE = torch.nn.BCELoss()
    for level in range(NDP.n_hierarchy):
        NDP.gradient_setup(optimized_level=level)
        optimizer = torch.optim.Adam(NDP.pyramid[level].parameters(), lr=c["lr"])
        break_counter, loss_prev, losses = 0, 1e+6, []
        for it in range(c["iters"]):
            if c["w_cd"] > 0:
                src_pts = torch.cat([src_ldmk, s_sample])
                warped_pts, data = NDP.warp(src_pts, max_level=level, min_level=level)
                warped_ldmk = warped_pts[: len(src_ldmk)]
                s_sample_warped = warped_pts[len(src_ldmk):]
                loss_ldmk = torch.mean(torch.sum((warped_ldmk - tgt_ldmk) ** 2, dim=-1))
                loss_CD = trunc_chamfer(s_sample_warped[None], t_sample[None], c["trunc_cd"], (tag, level, it))
                loss = loss_ldmk + c["w_cd"] * loss_CD
            else:
                warped_ldmk, data = NDP.warp(src_ldmk, max_level=level, min_level=level)
                loss = torch.mean(torch.sum((warped_ldmk - tgt_ldmk) ** 2, dim=-1))
            if level > 0 and c["w_reg"] > 0:
                nonrigidity = data[level][1]
                loss = loss + c["w_reg"] * BCE(nonrigidity, torch.zeros_like(nonrigidity))
            losses.append(loss.item())
            if loss.item() < 1e-4:
                break
            if abs(loss_prev - loss.item()) < loss_prev * c["break_threshold_ratio"]:
                break_counter += 1
            if break_counter >= c["max_break_count"]:
                break
            loss_prev = loss.item()
            optimizer.zero_grad()
            loss.backward()
            optimizer.step()
        out[f"{tag}/loss/l{level}"] = np.array(losses)
        out[f"{tag}/ldmk/l{level}"] = (warped_ldmk + tgt_mean).detach().numpy()
        src_ldmk = warped_ldmk.detach()
        if c["w_cd"] > 0:
            out[f"{tag}/hist/l{level}"] = (s_sample_warped + tgt_mean).detach().numpy()
            s_sample = s_sample_warped.detach()
    NDP.gradient_setup(optimized_level=-1)
    with torch.no_grad():
        warped_pcd, _ = NDP.warp(src_pcd)
    out[f"{tag}/warped"] = (warped_pcd + tgt_mean).numpy()


def main():
    sys.path.insert(0, f"{REF}/c2p-net/deformationpyramid")
    from model.nets import Deformation_Pyramid
    src, tgt, sl, tl = clouds(np.random.default_rng(11))
    out = {"src": src, "tgt": tgt, "src_ldmk": sl, "tgt_ldmk": tl}
    init = np.load(os.path.join(HERE, "ndp_opt_golden.npz"))
    for tag, wts in RUNS.items():
        c = dict(CFG, **wts)
        NDP = Deformation_Pyramid(depth=c["depth"], width=c["width"], device="cpu", k0=c["k0"], m=c["m"],
                                  nonrigidity_est=c["w_reg"] > 0, rotation_format="axis_angle", motion="SE3")
        for lvl, layer in enumerate(NDP.pyramid):
            layer.load_state_dict({k: torch.from_numpy(init[f"init/l{lvl}/{k}"]) for k in layer.state_dict()})
        run(NDP, c, torch.from_numpy(src), torch.from_numpy(tgt), (torch.from_numpy(sl), torch.from_numpy(tl)),
            out, tag)
    path = os.path.join(HERE, "ndp_ldmk_golden.npz")
    np.savez_compressed(path, **out)
    print({k: np.round(v, 6).tolist() for k, v in out.items() if "/loss/" in k})
    size, cap = os.path.getsize(path), os.path.getsize(os.path.join(HERE, "ndp_opt_golden.npz"))
    print(size, cap)
    assert size <= cap


if __name__ == "__main__":
    main()
