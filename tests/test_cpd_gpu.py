"""GPU: pcr_cpd_estep / pcr_cpd_register and the cpd module against the f64
restatement of the contract (tests/cpd_ref.py).

Tolerances are measured, not fixed: probreg's dense formulation is evaluated in
numpy f32 on the CPU (cpd_ref.estep_f32) and its distance from f64, per output
and normalised by the output's largest magnitude, is what the kernels may
exceed at most 4 times (the margin the PPF channels got), floored at 4 * 2^-24
for the rounding of the f32 outputs themselves.  The loop is held to 4 times the
deviation of the restatement driven by the f32 program from the one driven by
f64, floored at 2^-20 for T and relatively for sigma2 and q."""
import functools

import numpy as np
import pytest
import torch

import cpd_ref as cr
from pointcloudregistration_amd import _lib, cpd

pytestmark = pytest.mark.gpu
F32 = np.float32
CHUNK = 512      # the sums' chunk and the sweeps' LDS stage (include/pcr_api.h)
FLOOR_E = 4 * 2.0 ** -24
FLOOR_L = 2.0 ** -20
T_PROBE = np.eye(4)
T_PROBE[:3, :3] = cr.rot_z(0.3) * 0.9
T_PROBE[:3, 3] = (0.05, -0.1, 0.2)

# (P, M, N): one lane, one group, group and tile edges, two tiles and a batch, one
# LDS chunk + 1 on either axis, and a split of either sweep (one pair, > 1 chunk)
SHAPES = [(1, 1, 1), (1, 1, 65), (1, 65, 1), (1, 63, 64), (1, 64, 65), (2, 257, 200), (1, CHUNK + 1, 70),
          (1, 70, CHUNK + 1), (1, 1100, 300), (1, 300, 1100)]
FAR = {(1, 64, 65), (2, 257, 200)}     # shapes with targets no source reaches


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def make_pair(M, N, sigma2, seed, far):
    """Unit-cube sources Y and targets near the transformed sources, so that every
    target column's largest exponent argument is far above -80 -- or, for the
    `far` columns, every argument is below -120."""
    rng = np.random.default_rng(seed)
    Y = rng.random((M, 3), dtype=F32)
    ys = cr.apply_T(T_PROBE, Y)
    X = (ys[rng.integers(0, M, N)] + rng.normal(0, 0.3 * np.sqrt(sigma2), (N, 3))).astype(F32)
    nfar = min(3, N - 1) if far else 0
    X[:nfar] += F32(9.0)
    colmax = cr.column_max_args(ys, X, sigma2)
    assert ((colmax > -80) | (colmax < -120)).all()          # the issue's condition
    assert (colmax[nfar:] > -40).all() and (colmax[:nfar] < -120).all()
    return Y, X


def gpu_estep(src, tgt, n_src, n_tgt, sigma2, w, transform=T_PROBE):
    out = cpd.expectation_step(dev(src), dev(tgt), sigma2, w, transform=transform,
                               n_src=None if n_src is None else dev(np.asarray(n_src, np.int32)),
                               n_tgt=None if n_tgt is None else dev(np.asarray(n_tgt, np.int32)))
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in out]


def check_estep(got, Y, X, sigma2, w, what):
    """One pair's (pt1, p1, px, n_p) against f64, within 4x the f32 program's own error."""
    ys = cr.apply_T(T_PROBE, Y)
    want, prog = cr.estep(ys, X, sigma2, w), cr.estep_f32(ys, X, sigma2, w)
    for name, g, w64, p32 in zip(("pt1", "p1", "px", "n_p"), got, want, prog):
        e_prog, e_gpu = cr.rel_err(p32, w64), cr.rel_err(g, w64)
        tol = max(4 * e_prog, FLOOR_E)
        print(f"{what} {name}: kernel {e_gpu:.3e}  f32 program {e_prog:.3e}  tol {tol:.3e}")
        assert e_gpu <= tol, (what, name, e_gpu, e_prog)


@pytest.mark.parametrize("w", [0.0, 0.1])
@pytest.mark.parametrize("sigma2", [1e-1, 1e-2, 1e-3])
@pytest.mark.parametrize("P,M,N", SHAPES)
def test_estep_matches_f64(P, M, N, sigma2, w):
    pairs = [make_pair(M, N, sigma2, 1000 * M + N + p, (P, M, N) in FAR) for p in range(P)]
    got = gpu_estep(np.stack([a for a, _ in pairs]), np.stack([b for _, b in pairs]), None, None, sigma2, w)
    for p, (Y, X) in enumerate(pairs):
        check_estep([got[0][p], got[1][p], got[2][p], got[3][p]], Y, X, sigma2, w, f"({P},{M},{N}) s2={sigma2} w={w} p{p}")
    if (P, M, N) in FAR:    # the FLT_EPSILON rule, where f32 and f64 agree that the sum is 0
        c = cr.const_c(sigma2, w, M, N)
        assert (got[0][:, :3] == F32(cr.FLT_EPSILON / (cr.FLT_EPSILON + c))).all()


def test_split_shapes_take_the_split_path():
    """The scratch of the split shapes holds the per-chunk f64 partials (3 chunks);
    that of the 512-pair batches below, whose launches fill the chip unsplit, does not."""
    f = _lib.load().pcr_cpd_scratch_bytes
    # state, inv, Pt1, P1, PX, row moments, one f64 a target, rounding of the ten regions
    plain = lambda P, M, N: P * (256 + 56 * M + 16 * N) + 10 * 256
    assert f(1, 1100, 300) >= plain(1, 1100, 300) - 10 * 256 + 8 * 3 * 300          # column partials
    assert f(1, 300, 1100) >= plain(1, 300, 1100) - 10 * 256 + 8 * 3 * 300 * 5      # row partials
    assert 8 * 3 * 300 > 10 * 256
    assert f(512, CHUNK + 1, 3) <= plain(512, CHUNK + 1, 3) and f(512, 3, CHUNK + 1) <= plain(512, 3, CHUNK + 1)


@pytest.mark.parametrize("M,N", [(CHUNK + 1, 3), (3, CHUNK + 1)])
def test_estep_unsplit_sweep_over_two_chunks(M, N):
    """512 pairs: enough workgroups without a split, so one workgroup walks both chunks."""
    pairs = [make_pair(M, N, 1e-2, 4000 + p, False) for p in range(512)]
    got = gpu_estep(np.stack([a for a, _ in pairs]), np.stack([b for _, b in pairs]), None, None, 1e-2, 0.1)
    for p in range(0, 512, 37):
        check_estep([g[p] for g in got], *pairs[p], 1e-2, 0.1, f"(512,{M},{N}) p{p}")


def ragged_batch(sigma2):
    counts = [(257, 200), (70, 513), (33, 1)]
    Mmax, Nmax = 300, 520
    src = np.full((3, Mmax, 3), np.nan, F32)
    tgt = np.full((3, Nmax, 3), np.nan, F32)
    pairs = []
    for p, (m, n) in enumerate(counts):
        Y, X = make_pair(m, n, sigma2, 77 + p, False)
        src[p, :m], tgt[p, :n] = Y, X
        pairs.append((Y, X))
    return src, tgt, [c[0] for c in counts], [c[1] for c in counts], pairs


@pytest.mark.parametrize("w", [0.0, 0.1])
def test_estep_ragged_batch_never_reads_padding(w):
    src, tgt, ns, nt, pairs = ragged_batch(1e-2)
    got = gpu_estep(src, tgt, ns, nt, 1e-2, w)
    for p, (Y, X) in enumerate(pairs):
        m, n = ns[p], nt[p]
        check_estep([got[0][p, :n], got[1][p, :m], got[2][p, :m], got[3][p]], Y, X, 1e-2, w, f"ragged w={w} p{p}")
        assert not got[0][p, n:].any() and not got[1][p, m:].any() and not got[2][p, m:].any()
    assert all(np.isfinite(g).all() for g in got)


def test_estep_without_transform_and_numpy_inputs():
    Y, X = make_pair(64, 65, 1e-2, 5, False)
    ys = cr.apply_T(T_PROBE, Y)
    a = cpd.expectation_step(ys, X, 1e-2, 0.1)
    assert [type(v) for v in a] == [np.ndarray, np.ndarray, np.ndarray, float]
    assert a[0].shape == (65,) and a[1].shape == (64,) and a[2].shape == (64, 3) and a[0].dtype == F32
    b = gpu_estep(Y[None], X[None], None, None, 1e-2, 0.1)
    for u, v in zip(a[:3], b[:3]):
        assert u.tobytes() == v[0].tobytes()      # the transform applied in the sweep is apply_T
    assert a[3] == float(b[3][0])


@pytest.mark.parametrize("shape", ["ragged", (1, 1100, 300), (1, 300, 1100)])
def test_estep_is_deterministic(shape):
    if shape == "ragged":
        src, tgt, ns, nt, _ = ragged_batch(1e-2)
    else:
        Y, X = make_pair(shape[1], shape[2], 1e-2, 9, False)
        src, tgt, ns, nt = Y[None], X[None], None, None
    a, b = gpu_estep(src, tgt, ns, nt, 1e-2, 0.1), gpu_estep(src, tgt, ns, nt, 1e-2, 0.1)
    assert all(u.tobytes() == v.tobytes() for u, v in zip(a, b))


# ---------------------------------------------------------------- the loop
def loop_pairs():
    """(65, 130): the stop-rule pair; (257, 200): every target moved and noised once,
    57 of them twice, so that no target is left without a source as sigma2 falls."""
    rng = np.random.default_rng(11)
    X = rng.random((200, 3))
    idx = np.concatenate([rng.permutation(200), rng.integers(0, 200, 57)])
    Y = (X[idx] - np.array([0.05, -0.1, 0.1])) @ cr.rot_z(0.3) + rng.normal(0, 0.01, (257, 3))
    return [cr.stop_rule_pair(), (Y.astype(F32), X.astype(F32))]


@functools.lru_cache(maxsize=None)
def restated(pair, kind, w, maxiter, tol, f32):
    Y, X = loop_pairs()[pair]
    return cr.register(Y, X, kind, w=w, maxiter=maxiter, tol=tol, estep_fn=cr.estep_f32 if f32 else cr.estep)


def pack(pairs):
    Mmax, Nmax = max(len(a) for a, _ in pairs), max(len(b) for _, b in pairs)
    src = np.full((len(pairs), Mmax, 3), np.nan, F32)
    tgt = np.full((len(pairs), Nmax, 3), np.nan, F32)
    for p, (a, b) in enumerate(pairs):
        src[p, :len(a)], tgt[p, :len(b)] = a, b
    return dev(src), dev(tgt), dev(np.array([len(a) for a, _ in pairs], np.int32)), \
        dev(np.array([len(b) for _, b in pairs], np.int32))


def gpu_register(pairs, kind, **kw):
    src, tgt, ns, nt = pack(pairs)
    r = cpd.register_batch(src, tgt, ns, nt, kind=kind, **kw)
    torch.cuda.synchronize()
    return {k: getattr(r, k).cpu().numpy() for k in ("transformation", "scale", "sigma2", "q", "iters", "status")}


def check_loop(got, p, a64, a32, what):
    devs = dict(T=np.abs(a32["T"] - a64["T"]).max(), sigma2=abs(a32["sigma2"] - a64["sigma2"]) / a64["sigma2"],
                q=abs(a32["q"] - a64["q"]) / max(1.0, abs(a64["q"])))
    errs = dict(T=np.abs(got["transformation"][p] - a64["T"]).max(),
                sigma2=abs(got["sigma2"][p] - a64["sigma2"]) / a64["sigma2"],
                q=abs(got["q"][p] - a64["q"]) / max(1.0, abs(a64["q"])))
    for k in ("T", "sigma2", "q"):
        tol = max(4 * devs[k], FLOOR_L)
        print(f"{what} {k}: kernel {errs[k]:.3e}  f32-driven restatement {devs[k]:.3e}  tol {tol:.3e}")
        assert errs[k] <= tol, (what, k, errs[k], devs[k])
    assert abs(got["scale"][p] - a64["scale"]) <= max(4 * abs(a32["scale"] - a64["scale"]), FLOOR_L)


@pytest.mark.parametrize("w", [0.0, 0.1])
@pytest.mark.parametrize("maxiter", [5, 30])
@pytest.mark.parametrize("kind", [cr.RIGID, cr.RIGID_SCALE, cr.AFFINE])
def test_fixed_iterations_match_restatement(kind, maxiter, w):
    got = gpu_register(loop_pairs(), kind, w=w, maxiter=maxiter, tol=0.0)
    assert (got["status"] == 0).all() and (got["iters"] == maxiter).all()
    for p in range(2):
        a64, a32 = restated(p, kind, w, maxiter, 0.0, False), restated(p, kind, w, maxiter, 0.0, True)
        if w == 0.0:    # the FLT_EPSILON rule is discontinuous there: stay clear of it
            assert min(a64["min_colmax"]) > -80 and min(a32["min_colmax"]) > -80
        check_loop(got, p, a64, a32, f"kind={kind} it={maxiter} w={w} p{p}")
        assert np.array_equal(got["transformation"][p][3], [0, 0, 0, 1])
        assert kind == cr.RIGID_SCALE or got["scale"][p] == 1.0


def outlier_pair():
    """200 matched points (noise 0.002) and 5 outlier targets 4 away on every axis:
    no source reaches them from the second iteration on."""
    rng = np.random.default_rng(0)
    X = rng.random((200, 3))
    Y = (X - np.array([0.05, -0.1, 0.1])) @ cr.rot_z(0.3) + rng.normal(0, 0.002, (200, 3))
    return Y.astype(F32), np.concatenate([X, X[:5] + 4.0]).astype(F32)


@pytest.mark.parametrize("kind", [cr.RIGID, cr.RIGID_SCALE, cr.AFFINE])
def test_outlier_targets_follow_the_eps_rule(kind):
    """w = 0.1 with targets no source reaches: their Pt1 = eps / (eps + c) enters
    trXPX (and pulls sigma2 up once c falls towards eps), in the loop as in the
    restatement.  The FLT_EPSILON rule is discontinuous, so the inputs keep every
    column's largest argument above -80 or below -120 at every iteration."""
    Y, X = outlier_pair()
    a64 = cr.register(Y, X, kind, w=0.1, maxiter=30, tol=0.0)
    a32 = cr.register(Y, X, kind, w=0.1, maxiter=30, tol=0.0, estep_fn=cr.estep_f32)
    for a in (a64, a32):
        cm = np.array(a["colmax"])
        assert ((cm > -80) | (cm < -120)).all()
        assert (cm[1:, 200:] < -120).all() and (cm[:, :200] > -80).all()
    # the rule matters here: without the unreached targets' Pt1 the loop ends elsewhere
    drop = lambda ys, X_, s2, w: (lambda r: (np.where(cr.column_max_args(ys, X_, s2) < -120, 0.0, r[0]),) + r[1:])(
        cr.estep(ys, X_, s2, w))
    other = cr.register(Y, X, kind, w=0.1, maxiter=30, tol=0.0, estep_fn=drop)
    gap = abs(other["sigma2"] - a64["sigma2"]) / a64["sigma2"]
    assert gap > 32 * FLOOR_L and (kind != cr.RIGID or gap > 0.5)
    got = gpu_register([(Y, X)], kind, w=0.1, maxiter=30, tol=0.0)
    assert got["status"][0] == 0 and got["iters"][0] == 30
    check_loop(got, 0, a64, a32, f"outliers kind={kind}")


@pytest.mark.parametrize("w", [0.0, 0.1])
@pytest.mark.parametrize("kind", [cr.RIGID, cr.RIGID_SCALE])
def test_stop_rule_stops_at_the_restatements_iteration(kind, w):
    a64, a32 = restated(0, kind, w, 60, 0.1, False), restated(0, kind, w, 60, 0.1, True)
    assert a64["iters"] == a32["iters"] < 60
    qd = np.abs(np.array(a64["qs"]) - np.array(a32["qs"])).max()
    margin = np.abs(np.abs(np.diff(a64["qs"])) - 0.1).min()
    assert margin >= 8 * qd                       # every |dq| is unambiguous
    assert w > 0 or min(a64["min_colmax"]) > -80
    got = gpu_register(loop_pairs()[:1], kind, w=w, maxiter=60, tol=0.1)
    print(f"kind={kind} w={w}: iters {got['iters'][0]} (restatement {a64['iters']}), q diff {qd:.2e}, margin {margin:.2e}")
    assert got["iters"][0] == a64["iters"] and got["status"][0] == 0
    check_loop(got, 0, a64, a32, f"stop kind={kind} w={w}")


def test_stopped_pairs_are_frozen_in_a_batch():
    """Three pairs that stop at iterations 37, 34 and 48: each one's outputs in
    the batch are the bytes of its run alone."""
    a, b, c = cr.stop_rule_pair(3, 0.5), cr.stop_rule_pair(6, 0.2), cr.stop_rule_pair(7, 0.6)
    pairs = [a, (b[0][:50], b[1]), c]
    batch = gpu_register(pairs, cr.RIGID_SCALE, w=0.1, maxiter=60, tol=0.1)
    assert len(set(batch["iters"].tolist())) == 3 and (batch["iters"] < 60).all()
    for p, pr in enumerate(pairs):
        want = cr.register(pr[0], pr[1], cr.RIGID_SCALE, w=0.1, maxiter=60, tol=0.1)
        assert batch["iters"][p] == want["iters"]
        alone = gpu_register([pr], cr.RIGID_SCALE, w=0.1, maxiter=60, tol=0.1)
        for k in batch:
            assert batch[k][p].tobytes() == alone[k][0].tobytes(), (p, k)


def test_initial_transform_is_kept():
    """A pair rotated by 2.5 rad, started from its ground truth, stays there."""
    rng = np.random.default_rng(8)
    X = rng.random((130, 3))
    R, t = cr.rot_z(2.5), np.array([0.3, -0.2, 0.1])
    Y = ((X - t) @ R + rng.normal(0, 0.002, (130, 3))).astype(F32)      # x = R y + t
    X = X.astype(F32)
    T0 = np.eye(4)
    T0[:3, :3], T0[:3, 3] = R, t
    got = gpu_register([(Y, X)], cr.RIGID, w=0.0, maxiter=30, tol=0.0, init=T0)
    assert np.abs(got["transformation"][0] - T0).max() < 5e-3
    a64 = cr.register(Y, X, cr.RIGID, w=0.0, maxiter=30, tol=0.0, init=T0)
    a32 = cr.register(Y, X, cr.RIGID, w=0.0, maxiter=30, tol=0.0, init=T0, estep_fn=cr.estep_f32)
    assert min(a64["min_colmax"]) > -80
    check_loop(got, 0, a64, a32, "init")
    # maxiter = 0 returns init and the initial sigma2
    zero = gpu_register([(Y, X)], cr.RIGID, maxiter=0, init=T0)
    assert np.array_equal(zero["transformation"][0], T0) and zero["iters"][0] == 0
    assert zero["sigma2"][0] == pytest.approx(cr.initial_sigma2(Y, X), rel=1e-12)


def test_empty_cloud_gives_status_1():
    y, x = cr.stop_rule_pair()
    src, tgt, ns, nt = pack([(y, x), (y, x), (y, x)])
    ns[1], nt[2] = 0, 0
    r = cpd.register_batch(src, tgt, ns, nt, kind="rigid", maxiter=5, tol=0.0)
    torch.cuda.synchronize()
    assert r.status.tolist() == [0, 1, 1] and r.iters.tolist() == [5, 0, 0]
    for p in (1, 2):        # the other outputs are left as the module initialised them
        assert torch.equal(r.transformation[p].cpu(), torch.eye(4, dtype=torch.float64)) and float(r.sigma2[p]) == 0.0
    alone = gpu_register([(y, x)], cr.RIGID, maxiter=5, tol=0.0)
    assert r.transformation[0].cpu().numpy().tobytes() == alone["transformation"][0].tobytes()


def test_graph_replay_equals_eager():
    src, tgt, ns, nt = pack(loop_pairs())
    run = lambda: cpd.register_batch(src, tgt, ns, nt, kind="rigid_scale", w=0.1, maxiter=12, tol=0.1)
    eager = run()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        captured = run()
    g.replay()
    torch.cuda.synchronize()
    for k in ("transformation", "scale", "sigma2", "q", "iters", "status"):
        assert getattr(eager, k).cpu().numpy().tobytes() == getattr(captured, k).cpu().numpy().tobytes(), k
    assert (eager.status == 0).all() and (eager.iters >= 2).all()


def nonrigid_pair():
    rng = np.random.default_rng(12)
    Y = rng.random((129, 3))
    moved = Y + 0.05 * np.sin(3.0 * Y[:, [1, 2, 0]])
    X = np.concatenate([moved, moved[:11] + 0.01])
    return Y.astype(F32), X.astype(F32)


def test_nonrigid_matches_restatement():
    Y, X = nonrigid_pair()
    tf, sigma2, q = cpd.NonRigidCPD(Y).registration(X, w=0.1, maxiter=10, tol=0.0)
    a64 = cr.nonrigid(Y, X, w=0.1, maxiter=10, tol=0.0)
    a32 = cr.nonrigid(Y, X, w=0.1, maxiter=10, tol=0.0, estep_fn=cr.estep_f32)
    moved = lambda r: Y.astype(np.float64) + r["g"] @ r["w"]
    got = Y.astype(np.float64) + tf.g @ tf.w
    figures = [("T(Y)", np.abs(got - moved(a64)).max(), np.abs(moved(a32) - moved(a64)).max()),
               ("sigma2", abs(sigma2 - a64["sigma2"]) / a64["sigma2"], abs(a32["sigma2"] - a64["sigma2"]) / a64["sigma2"]),
               ("q", abs(q - a64["q"]) / max(1.0, abs(a64["q"])), abs(a32["q"] - a64["q"]) / max(1.0, abs(a64["q"])))]
    for name, err, dev32 in figures:
        tol = max(4 * dev32, FLOOR_L)
        print(f"nonrigid {name}: module {err:.3e}  f32-driven restatement {dev32:.3e}  tol {tol:.3e}")
        assert err <= tol, (name, err, dev32)
    assert isinstance(tf.g, np.ndarray) and tf.g.shape == (129, 129) and tf.w.shape == (129, 3)
    out = tf.transform(Y)
    assert isinstance(out, np.ndarray) and out.dtype == F32 and np.abs(out - got).max() < 1e-6


def test_classes_return_the_documented_types():
    y, x = cr.stop_rule_pair()
    tf, sigma2, q = cpd.RigidCPD(y).registration(x, w=0.1, maxiter=5)
    assert isinstance(tf.rot, np.ndarray) and tf.rot.shape == (3, 3) and tf.t.shape == (3,)
    assert isinstance(tf.scale, float) and isinstance(sigma2, float) and isinstance(q, float)
    assert np.allclose(tf.rot @ tf.rot.T, np.eye(3), atol=1e-12)
    moved = tf.transform(y)
    assert isinstance(moved, np.ndarray) and moved.shape == y.shape and moved.dtype == F32
    assert np.allclose(moved, tf.scale * y.astype(np.float64) @ tf.rot.T + tf.t, atol=1e-6)
    noscale, _, _ = cpd.RigidCPD(y, update_scale=False).registration(x, maxiter=3)
    assert noscale.scale == 1.0
    af, _, _ = cpd.AffineCPD(y).registration(x, maxiter=3)
    assert af.b.shape == (3, 3) and af.t.shape == (3,) and af.transform(y).shape == y.shape
    # device tensors stay device tensors
    yd, xd = dev(y), dev(x)
    tfd, s2d, qd = cpd.RigidCPD(yd).registration(xd, w=0.1, maxiter=5)
    assert tfd.rot.is_cuda and tfd.t.is_cuda and isinstance(s2d, float) and isinstance(qd, float)
    md = tfd.transform(yd)
    assert md.is_cuda and md.dtype == torch.float32 and md.shape == yd.shape
    assert np.array_equal(tfd.rot.cpu().numpy(), tf.rot) and s2d == sigma2 and qd == q
    nr, _, _ = cpd.NonRigidCPD(yd).registration(xd, maxiter=2)
    assert nr.g.is_cuda and nr.w.is_cuda and nr.transform(yd).is_cuda
    with pytest.raises(ValueError):
        cpd.RigidCPD(yd).registration(x)      # numpy target for a device source
