"""The TFMR matching contract (include/pcr_api.h, "Similarity top-k matching")
restated on the CPU, and the case generator its tests share.

Contract.  fx (B,N1,C), fy (B,M1,C) f32, normalised and gathered; tgt (B,M1,3).
  S[i][j] = the f32 fmaf chain over c = 0 .. C-1 ascending from +0 -- numpy has no
  fmaf, so tests/cpp/tfmr_chain.cpp is compiled with the host compiler
  (-O2 -ffp-contract=off) and loaded with ctypes; everything after the chain is
  plain numpy f32.  Per row the k largest by (S descending, j ascending), -0
  equal to +0 and reported as +0: val, idx.  Rows ordered by (val[:, 0]
  descending, i ascending): sel = the first n_keep.  Per kept row
  sum = ((v0 + v1) + ...), den = sum + 1e-8f, w_t = v_t / den,
  tgt_corr = ((w0 t0) + w1 t1) + ..., every operation rounded to f32.

Cases.  Raw features are integers in [-64, 64] (16 x a standard normal, rounded
and clipped), so a row's sum of squares is an integer below 2^24: exact in f32
in any summation order, which makes the normalisation f / (|f| + 1e-8)
reproducible bit for bit by torch and numpy alike, whatever their reduction
order.  Half of the targets are copies of sources plus noise on a ramp
0.05 .. 1.5 (in units of the rows' sigma).  The overlap scores are permutations
of distinct values: the reference's unstable sort has one answer.  Inputs are
regenerated from the seed, never stored.
"""
import atexit
import ctypes
import functools
import os
import shutil
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
F32 = np.float32

# chosen among 1 .. 8 (3, 7 and 8 qualify) as one for which the restatement equals the reference on every
# stored array (make_golden_tfmr.py --seed S probes another)
GOLDEN_SEED = 3
# name -> (B, N1, M1, C, k, top_prob): the golden cases (tests/golden/make_golden_tfmr.py)
GOLDEN_CASES = {
    "ropnet_k1_p4": (2, 896, 1434, 960, 1, 0.4),
    "ropnet_k1_p6": (2, 896, 1434, 960, 1, 0.6),
    "ropnet_k3_p4": (2, 896, 1434, 960, 3, 0.4),
    "ropnet_k3_p6": (2, 896, 1434, 960, 3, 0.6),
    "mid_k3": (2, 129, 131, 191, 3, 0.6),
    "small_k3": (1, 33, 35, 960, 3, 0.6),
}


@functools.lru_cache(maxsize=None)
def _chain_lib():
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        raise RuntimeError("no host C++ compiler for tests/cpp/tfmr_chain.cpp")
    d = tempfile.mkdtemp(prefix="tfmr_chain_")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    so = os.path.join(d, "libtfmr_chain.so")
    base = [cxx, "-O2", "-ffp-contract=off", "-shared", "-fPIC", os.path.join(HERE, "cpp", "tfmr_chain.cpp"),
            "-o", so, "-lm"]
    # -march=native inlines fmaf where the host has the instruction (same
    # result, much faster); without it libm's fmaf is called
    if subprocess.run(base + ["-march=native"], capture_output=True).returncode != 0:
        subprocess.run(base, check=True)
    lib = ctypes.CDLL(so)
    lib.tfmr_chain.restype = None
    lib.tfmr_chain.argtypes = [ctypes.c_void_p] * 2 + [ctypes.c_int64] * 3 + [ctypes.c_void_p]
    return lib


def chain(fx, fy):
    """S (B,N1,M1): the contract's fmaf chain."""
    fx, fy = np.ascontiguousarray(fx, F32), np.ascontiguousarray(fy, F32)
    B, N1, C = fx.shape
    M1 = fy.shape[1]
    out = np.empty((B, N1, M1), F32)
    for b in range(B):
        _chain_lib().tfmr_chain(fx[b].ctypes.data, fy[b].ctypes.data, N1, M1, C, out[b].ctypes.data)
    return out


def topk(S, k):
    """val (B,N1,k) f32, idx (B,N1,k) int64 by (S descending, j ascending)."""
    S = S + F32(0.0)                                   # -0 -> +0
    idx = np.argsort(-S, axis=-1, kind="stable")[..., :k]
    return np.take_along_axis(S, idx, -1), idx


def select(val, n_keep):
    """sel (B,n_keep) int64: rows by (val[:, 0] descending, i ascending)."""
    return np.argsort(-val[..., 0], axis=-1, kind="stable")[:, :n_keep]


def weights(val, idx, tgt, sel):
    """w (B,n_keep,k), tgt_corr (B,n_keep,3), idx_keep of the kept rows."""
    B, k = val.shape[0], val.shape[2]
    bi = np.arange(B)[:, None]
    v, j = val[bi, sel].astype(F32), idx[bi, sel]
    s = v[..., 0].copy()
    for t in range(1, k):
        s = (s + v[..., t]).astype(F32)
    den = (s + F32(1e-8)).astype(F32)
    with np.errstate(all="ignore"):
        w = (v / den[..., None]).astype(F32)
    t = np.asarray(tgt, F32)[bi[:, :, None], j]              # (B,n_keep,k,3)
    corr = (w[..., 0, None] * t[..., 0, :]).astype(F32)
    for q in range(1, k):
        corr = (corr + (w[..., q, None] * t[..., q, :]).astype(F32)).astype(F32)
    return w, corr, j


def restate(fx, fy, tgt, k, n_keep, S=None):
    """Every output of the two entries for one call."""
    S = chain(fx, fy) if S is None else S
    val, idx = topk(S, k)
    sel = select(val, n_keep)
    w, corr, idx_keep = weights(val, idx, tgt, sel)
    return dict(val=val, idx=idx, sel=sel, w=w, tgt_corr=corr, idx_keep=idx_keep)


def make_case(B, N1, M1, C, seed):
    """Raw inputs of TFMRModule.forward's matching: the attention outputs (already
    (B,N,C)), the clouds and the overlap scores, N = N1 and M = M1."""
    rng = np.random.default_rng(seed)
    gx = rng.standard_normal((B, N1, C))
    gy = rng.standard_normal((B, M1, C))
    half = M1 // 2
    ramp = np.linspace(0.05, 1.5, max(half, 1))[:half]
    for j in range(half):
        gy[:, j] = gx[:, j % N1] + ramp[j] * rng.standard_normal((B, C))
    quant = lambda g: np.clip(np.rint(16.0 * g), -64, 64).astype(F32)  # noqa: E731
    perm = lambda n: np.stack([rng.permutation(n) for _ in range(B)])   # noqa: E731
    return dict(
        f_x_attn=quant(gx), f_y_attn=quant(gy),
        src=rng.uniform(-1, 1, (B, N1, 3)).astype(F32), tgt=rng.uniform(-1, 1, (B, M1, 3)).astype(F32),
        x_ol_score=(0.05 + 0.9 * (perm(N1) + 0.5) / N1).astype(F32),
        y_ol_score=(0.05 + 0.9 * (perm(M1) + 0.5) / M1).astype(F32))


def golden_case(name):
    B, N1, M1, C, k, p = GOLDEN_CASES[name]
    return make_case(B, N1, M1, C, (GOLDEN_SEED, N1, C))


def normalise(f):
    """f / (|f| + 1e-8) as TFMR.py:195 forms it; exact for make_case's integer rows."""
    f = np.asarray(f, F32)
    ss = (f.astype(np.float64) ** 2).sum(-1, keepdims=True)
    assert ss.max() < 2 ** 24 and (ss == np.rint(ss)).all()
    return (f / (np.sqrt(ss.astype(F32)) + F32(1e-8)).astype(F32)).astype(F32)


def prepare(case, N1=None, M1=None):
    """TFMR.py:195-200 and 214-219: normalise, sort the overlap scores descending
    (stable) and gather.  Returns fx, fy, src, tgt, x_ol (all gathered)."""
    B = case["src"].shape[0]
    N1 = case["src"].shape[1] if N1 is None else N1
    M1 = case["tgt"].shape[1] if M1 is None else M1
    bi = np.arange(B)[:, None]
    xi = np.argsort(-case["x_ol_score"], axis=-1, kind="stable")
    yi = np.argsort(-case["y_ol_score"], axis=-1, kind="stable")[:, :M1]
    x_ol = np.take_along_axis(case["x_ol_score"], xi, -1)   # the reference keeps all N sorted scores
    xi = xi[:, :N1]
    return (normalise(case["f_x_attn"])[bi, xi], normalise(case["f_y_attn"])[bi, yi],
            case["src"][bi, xi], case["tgt"][bi, yi], x_ol)


@functools.lru_cache(maxsize=None)
def golden_similarity(shape_key):
    """(prepared tensors, S) of a golden shape, computed once per process: the
    similarity does not depend on (k, top_prob)."""
    name = next(n for n, c in GOLDEN_CASES.items() if c[:4] == shape_key)
    prep = prepare(golden_case(name))
    return prep, chain(prep[0], prep[1])
