"""Seeded inputs of the attention tests.  Only the reference's outputs are stored
(attention_golden.npz); the inputs are rebuilt from these generators by
make_golden_attention.py and by the tests.

Multi-head cases are (B, dim, nhead, N, M, dv): standard-normal query, key and
value, so the scaled scores have unit variance.  The overlap-score case has
unit-norm rows of C = 256 channels pulled towards a few shared directions (so
that with the temperature's scale of about 27 the softmax is neither flat nor
one-hot) and attention scores in (0, 1).  The offset cases are (B, C, N) inputs
of an OverlapAttentionBlock whose 1x1 convolutions are signed, power-of-two
scaled channel selections: their f32 outputs are exact, so the restatement can
be given the very tensors the reference's bmm saw.
"""
import numpy as np

SEED = 20241020

# name -> (B, dim, nhead, N, M, dv)
MHA_CASES = {
    "heads": (2, 8, 4, 33, 17, 8),      # batch, four interleaved heads, N past a tile, M below one
    "ngenet": (1, 64, 4, 20, 70, 64),   # NgeNet's 64 channels per head; three key tiles
}
# unit rows, C channels, n1 source and n2 target rows, NgeNet's temperature at initialisation
OVERLAP_CASE = dict(C=256, n1=40, n2=70, temperature=float(np.exp(np.float32(-5.0)) + 0.03))
# name -> (B, C, N); d = C // 4
OFFSET_CASES = {
    "block": (2, 32, 45),
}
_POW2 = np.array([1.0, -1.0, 0.5, 2.0], np.float32)


def _rng(kind, name):
    names = sorted(MHA_CASES) + ["overlap"] + sorted(OFFSET_CASES)
    return np.random.default_rng((SEED, names.index(name), len(kind)))


def random_mha(rng, B, d, h, N, M, dv):
    """(query (B,d,h,N), key (B,d,h,M), value (B,dv,h,M)) f32, standard normal."""
    return (rng.standard_normal((B, d, h, N)).astype(np.float32),
            rng.standard_normal((B, d, h, M)).astype(np.float32),
            rng.standard_normal((B, dv, h, M)).astype(np.float32))


def make_mha(name):
    q, k, v = random_mha(_rng("mha", name), *MHA_CASES[name])
    return dict(query=q, key=k, value=v)


def unit_rows(rng, n, C, centres=6):
    """(n, C) f32 rows of unit norm clustered around `centres` directions."""
    c = rng.standard_normal((centres, C))
    f = c[rng.integers(0, centres, n)] + 0.8 * rng.standard_normal((n, C))
    f = f / np.linalg.norm(f, axis=1, keepdims=True)
    return f.astype(np.float32)


def make_overlap():
    """-> dict(feats_norm (n,C), attn_scores (n,1), len_src, temperature)."""
    o = OVERLAP_CASE
    rng = _rng("overlap", "overlap")
    n = o["n1"] + o["n2"]
    return dict(feats_norm=unit_rows(rng, n, o["C"]), attn_scores=rng.random((n, 1)).astype(np.float32),
                len_src=o["n1"], temperature=o["temperature"])


def selection(rng, rows, cols):
    """(rows, cols) f32 with one entry of +-1, 0.5 or 2 per row: a 1x1 convolution with it is exact."""
    w = np.zeros((rows, cols), np.float32)
    w[np.arange(rows), rng.permutation(cols)[:rows]] = _POW2[rng.integers(0, 4, rows)]
    return w


def make_offset(name):
    """-> dict(x (B,C,N), w_qk (C//4,C), w_v (C,C), ol (B,N)); the block's q, k, v are
    w_qk x, w_qk x and w_v x (no bias), exactly."""
    B, C, N = OFFSET_CASES[name]
    rng = _rng("offset", name)
    x = rng.standard_normal((B, C, N)).astype(np.float32)
    ol = rng.random((B, N)).astype(np.float32)
    ol[:, 3] = 0.0                                   # a row without overlap: uniform attention
    return dict(x=x, w_qk=selection(rng, C // 4, C), w_v=selection(rng, C, C), ol=ol)


def offset_qkv(c):
    """The block's exact f32 q (= k) and v of a make_offset case."""
    q = np.einsum("oc,bcn->bon", c["w_qk"], c["x"]).astype(np.float32)
    v = np.einsum("oc,bcn->bon", c["w_v"], c["x"]).astype(np.float32)
    return q, v
