"""CPU: the f64 restatement of the KPConv forward / neighbour max-pool contracts
(tests/kpconv_conv_ref.py) agrees with what the reference's own KPConv.forward
and MaxPoolBlock.forward returned (tests/golden/kpconv_conv_golden.npz): the
convolution within the derived bound at every case, the pool byte for byte.
That is what lets the GPU tests stand on the restatement.  Also: the entries
are declared, exported and bound, refuse bad arguments with their messages
before any device work, and empty calls return 0."""
import ctypes
import os
import re

import numpy as np
import pytest

import kpconv_conv_cases as kc
import kpconv_conv_ref as kr
from pointcloudregistration_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, "tests", "golden", "kpconv_conv_golden.npz"))
ENTRIES = ("pcr_kpconv_forward", "pcr_neighbor_max")


def test_fixture_covers_the_cases():
    want = {f"linear/{c}" for c in kc.CASES} | {f"constant/{kc.CONSTANT_CASE}"} | \
        {f"pool/{c}" for c in kc.POOL_CASES}
    assert set(G.files) == want
    assert {c[0] for c in kc.CASES.values()} == {
        (129, 65, 37, 15, 1, 64), (300, 257, 20, 15, 32, 32), (33, 33, 5, 15, 256, 256),
        (70, 40, 40, 15, 128, 128), (64, 300, 38, 7, 24, 40), (33, 1, 3, 16, 8, 8)}
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "kpconv_conv_golden.npz")) < 512 * 1024


@pytest.mark.parametrize("name", sorted(kc.CASES))
def test_inputs_have_the_stated_properties(name):
    c = kc.make(name)
    (n, m, k, K, c_in, c_out), _ = kc.CASES[name]
    assert c["q"].shape == (n, 3) and c["s"].shape == (m, 3) and c["f"].shape == (m, c_in)
    assert c["idx"].shape == (n, k) and c["kp"].shape == (K, 3) and c["W"].shape == (K, c_in, c_out)
    real = c["idx"] < m
    assert (~real).all(1).any(), "no all-pad query"
    assert real.any()
    # pads trail the real columns, as a radius search leaves them
    assert (np.diff(real.astype(np.int8), axis=1) <= 0).all()
    assert m < 8 or not c["f"].any(1).all(), "no exactly-zero row"
    if sorted(kc.CASES).index(name) % 2 == 1 and m > 8:
        assert (c["f"].astype(np.float64).sum(1) < 0).any(), "no negative row sum in a signed case"
    if name == "pads":
        assert 0.85 <= (~real).mean() <= 0.97


@pytest.mark.parametrize("key", sorted(k for k in G.files if not k.startswith("pool/")))
def test_restatement_agrees_with_reference(key):
    infl, name = key.split("/")
    c = kc.make(name)
    want, bound, allpad = kr.kpconv(c["q"], c["s"], c["f"], c["idx"], c["kp"], c["W"], c["extent"], infl)
    ref = G[key]
    assert ref.dtype == np.float32 and ref.shape == want.shape
    err = np.abs(ref.astype(np.float64) - want)
    assert (err <= bound).all(), f"max err / bound = {(err / np.maximum(bound, 1e-300)).max()}"
    assert not ref[allpad].any() and not want[allpad].any()
    # the bound has teeth: the neighbour columns shifted by one support miss it by orders of magnitude
    m = c["s"].shape[0]
    if m > 1:
        off = np.where(c["idx"] < m, (c["idx"] + 1) % m, m)
        wrong = kr.kpconv(c["q"], c["s"], c["f"], off, c["kp"], c["W"], c["extent"], infl)[0]
        assert (np.abs(wrong - want) > 100 * bound).any()


@pytest.mark.parametrize("name", kc.POOL_CASES)
def test_pool_restatement_is_byte_equal(name):
    c = kc.make(name)
    assert kr.neighbor_max(c["f"], c["idx"]).tobytes() == G[f"pool/{name}"].tobytes()
    # every pad value reads the same zero
    m = c["s"].shape[0]
    for pad in (-1, m + 5):
        alt = np.where(c["idx"] == m, pad, c["idx"])
        assert kr.neighbor_max(c["f"], alt).tobytes() == G[f"pool/{name}"].tobytes()


def test_entry_points_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "pcr_api.h")).read()
    lib = _lib.load()
    for s in ENTRIES:
        assert s in _lib.exported_symbols() and s in _lib.SIGNATURES
        assert re.search(r"\bint\s+%s\s*\(" % s, hdr)
        assert hasattr(lib, s)
    assert len(_lib.SIGNATURES["pcr_kpconv_forward"]) == 18
    assert len(_lib.SIGNATURES["pcr_neighbor_max"]) == 9
    from pointcloudregistration_amd import kpconv
    for name in ("kpconv_forward", "neighbor_max", "KPConv", "fuse"):
        assert hasattr(kpconv, name)


def _err(lib):
    return lib.pcr_last_error().decode()


def test_argument_errors_without_gpu():
    lib = _lib.load()
    one = ctypes.c_void_p(256)   # non-null: never dereferenced, validation comes first

    def conv(q=one, s=one, f=one, inds=one, width=8, n=8, m=8, k=4, kp=one, w=one, K=15, c_in=4, c_out=4,
             ext=0.5, infl=0, flags=one, out=one):
        return lib.pcr_kpconv_forward(q, s, f, inds, width, n, m, k, kp, w, K, c_in, c_out, ext, infl, flags,
                                      out, None)

    def pool(f=one, inds=one, width=4, n=8, m=8, k=4, c=4, out=one):
        return lib.pcr_neighbor_max(f, inds, width, n, m, k, c, out, None)

    for name in ("q", "s", "f", "inds", "kp", "w", "flags", "out"):
        assert conv(**{name: None}) == -1 and "kpconv_forward: null pointer" in _err(lib), name
    for name in ("f", "inds", "out"):
        assert pool(**{name: None}) == -1 and "neighbor_max: null pointer" in _err(lib), name
    assert conv(width=2) == -1 and "index width 2" in _err(lib)
    assert pool(width=16) == -1 and "index width 16" in _err(lib)
    assert conv(K=0) == -1 and "K=0 outside 1..16" in _err(lib)
    assert conv(K=17) == -1 and "K=17 outside 1..16" in _err(lib)
    assert conv(k=0) == -1 and "k=0 outside 1..256" in _err(lib)
    assert conv(k=257) == -1 and "k=257 outside 1..256" in _err(lib)
    assert pool(k=257) == -1 and "k=257 outside 1..256" in _err(lib)
    assert conv(c_in=0) == -1 and "c_in=0 outside 1..2048" in _err(lib)
    assert conv(c_in=2049) == -1 and "c_in=2049" in _err(lib)
    assert conv(c_out=0) == -1 and "c_out=0 outside 1..2048" in _err(lib)
    assert conv(c_out=2049) == -1 and "c_out=2049" in _err(lib)
    assert pool(c=0) == -1 and "c=0 outside 1..4096" in _err(lib)
    assert pool(c=4097) == -1 and "c=4097" in _err(lib)
    assert conv(n=-1) == -1 and "n=-1" in _err(lib)
    assert conv(n=(1 << 24) + 1) == -1 and "n=16777217" in _err(lib)
    assert conv(m=0) == -1 and "m=0" in _err(lib)
    assert pool(m=(1 << 24) + 1) == -1 and "m=16777217" in _err(lib)
    assert conv(infl=2) == -1 and "influence=2" in _err(lib)
    assert conv(ext=0.0) == -1 and "KP_extent" in _err(lib)
    assert conv(ext=float("nan")) == -1 and "KP_extent" in _err(lib)
    # empty calls: no launch, no pointer needed
    assert conv(n=0, q=None, s=None, f=None, inds=None, kp=None, w=None, flags=None, out=None) == 0
    assert pool(n=0, f=None, inds=None, out=None) == 0
