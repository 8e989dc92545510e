"""CPU: the f64 restatements of the two attention contracts
(tests/attention_ref.py) agree, within their own derived bounds, with what the
reference's multi_head_attention and OverlapAttentionBlock.forward returned
(tests/golden/attention_golden.npz).  That is what lets the GPU tests stand on
the restatement.  Also: the bound has teeth (a dropped key misses it by orders
of magnitude), its conditions hold for the chosen cases, and the entry points
are declared, exported and bound and refuse bad arguments before any device
work."""
import ctypes
import os
import re
import shlex
import subprocess

import numpy as np
import pytest

import attention_cases as ac
import attention_ref as ar
from pointcloudregistration_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH = os.path.join(ROOT, "tests", "golden", "attention_golden.npz")
G = np.load(PATH)
ENTRIES = {"pcr_attention_forward": 25, "pcr_offset_attention_forward": 20}
SIZERS = {"pcr_attention_scratch_bytes": 6, "pcr_offset_attention_scratch_bytes": 4}


def _ratio(ref, want, bound):
    return float((np.abs(ref.astype(np.float64) - want) / bound).max())


def test_fixture_covers_the_cases():
    want = {f"mha/{c}" for c in ac.MHA_CASES} | {"overlap/src", "overlap/tgt"} | \
        {f"offset/{c}/{k}" for c in ac.OFFSET_CASES for k in ("ol", "none")}
    assert set(G.files) == want
    assert all(G[k].dtype == np.float32 for k in G.files)
    assert os.path.getsize(PATH) < 96 * 1024


@pytest.mark.parametrize("name", sorted(ac.MHA_CASES))
def test_multi_head_restatement_agrees_with_reference(name):
    c = ac.make_mha(name)
    want, bound = ar.multi_head(c["query"], c["key"], c["value"])
    ref = G[f"mha/{name}"]
    assert ref.shape == want.shape
    assert _ratio(ref, want, bound) <= 1.0
    # teeth: without the last of the M keys (a weight of order 1 / M) nearly every output misses the
    # bound by more than a factor of ten
    wrong, _ = ar.multi_head(c["query"], c["key"][..., :-1], c["value"][..., :-1])
    assert (np.abs(wrong - want) > 10 * bound).mean() > 0.9


def test_overlap_restatement_agrees_with_reference():
    c = ac.make_overlap()
    n1 = c["len_src"]
    want, bound = ar.overlap_scores(c["feats_norm"], c["attn_scores"], n1, c["temperature"])
    ref = np.concatenate([G["overlap/src"], G["overlap/tgt"]])[:, None]
    assert ref.shape == want.shape == (n1 + ac.OVERLAP_CASE["n2"], 1)
    assert _ratio(ref, want, bound) <= 1.0
    # the stated properties: unit rows, a scale of about 27, a softmax that is neither flat nor one-hot
    f = c["feats_norm"].astype(np.float64)
    assert np.abs(np.linalg.norm(f, axis=1) - 1).max() < 1e-6
    assert 25 < 1 / c["temperature"] < 29
    _, _, p, _ = ar.attention(f[:n1].T, f[n1:].T, c["attn_scores"][n1:].T, 1 / c["temperature"])
    assert 0.05 < np.median(p.max(1)) < 0.999


@pytest.mark.parametrize("key", [f"{c}/{k}" for c in sorted(ac.OFFSET_CASES) for k in ("ol", "none")])
def test_offset_restatement_agrees_with_reference(key):
    name, which = key.split("/")
    c = ac.make_offset(name)
    q, v = ac.offset_qkv(c)
    # the selections are exact: the block's convolutions return these very tensors
    assert np.array_equal(q.astype(np.float64), np.einsum("oc,bcn->bon", c["w_qk"].astype(np.float64), c["x"]))
    assert np.array_equal(v.astype(np.float64), np.einsum("oc,bcn->bon", c["w_v"].astype(np.float64), c["x"]))
    ol = c["ol"] if which == "ol" else None
    want, bound = ar.offset_batched(q, q, v, ol)
    # the block returned x + (x - x_r): x_r = 2 x - output, to one ulp of |2 x|
    x_r = 2.0 * c["x"].astype(np.float64) - G[f"offset/{key}"].astype(np.float64)
    ulp = np.spacing(np.abs(2.0 * c["x"]).astype(np.float32)).astype(np.float64)
    assert _ratio(x_r, want, bound + ulp) <= 1.0
    assert (c["ol"][:, 3] == 0).all()
    if which == "ol":   # the zero-overlap row attends uniformly
        _, _, p = ar.offset_attention(q[0], q[0], v[0], c["ol"][0])
        assert np.allclose(p[3], 1.0 / p.shape[1], rtol=1e-12)


def test_bound_constants_follow_the_tiling():
    # K = 43 + 4 T with T = ceil(m / 32) tiles (attention_ref's docstring counts them from the kernel)
    assert [ar.k_attention(m) for m in (1, 32, 33, 130, 4096)] == [47, 47, 51, 63, 555]
    src = open(os.path.join(ROOT, "pointcloudregistration_amd", "csrc", "attention.hip")).read()
    assert re.search(r"constexpr int kRegTile = %d;" % ar.TILE, src)
    assert re.search(r"constexpr int kMaxSplit = 16;", src)


def test_entry_points_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "pcr_api.h")).read()
    lib = _lib.load()

    def arity(name, ret):
        m = re.search(r"\b%s\s+%s\s*\(([^;]*)\);" % (ret, name), hdr)
        assert m, name
        return len(m.group(1).split(","))

    for s, n in ENTRIES.items():
        assert s in _lib.exported_symbols() and s in _lib.SIGNATURES and hasattr(lib, s)
        assert arity(s, "int") == n == len(_lib.SIGNATURES[s])
    for s, n in SIZERS.items():
        assert s in _lib.exported_symbols() and hasattr(lib, s)
        assert arity(s, "int64_t") == n == len(getattr(lib, s).argtypes)
    import pointcloudregistration_amd as pcr
    assert "attention" in pcr.__all__
    from pointcloudregistration_amd import attention
    for name in ("multi_head_attention", "overlap_scores", "offset_attention", "CrossAttention",
                 "OverlapAttentionBlock", "fuse"):
        assert hasattr(attention, name) and name in attention.__all__
    assert pcr.attention is attention


def _err(lib):
    return lib.pcr_last_error().decode()


def test_argument_errors_without_gpu():
    lib = _lib.load()
    one = ctypes.c_void_p(256)   # non-null: never dereferenced, validation comes first

    def att(q=one, k=one, v=one, out=one, b=1, h=1, n=8, m=8, d=4, dv=4, scratch=one):
        return lib.pcr_attention_forward(q, 0, 0, 8, k, 0, 0, 8, v, 0, 0, 8, out, 0, 0, 8, b, h, n, m, d, dv, 1.0,
                                         scratch, None)

    def off(q=one, k=one, v=one, r=None, out=one, b=1, n=8, d=4, dv=4, scratch=one):
        return lib.pcr_offset_attention_forward(q, 0, 8, k, 0, 8, v, 0, 8, r, 0, out, 0, 8, b, n, d, dv, scratch,
                                                None)

    for name in ("q", "k", "v", "out"):
        assert att(**{name: None}) == -1 and "attention_forward: null pointer" in _err(lib), name
        assert off(**{name: None}) == -1 and "offset_attention_forward: null pointer" in _err(lib), name
    assert off(scratch=None) == -1 and "null scratch" in _err(lib)
    for fn in (att, off):
        for kw, msg in ((dict(d=0), "d=0 outside 1..256"), (dict(d=257), "d=257 outside 1..256"),
                        (dict(dv=0), "dv=0 outside 1..256"), (dict(dv=257), "dv=257 outside 1..256"),
                        (dict(n=-1), "n=-1"), (dict(n=(1 << 24) + 1), "n=16777217"), (dict(b=-1), "b=-1")):
            assert fn(**kw) == -1 and msg in _err(lib), (fn.__name__, kw)
    assert att(m=0) == -1 and "m=0 outside 1.." in _err(lib)
    assert att(m=(1 << 24) + 1) == -1 and "m=16777217" in _err(lib)
    assert att(h=0) == -1 and "h=0" in _err(lib)
    # a split call needs its scratch; an unsplit one takes a null
    assert lib.pcr_attention_scratch_bytes(1, 1, 128, 4096, 64, 64) > 0
    assert att(n=128, m=4096, d=64, dv=64, scratch=None) == -1 and "null scratch" in _err(lib)
    # empty calls: no launch, no pointer needed
    assert att(n=0, q=None, k=None, v=None, out=None, scratch=None) == 0
    assert att(b=0, q=None, k=None, v=None, out=None, scratch=None) == 0
    assert off(n=0, q=None, k=None, v=None, out=None, scratch=None) == 0
    assert off(b=0, q=None, k=None, v=None, out=None, scratch=None) == 0


def test_scratch_sizes():
    lib = _lib.load()
    # the offset form: the rows' maxima and sums, 8 b n bytes (rounded up to 256)
    assert lib.pcr_offset_attention_scratch_bytes(3, 1000, 48, 192) == 24064
    assert lib.pcr_offset_attention_scratch_bytes(2, 1024, 48, 192) == 8 * 2 * 1024
    # attention: nothing unless the keys are split (small grid and at least 8 key tiles) ...
    assert lib.pcr_attention_scratch_bytes(1, 4, 4096, 4096, 64, 64) == 0     # 128 workgroups
    assert lib.pcr_attention_scratch_bytes(1, 1, 100, 224, 64, 64) == 0       # 7 tiles
    assert lib.pcr_attention_scratch_bytes(0, 4, 100, 300, 64, 64) == 0
    # ... then splits * b * h * (dv + 2) * n floats, whole tiles per split, at most 16 splits
    assert lib.pcr_attention_scratch_bytes(1, 4, 256, 256, 64, 64) == 2 * 4 * 66 * 256 * 4      # 8 tiles: 2 runs of 4
    assert lib.pcr_attention_scratch_bytes(1, 1, 1000, 3000, 256, 1) == 16 * 3 * 1000 * 4      # 94 tiles: 16 runs of 6
    assert lib.pcr_attention_scratch_bytes(1, 1, 8, 8, 0, 4) == -1 and "d=0" in _err(lib)
    assert lib.pcr_offset_attention_scratch_bytes(1, 8, 4, 300) == -1 and "dv=300" in _err(lib)


def test_kernels_compile_without_spills(tmp_path):
    """The staging loops rely on the compiler not hoisting their lane masks (attention.hip: the opaque
    copies of d and dv).  Compile the unit as the Makefile does, with the resource remarks on: every
    kernel must report no spilled VGPR or SGPR and no scratch, whatever the compiler version."""
    csrc = os.path.join(ROOT, "pointcloudregistration_amd", "csrc")
    plan = subprocess.run(["make", "-C", csrc, "-n", "-B", "build/attention.hip.o"], capture_output=True,
                          text=True, check=True).stdout
    cmd = [ln for ln in plan.splitlines() if "attention.hip" in ln and " -c " in ln]
    assert len(cmd) == 1, plan
    argv = shlex.split(cmd[0])
    argv[argv.index("-o") + 1] = str(tmp_path / "attention.o")
    run = subprocess.run(argv + ["-Rpass-analysis=kernel-resource-usage"], cwd=csrc, capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    remarks = run.stderr
    kernels = re.findall(r"Function Name: (\S+)", remarks)
    assert len(kernels) == 17 and sum("attn_combine" in k for k in kernels) == 1, kernels
    for field in ("SGPRs Spill", "VGPRs Spill", r"ScratchSize \[bytes/lane\]"):
        values = re.findall(field + r": (\d+)", remarks)
        assert len(values) == len(kernels) and set(values) == {"0"}, (field, values)
