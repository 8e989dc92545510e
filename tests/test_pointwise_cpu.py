"""CPU: the f64 restatement of pcr_pointwise_forward (tests/pointwise_ref.py)
against f64 torch (Conv1d, GroupNorm, the activation) at 1e-12 on every kernel
case; the product bound's constants in exact rational arithmetic; the
reference's recorded outputs (tests/golden/ropnet_golden.npz) within the
restatement's bounds; and the conditions under which the tiny network's sorts
are decided (the maker's search, re-checked here from the stored figures)."""
import os
from fractions import Fraction

import numpy as np
import pytest
import torch

import pointwise_cases as pc
import pointwise_ref as pr
import ropnet_blocks as rb

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ropnet_golden.npz"))


def torch_form(d):
    """The case in torch's own layers, f64."""
    t = lambda a: None if a is None else torch.from_numpy(np.asarray(a, np.float64))   # noqa: E731
    row = torch.cat([t(s) if u is None else t(s) - t(u) for s, u in zip(d["sources"], d["subs"])], dim=1)
    y = torch.nn.functional.conv1d(row, t(d["w"])[:, :, None], t(d["bias_v"]))
    if d["cbias_v"] is not None:
        y = y + t(d["cbias_v"])[:, :, None]
    if d["groups"]:
        y = torch.nn.functional.group_norm(y, d["groups"], t(d["gamma"]), t(d["beta"]), pc.EPS)
    if d["act"]:
        y = torch.nn.functional.leaky_relu(y, d["slope"])
    if d["res_v"] is not None:
        y = y + t(d["res_v"])
    return y.numpy()


@pytest.mark.parametrize("name", sorted(pc.KERNEL))
def test_restatement_is_torchs_layers(name):
    d = pc.make_kernel(name)
    gw = d["cout"] // d["groups"] if d["groups"] else 0
    r = pr.pointwise(d["sources"], d["w"], d["subs"], d["bias_v"], d["cbias_v"], gw, d["gamma"], d["beta"], pc.EPS,
                     d["act"], d["slope"], d["res_v"])
    want = torch_form(d)
    assert r["out"].shape == want.shape
    assert np.abs(r["out"] - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
    assert np.array_equal(r["max"], r["out"].max(2))
    assert (r["bound"] >= 0).all() and np.isfinite(r["bound"]).all()


def test_product_constants_in_exact_arithmetic():
    """g_n = n u / (1 - n u) <= (n + 1) u exactly up to n = 4095 and not at 4096 (so layer's (n + 2) u may
    not be used past it), and (1 + u)^n - 1 <= g_n at the widths the CG issues and the reference's 6144."""
    u = Fraction(1, 2 ** 24)
    g = lambda n: n * u / (1 - n * u)   # noqa: E731
    assert g(4095) <= 4096 * u and g(4096) > 4097 * u
    assert pr.N_FIRST_ORDER == 4095
    for n in (3072, 4608, 6144, 8192):
        assert (1 + u) ** n - 1 <= g(n)
        assert float(g(n)) <= pr.gamma_n(n) * (1 + 2.0 ** -50)     # the float the bound uses is not below it
    widths = [sum(k["widths"]) for k in pc.KERNEL.values()]
    assert max(widths) == 4608 and 3072 in widths


def test_case_conditions():
    """What the kernel cases are there for."""
    k = pc.KERNEL
    assert {k[f"n{n}"]["n"] for n in (1, 2, 63, 64, 65, 129)} == {1, 2, 63, 64, 65, 129}
    assert k["n1"]["groups"] and {k["b1"]["b"], k["b3"]["b"]} == {1, 3}
    assert k["seams"]["widths"] == (5, 1, 32) and k["seams"]["sub"] == (False, False, True)
    assert 5 % 2 == 1 and (5 + 1) % 2 == 0 and sum(k["cin3"]["widths"]) % 2 == 1     # seams and tail inside a k-pair
    assert {k[c]["cout"] for c in ("cout2", "cout7", "cout129", "cout192")} == {2, 7, 129, 192}
    gws = {c["cout"] // c["groups"] for c in k.values() if c["groups"]}
    assert {24, 32, 48} <= gws
    assert k["bias"]["bias"] and not k["bias"]["cbias"] and k["cbias"]["cbias"] and not k["cbias"]["bias"]
    assert k["both"]["bias"] and k["both"]["cbias"]
    assert {c["slope"] for c in k.values() if c["act"]} == {0.0, 0.2}
    assert k["fuse5"]["widths"] == (32,) * 5 and k["fuse5"]["groups"] == 20


@pytest.mark.parametrize("name", sorted(pc.POINTNET))
def test_pointnet_golden_within_bound(name):
    in_dim, gn, dims, cls, b, n = pc.POINTNET[name]
    net = rb.load(rb.PointNet(in_dim, gn, list(dims), cls), "pointnet", name)
    x = pc.pointnet_input(name)
    want, bound = pr.backbone(rb.layer_arrays(net.backbone), x)[-1]
    assert pr.ratio(GOLD[f"pointnet/{name}/f"], want, bound) <= 1
    assert pr.ratio(GOLD[f"pointnet/{name}/g"], want.max(2), bound.max(2)) <= 1
    with torch.no_grad():      # and the stand-in computes what the reference did
        f, g = net(torch.from_numpy(x))
    assert pr.ratio(f.numpy(), GOLD[f"pointnet/{name}/f"], 2 * bound) <= 1
    assert pr.ratio(g.numpy(), GOLD[f"pointnet/{name}/g"], 2 * bound.max(2)) <= 1


def test_cg_golden_within_both_forms_bounds():
    """The reference's CG outputs within the bound of its own form (one 6144-term product), and the split
    form's restatement within the sum of the two forms' bounds of it."""
    net = rb.load(rb.CGModule(3, False), "cg")
    src, tgt = pc.cg_inputs()
    ref_form, split = rb.cg_reference_form(net, src, tgt), rb.cg_split_form(net, src, tgt)
    for key in ("qt", "x_ol", "y_ol"):
        assert pr.ratio(GOLD[f"cg/{key}"], *ref_form[key]) <= 1
        assert pr.ratio(split[key][0], ref_form[key][0], split[key][1] + ref_form[key][1]) <= 1
        # in f64 the two forms are one function: they differ by f64 rounding of 6144-term sums only
        assert np.abs(split[key][0] - ref_form[key][0]).max() <= 1e-9 * max(1.0, np.abs(ref_form[key][0]).max())


def test_tiny_network_sorts_are_decided():
    """The maker's search: in the reference's f64 run every cut (N1 / M1 of the overlap scores, N2 of
    similarity_max, top-1 to top-2 of every kept row, each iteration, no row or cloud left out) is wider
    than GAP_FACTOR x the measured f32 deviation of the quantity sorted."""
    gaps = GOLD["net/gaps"]
    assert int(GOLD["net/seed"]) == pc.NET_SEED
    assert gaps.shape == (2 + 2 * pc.NET["num_iter"], 2)
    assert (gaps[:, 1] > 0).all() and (gaps[:, 0] > pc.GAP_FACTOR * gaps[:, 1]).all(), gaps
    n2 = int(pc.NET["top_prob"] * pc.NET["N1"])
    assert GOLD["net/src_ol1"].shape == (pc.NET["b"], pc.NET["N1"], 3)
    assert GOLD["net/src_ol2"].shape == (pc.NET["b"], n2, 3)
    assert float(GOLD["net/dev/src_ol1"]) == 0 and float(GOLD["net/dev/src_ol2"]) == 0   # the f32 run chose the same


def test_abi_is_declared_and_the_struct_matches_the_header(tmp_path):
    """The two entries are exported, declared in _lib, and _lib.PointwiseArgs has the size and the field
    offsets a C compiler gives pcr_pointwise_args."""
    import ctypes
    import subprocess
    from pointcloudregistration_amd import _lib
    lib = _lib.load()
    for s in ("pcr_pointwise_forward", "pcr_pointwise_scratch_bytes"):
        assert s in _lib.exported_symbols() and hasattr(lib, s)
    assert len(_lib.SIGNATURES["pcr_pointwise_forward"]) == 3
    fields = ("b", "c", "src", "sub_cs", "w", "w_ld", "cbias", "gw", "eps", "gamma", "act", "slope", "res",
              "out_cs", "cmax", "stats")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "abi.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "pcr_api.h"\nint main(void) {\n'
                   '  printf("%zu", sizeof(pcr_pointwise_args));\n'
                   + "".join(f'  printf(" %zu", offsetof(pcr_pointwise_args, {f}));\n' for f in fields)
                   + "  return 0;\n}\n")
    exe = tmp_path / "abi"
    subprocess.run(["cc", "-I", os.path.join(root, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    want = [ctypes.sizeof(_lib.PointwiseArgs)] + [getattr(_lib.PointwiseArgs, f).offset for f in fields]
    assert got == want
    assert lib.pcr_pointwise_scratch_bytes(2, 2048, 960) == (2 * 2 * 960 * 4 + 15) // 16 * 16 + 2 * 2 * 32 * 960 * 8
    assert lib.pcr_pointwise_scratch_bytes(1, -1, 4) == -1 and b"n=-1" in lib.pcr_last_error()
