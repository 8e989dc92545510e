"""GPU: the drop-in blocks of pointcloudregistration_amd.ngenet (Unary, NearestUpsample,
Simple, ResnetBottleneck), fuse() and forward() on reference-shaped composites
(tests/unary_blocks.py) with the golden cases' parameters.

Blocks: every stage within the restatement's bound (tests/unary_ref.py), the
tensors around the KPConv taken from the run itself by a forward hook, exactly
as make_golden_unary.py checks the reference's blocks.

ngenet.forward is a WIRING test against the reference's recorded h / m / l of
the tiny network (tests/golden/unary_cases.NET: the MRI architecture's three
decoder lists at small widths behind a stub encoder).  A wrong skip or branch
index moves the unit-norm features by O(0.1).  Tolerance: the maker measured the
torch f32 composite (the reference's own forward) against its f64 twin on the
same network on the CPU, max deviation 2.142e-04 (stored as net/deviation);
8 x that, 1.714e-03, is allowed for the different summation order over the
stacked layers."""
import functools
import os

import numpy as np
import pytest
import torch

import unary_blocks as ub
import unary_cases as uc
import unary_ref as ur

pytestmark = pytest.mark.gpu

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "unary_golden.npz"))
WIRING_FACTOR = 8


@pytest.mark.parametrize("name", sorted(uc.UNARY))
def test_unary_module_on_golden_cases(name):
    from pointcloudregistration_amd import ngenet
    n, cin, cout, use_bn, relu = uc.UNARY[name]
    c = uc.make_unary(name)
    mod = ngenet.Unary(cin, cout, use_bn, 0.02, relu=relu)
    sd = {"mlp.weight": torch.from_numpy(c["w"])}
    if not use_bn:
        sd["bn.bias"] = torch.from_numpy(c["bias"])
    mod.load_state_dict(sd, strict=True)
    mod = mod.cuda().eval()
    with torch.no_grad():
        got = mod(torch.from_numpy(c["x"]).cuda()).cpu().numpy()
    want, bound, _ = ur.unary(c["w"], c["x"], bias=c["bias"], norm=use_bn, eps=uc.EPS, slope=uc.SLOPE, act=relu)
    assert ur.ratio(got, want, bound) <= 1
    assert ur.ratio(got, GOLD[f"unary/{name}"], 2 * bound) <= 1      # both lie within the bound of the restatement


@pytest.mark.parametrize("name", sorted(uc.UPCAT))
def test_upsample_cat_unary_is_one_call(name):
    from pointcloudregistration_amd import ngenet
    m0, n, c0, c1, cout, use_bn, relu = uc.UPCAT[name]
    c = uc.make_upcat(name)
    blk = ub.UnaryBlock(c0 + c1, cout, use_bn, 0.02, relu=relu)
    blk.mlp.weight.data = torch.from_numpy(c["w"])
    if not use_bn:
        blk.bn.bias.data = torch.from_numpy(c["bias"])
    holder = torch.nn.ModuleList([ub.NearestUpsampleBlock(0), blk]).cuda().eval()
    assert ngenet.fuse(holder) == (1, 1, 0, 0)
    up, unary = holder
    x0, x1, table = (torch.from_numpy(c[k]).cuda() for k in ("x0", "x1", "up"))
    with torch.no_grad():
        fused = unary(x0, gather=table[:, 0], x1=x1)
        plain = unary(torch.cat([up(x0, {"upsamples": [table]}), x1], dim=1))   # the blocks one by one
    want, bound, _ = ur.unary(c["w"], c["x0"], c["up"][:, 0], c["x1"], bias=c["bias"], norm=use_bn, eps=uc.EPS,
                              slope=uc.SLOPE, act=relu)
    assert ur.ratio(fused.cpu().numpy(), want, bound) <= 1
    assert ur.ratio(fused.cpu().numpy(), GOLD[f"upcat/{name}"], 2 * bound) <= 1
    assert torch.equal(fused, plain), "the gather and the concat inside the kernel must not change a bit"


@pytest.mark.parametrize("order", ("ngenet, kpconv", "kpconv, ngenet", "ngenet"))
@pytest.mark.parametrize("name", sorted(uc.BLOCKS))
def test_block_stages_within_bound(name, order):
    from pointcloudregistration_amd import kpconv, ngenet
    kind = uc.BLOCKS[name][0]
    block, f, batch = ub.make_block(name)
    holder = torch.nn.ModuleList([block]).cuda()
    for step in order.split(", "):
        counts = ngenet.fuse(holder) if step == "ngenet" else kpconv.fuse(holder)
        assert counts[2 if kind == "simple" else 3] == 1 if step == "ngenet" else counts[0] == 1
    block = holder[0]
    assert isinstance(block, ngenet.Simple if kind == "simple" else ngenet.ResnetBottleneck)
    assert isinstance(block.KPConv, kpconv.KPConv) == ("kpconv" in order)
    rec = {}
    block.KPConv.register_forward_hook(lambda mod, inp, out: rec.update(conv_in=inp[2].cpu().numpy(),
                                                                        conv_out=out.cpu().numpy()))
    batch = {k: [t.cuda() for t in v] for k, v in batch.items()}
    with torch.no_grad():
        got = block(f.cuda(), batch).cpu().numpy()
    case = uc.make_block(name)
    st = ur.block_stages(kind, case, rec["conv_in"], rec["conv_out"], uc.EPS, uc.SLOPE)
    if st["conv_in"] is not None:
        assert ur.ratio(rec["conv_in"], *st["conv_in"]) <= 1
    assert ur.ratio(rec["conv_out"], *st["conv_out"]) <= 1
    r = ur.ratio(got, *st["out"])
    print(f"{name} ({order}): out err / bound = {r:.4f}")
    assert r <= 1
    assert got.shape == GOLD[f"block/{name}/out"].shape


@functools.lru_cache(maxsize=None)
def tiny(fused):
    """The tiny network on the device with the case's parameters (strict load), and its inputs."""
    from pointcloudregistration_amd import attention, groupmlp, kpconv, ngenet
    case = uc.make_net()
    net = ub.load_net(ub.TinyNet(ub.decider), case["params"]).cuda()
    if fused:
        assert ngenet.fuse(net) == (16, 6, 0, 0)
        assert kpconv.fuse(net) == (0, 3)
        assert attention.fuse(net) == (0, 0) and groupmlp.fuse(net) == (0, 0, 0)
        assert ngenet.fuse(net) == (0, 0, 0, 0)
    return net, ub.net_inputs(case["inputs"], device="cuda")


@pytest.mark.parametrize("fused", (False, True))
def test_forward_wiring_against_the_reference(fused):
    """See the module docstring for the tolerance (8 x 2.142e-04 = 1.714e-03)."""
    from pointcloudregistration_amd import ngenet
    net, inputs = tiny(fused)
    with torch.no_grad():
        outs = ngenet.forward(net, inputs)
    dev = float(GOLD["net/deviation"])
    tol = WIRING_FACTOR * dev
    assert abs(dev - 2.142e-04) < 1e-6, "the docstring's figures are the maker's"
    for key, got in zip("hml", outs):
        gold = GOLD[f"net/{key}"]
        err = float(np.abs(got.cpu().numpy() - gold).max())
        print(f"net/{key} fused={fused}: max |diff| {err:.3e}, tolerance {tol:.3e}")
        assert got.shape == gold.shape and err <= tol, (key, err, tol)


def test_forward_wiring_has_teeth():
    """Another up-sampling table, or the skips of another level, move the outputs far past the tolerance."""
    from pointcloudregistration_amd import ngenet
    net, inputs = tiny(True)
    tol = WIRING_FACTOR * float(GOLD["net/deviation"])
    wrong = dict(inputs)
    wrong["upsamples"] = [inputs["upsamples"][0].roll(1, 0)] + list(inputs["upsamples"][1:])
    with torch.no_grad():
        outs = ngenet.forward(net, wrong)
    for key, got in zip("hml", outs):
        assert float(np.abs(got.cpu().numpy() - GOLD[f"net/{key}"]).max()) > 10 * tol, key


def test_describe_splits_the_levels_per_cloud():
    from pointcloudregistration_amd import c2p, ngenet
    net, inputs = tiny(True)
    src, tgt = c2p.describe(net, inputs)
    with torch.no_grad():
        h, m, lo = ngenet.forward(net, inputs)
    n_src = uc.NET["lengths"][0][0]
    assert [tuple(t.shape) for t in src] == [(n_src, uc.NET["final"])] * 3
    assert [t.shape[0] for t in tgt] == [uc.NET["lengths"][0][1]] * 3
    assert torch.equal(src[0], h[:n_src, :-2]) and torch.equal(tgt[1], m[n_src:]) and torch.equal(src[2], lo[:n_src])
    assert all(t.is_cuda and not t.requires_grad for t in src + tgt)


def test_forward_refuses_what_it_cannot_fuse():
    from pointcloudregistration_amd import ngenet
    net, inputs = tiny(False)
    with pytest.raises(RuntimeError, match="forward-only"):
        ngenet.forward(net, inputs)                      # grad mode: the parameters require grad
    import copy
    odd = copy.deepcopy(net)
    odd.decoder_blocks[1] = torch.nn.Linear(48, 8).cuda()
    with torch.no_grad(), pytest.raises(ValueError, match="neither an up-sampling nor a unary"):
        ngenet.forward(odd, inputs)
