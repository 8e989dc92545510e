"""Torch composites with the attribute names, state-dict keys and arithmetic of the
reference's KPConv blocks (c2p-net/ngenet/models/KPConv/blocks.py:44-290), written
for the tests: the reference is not importable where the GPU tests run, and
ngenet.fuse goes by class name and attribute shape.  Also the stub interaction
block and the builder of the wiring test's tiny network (tests/golden/unary_cases.py),
which make_golden_unary.py shares so that the golden and the tests run one net.
"""
import numpy as np
import torch
from torch import nn

import unary_cases as uc


class KPConv(nn.Module):
    def __init__(self, in_channels, out_channels, radius, K, KP_extent):
        super().__init__()
        self.in_channels, self.out_channels, self.radius, self.K = in_channels, out_channels, radius, K
        self.KP_extent, self.KP_influence, self.aggregation_mode = KP_extent, "linear", "sum"
        self.weights = nn.Parameter(torch.zeros(K, in_channels, out_channels))
        self.kernel_points = nn.Parameter(torch.zeros(K, 3), requires_grad=False)

    def forward(self, q, s, f, idx):
        s = torch.cat([s, torch.zeros_like(s[:1]) + 1e6], 0)
        f = torch.cat([f, torch.zeros_like(f[:1])], 0)
        nf = f[idx]
        d = (s[idx] - q[:, None]).unsqueeze(2) - self.kernel_points
        h = torch.clamp(1 - torch.sqrt((d ** 2).sum(-1) + 1e-8) / self.KP_extent, min=0).transpose(1, 2)
        out = torch.matmul(torch.matmul(h, nf).transpose(0, 1), self.weights).sum(0)
        return out / torch.clamp((nf.sum(-1) > 0).sum(-1), min=1).unsqueeze(1)


class BatchNormBlock(nn.Module):
    def __init__(self, in_dim, use_bn, bn_momentum):
        super().__init__()
        self.use_bn = use_bn
        if use_bn:
            self.batch_norm = nn.InstanceNorm1d(in_dim, momentum=bn_momentum)
        else:
            self.bias = nn.Parameter(torch.zeros(in_dim))

    def forward(self, x):
        if self.use_bn:
            return self.batch_norm(x.t().unsqueeze(0)).squeeze(0).t().contiguous()
        return x + self.bias


class UnaryBlock(nn.Module):
    def __init__(self, in_dim, out_dim, use_bn, bn_momentum, relu=True):
        super().__init__()
        self.relu = relu
        self.mlp = nn.Linear(in_dim, out_dim, bias=False)
        self.bn = BatchNormBlock(out_dim, use_bn, bn_momentum)
        if relu:
            self.leaky_relu = nn.LeakyReLU(0.1)

    def forward(self, x, batch=None):
        x = self.bn(self.mlp(x))
        return self.leaky_relu(x) if self.relu else x


class MaxPoolBlock(nn.Module):
    def __init__(self, layer_ind):
        super().__init__()
        self.layer_ind = layer_ind

    def forward(self, feats, batch):
        padded = torch.cat([feats, torch.zeros_like(feats[:1])], 0)
        return padded[batch["pools"][self.layer_ind]].max(dim=1)[0]


class NearestUpsampleBlock(nn.Module):
    def __init__(self, layer_ind):
        super().__init__()
        self.layer_ind = layer_ind

    def forward(self, feats, batch):
        return feats[batch["upsamples"][self.layer_ind][:, 0]]


def _conv_inputs(block, batch):
    s = batch["points"][block.layer_ind]
    if "strided" in block.block_name:
        return batch["points"][block.layer_ind + 1], s, batch["pools"][block.layer_ind]
    return s, s, batch["neighbors"][block.layer_ind]


class SimpleBlock(nn.Module):
    def __init__(self, block_name, in_dim, out_dim, radius, use_bn, bn_momentum, layer_ind, K, KP_extent):
        super().__init__()
        self.block_name, self.layer_ind, self.in_dim, self.out_dim, self.radius = block_name, layer_ind, in_dim, \
            out_dim, radius
        self.KPConv = KPConv(in_dim, out_dim // 2, radius, K, KP_extent)
        self.bn = BatchNormBlock(out_dim // 2, use_bn, bn_momentum)
        self.leaky_relu = nn.LeakyReLU(0.1)

    def forward(self, s_feats, batch):
        return self.leaky_relu(self.bn(self.KPConv(*_conv_inputs(self, batch)[:2], s_feats,
                                                   _conv_inputs(self, batch)[2])))


class ResnetBottleneckBlock(nn.Module):
    def __init__(self, block_name, in_dim, out_dim, radius, use_bn, bn_momentum, layer_ind, K, KP_extent):
        super().__init__()
        self.block_name, self.layer_ind, self.in_dim, self.out_dim, self.radius = block_name, layer_ind, in_dim, \
            out_dim, radius
        mid = out_dim // 4
        self.unary1 = UnaryBlock(in_dim, mid, use_bn, bn_momentum) if in_dim != mid else nn.Identity()
        self.KPConv = KPConv(mid, mid, radius, K, KP_extent)
        self.bn = BatchNormBlock(mid, use_bn, bn_momentum)
        self.unary2 = UnaryBlock(mid, out_dim, use_bn, bn_momentum, relu=False)
        self.max_pool = MaxPoolBlock(layer_ind)
        self.unary_shortcut = UnaryBlock(in_dim, out_dim, use_bn, bn_momentum, relu=False) if in_dim != out_dim \
            else nn.Identity()
        self.leaky_relu = nn.LeakyReLU(0.1)

    def forward(self, s_feats, batch):
        q, s, idx = _conv_inputs(self, batch)
        x = self.unary2(self.leaky_relu(self.bn(self.KPConv(q, s, self.unary1(s_feats), idx))))
        short = self.max_pool(s_feats, batch) if "strided" in self.block_name else s_feats
        return self.leaky_relu(x + self.unary_shortcut(short))


def make_block(name):
    """The case's block with its parameters loaded (strict), and its inputs as torch tensors."""
    kind, in_dim, out_dim, use_bn = uc.BLOCKS[name]
    c = uc.make_block(name)
    g = uc.BLOCK_GEOMETRY
    cls = SimpleBlock if kind == "simple" else ResnetBottleneckBlock
    block = cls(kind, in_dim, out_dim, g["radius"], use_bn, 0.02, 0, g["K"], c["extent"])
    block.load_state_dict({k: torch.from_numpy(v) for k, v in c["params"].items()}, strict=True)
    batch = {k: [torch.from_numpy(a) for a in v] for k, v in c["batch"].items()}
    return block.eval(), torch.from_numpy(c["f"]), batch


class Interact(nn.Module):
    """Stub of the information-interaction block: two Conv1ds, each cloud's features plus the other
    cloud's mean features."""

    def __init__(self, dim):
        super().__init__()
        self.a, self.b = nn.Conv1d(dim, dim, 1), nn.Conv1d(dim, dim, 1)

    def forward(self, coords_src, feats_src, coords_tgt, feats_tgt, normals_src, normals_tgt):
        return (self.a(feats_src) + self.b(feats_tgt).mean(-1, keepdim=True),
                self.a(feats_tgt) + self.b(feats_src).mean(-1, keepdim=True))


class TinyNet(nn.Module):
    """The tiny network's submodules under NgeNet's attribute names (NgeNet.py:10-130); the decoder
    blocks come from `decider(block_name, in_dim, out_dim, layer_ind)`, the encoder is the stub plan."""

    def __init__(self, decider, unary=UnaryBlock, pool=MaxPoolBlock):
        super().__init__()
        g = uc.NET["gnn"]
        self.encoder_blocks = nn.ModuleList(
            unary(b[1], b[2], True, 0.02) if b[0] == "unary" else pool(b[1]) for b in uc.encoder_plan())
        self.encoder_skips, self.decoder_skips = list(uc.ENCODER_SKIPS), list(uc.DECODER_SKIPS)
        self.bottleneck = nn.Conv1d(uc.encoder_plan()[-1][2], g, 1)
        self.info_interative = Interact(g)
        self.pro_gnn, self.attn_score = nn.Conv1d(g, g, 1), nn.Conv1d(g, 1, 1)
        self.epsilon = nn.Parameter(torch.tensor(-5.0))
        h, m, lo = uc.decoder_plan()
        self.decoder_blocks = nn.ModuleList(decider(*b) for b in h)
        self.decoder_blocks_m = nn.ModuleList(decider(*b) for b in m)
        self.decoder_blocks_l = nn.ModuleList(decider(*b) for b in lo)
        self.sigmoid = nn.Sigmoid()


def decider(block_name, in_dim, out_dim, layer_ind, final=None):
    """block_decider (blocks.py:293-327) for the decoder's three block names, on this file's classes
    (final: final_feats_dim, the tiny network's by default)."""
    if block_name == "nearest_upsample":
        return NearestUpsampleBlock(layer_ind)
    if block_name == "last_unary":
        return UnaryBlock(in_dim, (final or uc.NET["final"]) + (0 if out_dim == -1 else 2), False, 0.02, relu=False)
    return UnaryBlock(in_dim, out_dim, True, 0.02)


def load_net(net, params):
    net.load_state_dict({k: torch.as_tensor(v) for k, v in params.items()}, strict=True)
    return net.eval()


def net_inputs(inputs, device="cpu", dtype=torch.float32):
    out = {}
    for k, v in inputs.items():
        conv = lambda a: torch.from_numpy(a).to(device=device, dtype=dtype if a.dtype == np.float32 else None)  # noqa: E731
        out[k] = [conv(a) for a in v] if isinstance(v, list) else conv(v)
    return out
