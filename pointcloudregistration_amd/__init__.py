"""pointcloudregistration_amd -- MI355X-native (gfx950) registration core.

Hot path of VatsalPandey0202/PointCloudRegistration rebuilt as HIP kernels behind
the C ABI in include/pcr_api.h (libpcr.so), with host-side mirrors of the
reference's operator interfaces:

  nndistance     torch_nndistance.nnd / NNDFunction / torch_nndistance_aten
  grouping       fps / gather_points / ball_query / sample_and_group of ROPNet's
                 model_utils and NgeNet's process, the fused PPF group, and the
                 k-NN graph and edge features (get_graph_features) of
                 NgeNet's GCN
  matching       the similarity top-k matching of ROPNet's TFMRModule.forward
                 (similarity, row selection, weights and correspondences)
  cpd            probreg.cpd's RigidCPD / AffineCPD / NonRigidCPD (Coherent
                 Point Drift) with a matrix-free E-step, and a batched loop
  attention      the softmax attention of NgeNet's Cross_Attention and overlap
                 scores and of ROPNet's OverlapAttentionBlock, fused (no score
                 matrix), with drop-in modules and fuse()
  pointnet       DIP's PointNetFeature forward (T-net, both MLPs, max-pool,
                 heads, l2 norm) fused for inference: fold / prepare /
                 describe, FusedPointNetFeature and fuse()
  groupmlp       what consumes grouping's PPF group and k-NN graph: the edge
                 conv of NgeNet's GCN and the grouped local-feature MLP of
                 NgeNet's PPF and ROPNet's LocalFeatue, fused (no per-neighbour
                 activation), with GCN / PPF / LocalFeature modules and fuse()
  ngenet         the unary family of NgeNet's KPConv blocks and decoder (rows
                 times weight, whole-cloud InstanceNorm, residual, LeakyReLU;
                 the decoder's up-sampling and concat inside the kernel), the
                 block modules and fuse(), and forward(): NgeNet end to end
  ropnet         ROPNet's point-wise convolutions (Conv1d weight times (B, C, N)
                 clouds, GroupNorm, biases, ReLU, residual and max over points
                 as one call; concat and subtraction inside the kernel), the
                 PointNet / CG / OverlapAttention modules and fuse(), and
                 forward(): ROPNet end to end
"""
from ._lib import PcrError, load as load_library  # noqa: F401

__all__ = ["PcrError", "load_library", "grouping", "matching", "cpd", "attention", "pointnet", "groupmlp", "ngenet", "ropnet"]


def __getattr__(name):
    # the op modules import torch; the package itself (ABI loader) does not
    if name in ("grouping", "matching", "cpd", "attention", "pointnet", "groupmlp", "ngenet", "ropnet"):
        import importlib
        return importlib.import_module("." + name, __name__)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
