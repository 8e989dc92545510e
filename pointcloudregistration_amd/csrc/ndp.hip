// a10: NDP deformation-pyramid warp, all levels fused in one launch
// (c2p-net/deformationpyramid/model/nets.py: Deformation_Pyramid.warp :36-48,
// NDPLayer.forward :111-140, posenc :164-177, get_Rotation axis_angle :144-161
// -> rigid_body.exp_so3/skew :89-95,:113-119, MLP :295-304; SE3 motion).
//
// Per level, for every point: pe = [sin wx, cos wx, sin wy, cos wy, sin wz,
// cos wz] (w = 2^(m+k0)), h = ReLU(W_in pe + b), depth-1 x h = ReLU(W h + b),
// r = 1e-3 (W_rot h + b), t = 1e-3 (W_trn h + b), R = exp_so3(r/|r|, |r|),
// x' = R x + t, and with a nonrigidity branch x' = x + s (x' - x),
// s = sigmoid(1e-3 (W_nr h + b)).  f32 throughout, as the reference.  That is
// the SE3 / axis_angle head; the other eight (euler, quaternion and 6D
// rotations, Sim3 and scene-flow motion; get_Rotation :144-161, rigid_body.py)
// are written out in ndp_head.h, one kernel instantiation per head.
//
// MI355X design: a workgroup of NT = width/32 waves owns 32 points across all
// levels, wave w computing feature tile w of every layer.  Every layer is a
// chain of exact-f32 v_mfma_f32_32x32x2_f32: the activation tile H (32 features
// x 32 points, features in the 16 accumulator registers, points on lanes) is
// the B operand of the next layer directly -- k-step r of input tile it takes
// the feature row (r&3) + 8(r>>2) + 4(lane>>5) that the lane already holds, and
// the A operand (weights) is read in that permuted k order; the other waves'
// tiles arrive through LDS in that layout (ndp_tile.h), in the chain order of
// one wave holding all tiles, so the split changes no bits while a 20k-point
// cloud runs NT x 625 waves.  Wave 0 runs the branch head and the warp and
// hands the new points to the others through LDS.  Biases seed the
// accumulators.  The weights (nn.Linear layout, ~140 KB per level at width
// 128) stream through L1/L2; a lane's 16 k-steps of one 32-column block share
// one 128-byte line.
#include "pcr_internal.h"
#include "ndp_tile.h"
#include "ndp_head.h"

namespace pcr {
namespace {

using ndpt::chain;
using ndpt::f32x16;
using ndpt::frow;
using ndpt::publish;
using ndpt::TileX;

constexpr int kMaxLevels = 16;

struct NdpLevelDev {
    const float *w_in, *b_in, *w_hid, *b_hid, *w_rot, *b_rot, *w_trn, *b_trn, *w_nr, *b_nr, *w_s, *b_s;
    int m;
};

struct NdpArgs {
    const float *x;
    int N, nlev, depth, k0;
    float *x_out, *x_levels, *nonrig;
    NdpLevelDev lv[kMaxLevels];
};

// torch's ReLU: NaN stays NaN (fmaxf(NaN, 0) is 0, which gave a point that an
// earlier level had made NaN a finite nonrigidity where the reference has NaN)
__device__ __forceinline__ float relu(float v) { return v < 0.0f ? 0.0f : v; }

template <int NT, int HEAD>
__global__ __launch_bounds__(64 * NT) void ndp_warp_kernel(NdpArgs a) {
    constexpr int W = 32 * NT;
    __shared__ TileX X[NT];
    __shared__ float xn[3][32];
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63, h = l >> 5, j = l & 31;
    const int pt = blockIdx.x * 32 + j;
    const bool valid = pt < a.N;
    float x0 = 0.f, x1 = 0.f, x2 = 0.f;
    if (valid) { x0 = a.x[3 * pt]; x1 = a.x[3 * pt + 1]; x2 = a.x[3 * pt + 2]; }
    for (int lv = 0; lv < a.nlev; ++lv) {
        const NdpLevelDev &L = a.lv[lv];
        const float wf = __builtin_ldexpf(1.0f, L.m + a.k0);
        // positional encoding as the input layer's B operand: k = 2s + h
        float pe[3];
        {
            const float v0 = x0 * wf, v1 = x1 * wf, v2 = x2 * wf;
            pe[0] = h ? cosf(v0) : sinf(v0);
            pe[1] = h ? cosf(v1) : sinf(v1);
            pe[2] = h ? cosf(v2) : sinf(v2);
        }
        f32x16 H;
#pragma unroll
        for (int r = 0; r < 16; ++r) H[r] = L.b_in[32 * w + frow(r, h)];
        {
            const float *wr = L.w_in + (32 * w + j) * 6;
#pragma unroll
            for (int s = 0; s < 3; ++s) H = __builtin_amdgcn_mfma_f32_32x32x2f32(wr[2 * s + h], pe[s], H, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) H[r] = relu(H[r]);
        for (int hl = 0; hl + 1 < a.depth; ++hl) {
            publish(X[w], l, H);
            __syncthreads();
            const float *wr = L.w_hid + (size_t)hl * W * W + (size_t)(32 * w + j) * W;
            const float *bm = L.b_hid + (size_t)hl * W;
            f32x16 Hn;
#pragma unroll
            for (int r = 0; r < 16; ++r) Hn[r] = bm[32 * w + frow(r, h)];
            Hn = chain<NT>(X, l, [&](int it, int r) { return wr[32 * it + frow(r, h)]; }, Hn);
            __syncthreads();
#pragma unroll
            for (int r = 0; r < 16; ++r) H[r] = relu(Hn[r]);
        }
        publish(X[w], l, H);
        __syncthreads();
        if (w == 0) {
            // branches in one 32-row tile (row map of the head: ndp_head.h)
            const bool has_nr = L.w_nr != nullptr;
            const ndph::BranchW bw{L.w_rot, L.b_rot, L.w_trn, L.b_trn, L.w_nr, L.b_nr, L.w_s, L.b_s};
            const float *br = ndph::branch_row<HEAD>(bw, j, W);
            f32x16 Bo;
#pragma unroll
            for (int r = 0; r < 16; ++r) Bo[r] = ndph::branch_bias<HEAD>(bw, frow(r, h));
            Bo = chain<NT>(X, l, [&](int it, int r) { return br ? br[32 * it + frow(r, h)] : 0.0f; }, Bo);
            ndph::HeadOut<HEAD> ho;
            ndph::head_forward<HEAD>(Bo, h, has_nr, x0, x1, x2, ho);
            const float n0 = ho.n[0], n1 = ho.n[1], n2 = ho.n[2], sg = ho.s;
            if (h == 0) {
                xn[0][j] = n0; xn[1][j] = n1; xn[2][j] = n2;
                if (valid) {
                    if (a.x_levels) {
                        float *o = a.x_levels + ((size_t)lv * a.N + pt) * 3;
                        o[0] = n0; o[1] = n1; o[2] = n2;
                    }
                    if (a.nonrig && has_nr) a.nonrig[(size_t)lv * a.N + pt] = sg;
                }
            }
        }
        __syncthreads();
        x0 = xn[0][j]; x1 = xn[1][j]; x2 = xn[2][j];
    }
    if (valid && h == 0 && w == 0) {
        a.x_out[3 * pt] = x0;
        a.x_out[3 * pt + 1] = x1;
        a.x_out[3 * pt + 2] = x2;
    }
}

}  // namespace
}  // namespace pcr

extern "C" int pcr_ndp_warp(const float *x, int32_t N, const pcr_ndp_level *levels,
                            int32_t n_levels, int32_t width, int32_t depth, int32_t k0,
                            float *x_out, float *x_levels, float *nonrigidity,
                            pcr_stream_t stream) {
    pcr::clear_error();
    PCR_REQUIRE(N >= 0 && n_levels >= 0, PCR_ERR_ARG, "ndp_warp: negative size");
    PCR_REQUIRE(n_levels <= pcr::kMaxLevels, PCR_ERR_ARG, "ndp_warp: %d levels > %d", n_levels,
                pcr::kMaxLevels);
    PCR_REQUIRE(width == 32 || width == 64 || width == 96 || width == 128, PCR_ERR_ARG,
                "ndp_warp: width %d not in {32, 64, 96, 128}", width);
    PCR_REQUIRE(depth >= 1, PCR_ERR_ARG, "ndp_warp: depth must be >= 1");
    if (N == 0) return PCR_OK;
    PCR_REQUIRE(x && x_out && (levels || n_levels == 0), PCR_ERR_ARG, "ndp_warp: null pointer");
    pcr::NdpArgs a;
    a.x = x; a.N = N; a.nlev = n_levels; a.depth = depth; a.k0 = k0;
    a.x_out = x_out; a.x_levels = x_levels; a.nonrig = nonrigidity;
    const int head = n_levels ? levels[0].head : 0;
    PCR_REQUIRE(pcr::ndph::head_valid(head), PCR_ERR_ARG, "ndp_warp: unknown head code %d", head);
    const int motion = pcr::ndph::head_motion(head);
    for (int i = 0; i < n_levels; ++i) {
        const pcr_ndp_level &s = levels[i];
        PCR_REQUIRE(s.head == head, PCR_ERR_ARG, "ndp_warp: level %d has head code %d, level 0 has %d (%s)", i,
                    s.head, head, pcr::ndph::head_name(head));
        PCR_REQUIRE(s.w_in && s.b_in && s.w_trn && s.b_trn && (depth == 1 || (s.w_hid && s.b_hid)) &&
                        (!s.w_nr || s.b_nr),
                    PCR_ERR_ARG, "ndp_warp: level %d has a null weight", i);
        PCR_REQUIRE(motion == pcr::ndph::kSflow || (s.w_rot && s.b_rot), PCR_ERR_ARG,
                    "ndp_warp: level %d of head %s has no rotation branch", i, pcr::ndph::head_name(head));
        PCR_REQUIRE(motion != pcr::ndph::kSim3 || (s.w_s && s.b_s), PCR_ERR_ARG,
                    "ndp_warp: level %d of head %s has no scale branch (w_s, b_s)", i, pcr::ndph::head_name(head));
        a.lv[i] = pcr::NdpLevelDev{s.w_in, s.b_in, s.w_hid, s.b_hid, s.w_rot, s.b_rot, s.w_trn,
                                   s.b_trn, s.w_nr, s.b_nr, s.w_s, s.b_s, s.m};
    }
    hipStream_t st = pcr::as_stream(stream);
    const dim3 g((unsigned)((N + 31) / 32));  // 32 points per workgroup, a wave per feature tile
#define PCR_NDP_WARP(HEAD)                                                                             \
    case HEAD:                                                                                         \
        switch (width / 32) {                                                                          \
            case 1: hipLaunchKernelGGL((pcr::ndp_warp_kernel<1, HEAD>), g, dim3(64), 0, st, a); break;  \
            case 2: hipLaunchKernelGGL((pcr::ndp_warp_kernel<2, HEAD>), g, dim3(128), 0, st, a); break; \
            case 3: hipLaunchKernelGGL((pcr::ndp_warp_kernel<3, HEAD>), g, dim3(192), 0, st, a); break; \
            default: hipLaunchKernelGGL((pcr::ndp_warp_kernel<4, HEAD>), g, dim3(256), 0, st, a); break; \
        }                                                                                              \
        break;
    switch (head) {
        PCR_NDP_WARP(0) PCR_NDP_WARP(1) PCR_NDP_WARP(2) PCR_NDP_WARP(3) PCR_NDP_WARP(4)
        PCR_NDP_WARP(5) PCR_NDP_WARP(6) PCR_NDP_WARP(7) PCR_NDP_WARP(8)
    }
#undef PCR_NDP_WARP
    PCR_LAUNCH_CHECK();
    return PCR_OK;
}
