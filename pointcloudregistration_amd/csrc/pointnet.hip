// DIP's PointNet descriptor forward (dip/network.py:50-100, eval mode) with no
// per-point activation in global memory.  Contract and numerics:
// include/pcr_api.h; f64 restatement with the derived bounds:
// tests/pointnet_ref.py.
//
// Two kernels, each used by the T-net and by the main branch with that
// branch's folded weights.
//
// pointnet_points: x (3, P) of a patch -> mx, amx (256).  One 256-thread
// workgroup per patch (a workgroup walks patches blockIdx.x, + gridDim.x, ...).
//  * A wave owns 64 of the 256 output channels, and keeps ITS rows of W2' in
//    registers for the whole kernel: lane (lr, hh) of wave w holds, for the two
//    channels o = 64 w + 32 ct + lr, the 64 weights W2'[o][2 t + hh] -- 128
//    VGPRs, as they sit the B operand of v_mfma_f32_32x32x2_f32's k-step t.
//    W2' is read from L2 once per workgroup, not once per tile.
//  * Points go in tiles of 64.  Per tile: the three coordinates are staged in
//    LDS (transformed first where the call has a T-net; xtrans is written from
//    there), layer 1 (3 -> 128, VALU fmaf, 32 values per thread) writes the
//    128 x 64 h1 tile to LDS as the A operand, pair-interleaved -- element
//    (c, p) at ((c >> 1) * 64 + p) * 2 + (c & 1), so the 64 lanes of a k-step
//    read 64 consecutive words (no bank conflict, no padding: 32 KiB) -- and
//    layer 2 is 64 k-steps x 2 x 2 accumulators of 32 x 32 (points on the
//    MFMA's rows, channels on its columns: a lane ends with 16 points of ITS
//    channel per accumulator).
//  * The running maximum and its point stay in registers across tiles: a
//    lane meets its points in ascending order, so a strict > keeps the lowest
//    index; the two lane halves (rows 4 hh apart) are folded once at the end.
//  * Layer 1's 512 weights and biases sit in LDS too (one broadcast read of
//    16 bytes per channel).
// Budget: 35.5 KiB LDS; 128 (weights) + 64 (accumulators) of 292 registers per
// lane, no spill: one wave per SIMD, which four independent accumulators keep
// at the f32 MFMA's issue rate.  Measured: DESIGN.md.
//
// pointnet_heads: mx (256) -> hid (128) -> f (dim) for 32 patches per
// workgroup, patches on the MFMA's rows, so W3' and W4' are read once per 32
// patches.  mx and hid sit in LDS with strides 258 and 130 (a k-step's 64
// lanes hit 64 banks); a wave owns 32 channels of fc1 and every fourth
// 32-channel tile of fc2.  Epilogue: + I (the T-net's head) or the l2
// normalisation, one thread per patch summing the squares.  49.6 KiB LDS.
#include <math.h>

#include "pcr_internal.h"
#include "wave.h"

namespace {

using pcr::cdiv64;
using pcr::f32x16;
using pcr::tile_row;

constexpr int kThreads = 256;
constexpr int kTile = 64;      // points per tile
constexpr int kC1 = 128;       // conv1 / fc1 outputs
constexpr int kC2 = 256;       // conv2 outputs (the pooled vector)
constexpr int kGroup = 32;     // patches per heads workgroup
constexpr int kMLd = kC2 + 2;  // mx rows in LDS
constexpr int kHLd = kC1 + 2;  // hid rows in LDS
constexpr int kFLd = kC2 + 1;  // f rows in LDS (aliases the mx rows)
constexpr int kMaxDim = 256;
constexpr int kMaxP = 4096;
constexpr int kMaxB = 1 << 20;
constexpr int kMaxPointBlocks = 512;  // two workgroups per CU

struct PointArgs {
    const float *x; long long sb, sc, sp;  // element (b, coord, point)
    const float *w1, *b1, *w2, *b2;        // (128, 3), (128), (256, 128), (256)
    const float *trans;                    // (B, 9): transform the patch first; or null
    float *xtrans;                         // (B, 3, P) or null
    float *mx;                             // (B, 256)
    int32_t *amx;                          // (B, 256) or null
    int B, P;
};

__global__ __launch_bounds__(kThreads) void pointnet_points(PointArgs a) {
    __shared__ float Xs[3 * kTile];
    __shared__ __attribute__((aligned(16))) float Hs[kC1 * kTile];
    __shared__ __attribute__((aligned(16))) float W1s[kC1 * 4];  // per channel: its three weights, its bias

    const int tid = threadIdx.x, l = tid & 63, hh = l >> 5, lr = l & 31;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int P = a.P;

    // layer 1's weights go through LDS: as scalar loads they are hoisted out of the tile loop,
    // 512 values that the scalar registers cannot hold.  The first tile's barrier publishes them.
    if (tid < kC1) {
        W1s[4 * tid + 0] = a.w1[3 * tid + 0];
        W1s[4 * tid + 1] = a.w1[3 * tid + 1];
        W1s[4 * tid + 2] = a.w1[3 * tid + 2];
        W1s[4 * tid + 3] = a.b1[tid];
    }

    // the wave's rows of W2', as the B operand of k-step t (channel 2 t + hh)
    float wr[2][kC1 / 2], bias[2];
#pragma unroll
    for (int ct = 0; ct < 2; ++ct) {
        const int o = wid * 64 + ct * 32 + lr;
        const float *row = a.w2 + (size_t)o * kC1 + hh;
#pragma unroll
        for (int t = 0; t < kC1 / 2; ++t) wr[ct][t] = row[2 * t];
        bias[ct] = a.b2[o];
    }

    for (int b = blockIdx.x; b < a.B; b += gridDim.x) {
        float T[9];
        if (a.trans) {
#pragma unroll
            for (int e = 0; e < 9; ++e) T[e] = a.trans[(size_t)b * 9 + e];
        }
        float m[2] = {-INFINITY, -INFINITY};
        int am[2] = {0x7fffffff, 0x7fffffff};

        for (int p0 = 0; p0 < P; p0 += kTile) {
            __syncthreads();  // the last tile's readers of Xs and Hs are done
            if (tid < 3 * kTile) {
                const int r = wid, p = p0 + l;
                float v = 0.0f;  // a point past P: staged as +0, kept out of the pool below
                if (p < P) {
                    const float *xp = a.x + b * a.sb + p * a.sp;
                    if (a.trans) {
                        const float x0 = xp[0], x1 = xp[a.sc], x2 = xp[2 * a.sc];
                        v = __fadd_rn(__fadd_rn(__fmul_rn(T[3 * r], x0), __fmul_rn(T[3 * r + 1], x1)),
                                      __fmul_rn(T[3 * r + 2], x2));
                    } else {
                        v = xp[r * a.sc];
                    }
                    if (a.xtrans) a.xtrans[((size_t)b * 3 + r) * P + p] = v;
                }
                Xs[r * kTile + l] = v;
            }
            __syncthreads();

            {   // layer 1 on the VALU: thread (wave w, point l) makes channels 32 w .. 32 w + 31
                const float x0 = Xs[l], x1 = Xs[kTile + l], x2 = Xs[2 * kTile + l];
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    const int c = wid * 32 + 2 * j;
                    float h[2];
#pragma unroll
                    for (int e = 0; e < 2; ++e) {
                        const float4 w = *reinterpret_cast<const float4 *>(W1s + 4 * (c + e));
                        const float y = fmaf(w.z, x2, fmaf(w.y, x1, fmaf(w.x, x0, w.w)));
                        h[e] = fmaxf(y, 0.0f);
                    }
                    *reinterpret_cast<float2 *>(Hs + ((c >> 1) * kTile + l) * 2) = make_float2(h[0], h[1]);
                }
            }
            __syncthreads();

            f32x16 acc[2][2];
#pragma unroll
            for (int ct = 0; ct < 2; ++ct)
#pragma unroll
                for (int pt = 0; pt < 2; ++pt)
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[ct][pt][r] = bias[ct];
#pragma unroll
            for (int t = 0; t < kC1 / 2; ++t) {
                const float a0 = Hs[(t * kTile + lr) * 2 + hh];
                const float a1 = Hs[(t * kTile + 32 + lr) * 2 + hh];
                acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, wr[0][t], acc[0][0], 0, 0, 0);
                acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, wr[0][t], acc[0][1], 0, 0, 0);
                acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, wr[1][t], acc[1][0], 0, 0, 0);
                acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, wr[1][t], acc[1][1], 0, 0, 0);
            }

            // ReLU and pool: the lane's points come in ascending order
#pragma unroll
            for (int pt = 0; pt < 2; ++pt)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int p = p0 + pt * 32 + tile_row(r, hh);
                    const bool in = p < P;  // used at once for both channels: 32 masks kept would not fit
#pragma unroll
                    for (int ct = 0; ct < 2; ++ct) {
                        const float v = in ? fmaxf(acc[ct][pt][r], 0.0f) : -INFINITY;
                        const bool take = v > m[ct];  // selects, not 64 branches
                        m[ct] = take ? v : m[ct];
                        am[ct] = take ? p : am[ct];
                    }
                }
        }

#pragma unroll
        for (int ct = 0; ct < 2; ++ct) {  // the other lane half holds the channel's other points
            const float om = __shfl_xor(m[ct], 32, 64);
            const int oa = __shfl_xor(am[ct], 32, 64);
            if (om > m[ct] || (om == m[ct] && oa < am[ct])) {
                m[ct] = om;
                am[ct] = oa;
            }
            if (hh == 0) {
                const size_t at = (size_t)b * kC2 + wid * 64 + ct * 32 + lr;
                a.mx[at] = m[ct];
                if (a.amx) a.amx[at] = am[ct] == 0x7fffffff ? 0 : am[ct];  // no point won: non-finite data
            }
        }
    }
}

struct HeadArgs {
    const float *mx;                 // (B, 256)
    const float *w3, *b3, *w4, *b4;  // (128, 256), (128), (dim, 128), (dim)
    float *hid;                      // (B, 128) or null
    float *f;                        // (B, dim)
    int B, dim, l2norm, add_identity;
};

__global__ __launch_bounds__(kThreads) void pointnet_heads(HeadArgs a) {
    __shared__ float Ms[kGroup * kMLd];  // the group's mx rows; later its f rows (kFLd <= kMLd)
    __shared__ float Hl[kGroup * kHLd];
    __shared__ float Ds[kGroup];

    const int tid = threadIdx.x, l = tid & 63, hh = l >> 5, lr = l & 31;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int b0 = blockIdx.x * kGroup, B = a.B, dim = a.dim;

#pragma unroll 4
    for (int i = 0; i < kGroup; ++i)  // a row past B repeats the last patch and is not stored
        Ms[i * kMLd + tid] = a.mx[(size_t)min(b0 + i, B - 1) * kC2 + tid];
    __syncthreads();

    {   // fc1: the wave's 32 channels, 128 k-steps
        const int o = wid * 32 + lr;
        const float *w = a.w3 + (size_t)o * kC2 + hh;
        const float bo = a.b3[o];
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = bo;
#pragma unroll 16
        for (int t = 0; t < kC2 / 2; ++t)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(Ms[lr * kMLd + 2 * t + hh], w[2 * t], acc, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = tile_row(r, hh);
            const float v = fmaxf(acc[r], 0.0f);
            Hl[row * kHLd + o] = v;
            if (a.hid && b0 + row < B) a.hid[(size_t)(b0 + row) * kC1 + o] = v;
        }
    }
    __syncthreads();  // Hl is complete, and Ms has no reader left

    for (int ct = wid; ct * 32 < dim; ct += 4) {  // fc2: 32-channel tiles ct, ct + 4
        const int o = ct * 32 + lr, oc = min(o, dim - 1);  // a channel past dim repeats the last; not kept
        const float *w = a.w4 + (size_t)oc * kC1 + hh;
        const float bo = a.b4[oc];
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = bo;
#pragma unroll 16
        for (int t = 0; t < kC1 / 2; ++t)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(Hl[lr * kHLd + 2 * t + hh], w[2 * t], acc, 0, 0, 0);
        if (o < dim) {
#pragma unroll
            for (int r = 0; r < 16; ++r) Ms[tile_row(r, hh) * kFLd + o] = acc[r];
        }
    }
    __syncthreads();

    if (a.l2norm) {
        if (tid < kGroup) {  // squares summed over channels ascending, each operation rounded
            float s = 0.0f;
            for (int o = 0; o < dim; ++o) {
                const float v = Ms[tid * kFLd + o];
                s = __fadd_rn(s, __fmul_rn(v, v));
            }
            Ds[tid] = fmaxf(sqrtf(s), 1e-12f);
        }
        __syncthreads();
    }
    for (int i = tid; i < kGroup * dim; i += kThreads) {
        const int row = i / dim, o = i - row * dim;
        if (b0 + row >= B) break;
        float v = Ms[row * kFLd + o];
        if (a.l2norm) v = v / Ds[row];
        if (a.add_identity) v = __fadd_rn(v, (o & 3) == 0 ? 1.0f : 0.0f);  // dim = 9: elements 0, 4, 8
        a.f[(size_t)(b0 + row) * dim + o] = v;
    }
}

int check_sizes(const char *who, int B, int P, int dim) {
    PCR_REQUIRE(B >= 0 && B <= kMaxB, PCR_ERR_ARG, "%s: B=%d outside 0..%d", who, B, kMaxB);
    PCR_REQUIRE(P >= 1 && P <= kMaxP, PCR_ERR_ARG, "%s: P=%d outside 1..%d", who, P, kMaxP);
    PCR_REQUIRE(dim >= 1 && dim <= kMaxDim, PCR_ERR_ARG, "%s: dim=%d outside 1..%d", who, dim, kMaxDim);
    return PCR_OK;
}

bool complete(const pcr_pointnet_layers &y) {
    return y.w1 && y.b1 && y.w2 && y.b2 && y.w3 && y.b3 && y.w4 && y.b4;
}

// mx_t (B, 256) | trans (B, 16): the T-net's pooled vector and its matrix
long long scratch_floats(int B, int tnet) { return tnet ? (long long)B * (kC2 + 16) : 0; }

int branch(const PointArgs &pa, const pcr_pointnet_layers &y, float *hid, float *f, int dim, int l2norm,
           int add_identity, hipStream_t s) {
    const int B = pa.B;
    PointArgs p = pa;
    p.w1 = y.w1; p.b1 = y.b1; p.w2 = y.w2; p.b2 = y.b2;
    hipLaunchKernelGGL(pointnet_points, dim3((unsigned)(B < kMaxPointBlocks ? B : kMaxPointBlocks)), dim3(kThreads),
                       0, s, p);
    PCR_LAUNCH_CHECK();
    HeadArgs h;
    h.mx = p.mx; h.w3 = y.w3; h.b3 = y.b3; h.w4 = y.w4; h.b4 = y.b4;
    h.hid = hid; h.f = f; h.B = B; h.dim = dim; h.l2norm = l2norm; h.add_identity = add_identity;
    hipLaunchKernelGGL(pointnet_heads, dim3((unsigned)cdiv64(B, kGroup)), dim3(kThreads), 0, s, h);
    PCR_LAUNCH_CHECK();
    return PCR_OK;
}

}  // namespace

extern "C" int64_t pcr_pointnet_scratch_bytes(int32_t B, int32_t dim, int32_t tnet) {
    pcr::clear_error();
    if (check_sizes("pointnet_scratch_bytes", B, 1, dim) != PCR_OK) return -1;
    return (scratch_floats(B, tnet) * 4 + 255) / 256 * 256;
}

extern "C" int pcr_pointnet_forward(const float *x, int64_t x_sb, int64_t x_sc, int64_t x_sp, int32_t B, int32_t P,
                                    const pcr_pointnet_weights *w, int32_t dim, int32_t tnet, int32_t l2norm,
                                    float *f, float *mx, int32_t *amx, float *hid, float *trans, float *xtrans,
                                    void *scratch, pcr_stream_t stream) {
    pcr::clear_error();
    int rc = check_sizes("pointnet_forward", B, P, dim);
    if (rc != PCR_OK) return rc;
    if (B == 0) return PCR_OK;
    PCR_REQUIRE(w, PCR_ERR_ARG, "pointnet_forward: null weights");
    PCR_REQUIRE(complete(w->main), PCR_ERR_ARG, "pointnet_forward: null pointer among the main layers");
    PCR_REQUIRE(!tnet || complete(w->stn), PCR_ERR_ARG, "pointnet_forward: null pointer among the T-net's layers");
    PCR_REQUIRE(x && f && mx, PCR_ERR_ARG, "pointnet_forward: null pointer (x, f and mx are required)");
    PCR_REQUIRE(!tnet || scratch, PCR_ERR_ARG, "pointnet_forward: null scratch (a T-net call needs it)");
    PCR_REQUIRE(!tnet || ((uintptr_t)scratch & 15) == 0, PCR_ERR_ARG,
                "pointnet_forward: scratch is not 16-byte aligned");
    hipStream_t s = pcr::as_stream(stream);
    PointArgs p;
    p.x = x; p.sb = x_sb; p.sc = x_sc; p.sp = x_sp;
    p.w1 = p.b1 = p.w2 = p.b2 = nullptr;
    p.trans = nullptr; p.xtrans = nullptr; p.mx = mx; p.amx = amx; p.B = B; p.P = P;
    if (tnet) {
        float *mx_t = (float *)scratch;
        float *tr = trans ? trans : mx_t + (size_t)B * kC2;
        p.mx = mx_t; p.amx = nullptr;
        rc = branch(p, w->stn, nullptr, tr, 9, 0, 1, s);
        if (rc != PCR_OK) return rc;
        p.trans = tr; p.mx = mx; p.amx = amx;
    }
    p.xtrans = xtrans;
    return branch(p, w->main, hid, f, dim, l2norm, 0, s);
}
