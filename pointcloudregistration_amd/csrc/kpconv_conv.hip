// KPConv forward and the neighbour max-pool of NgeNet's encoder
// (c2p-net/ngenet/models/KPConv/blocks.py:73-128, 182-188) without the
// (n,k,C_in) gather, the (n,k,K,3) differences or the (n,K,C_in) kernel
// features in global memory.  Contract: include/pcr_api.h.
//
//  * kpconv_row_flags: one thread per support row, flag = (f32 sum of the row,
//    channels ascending) > 0.  m bytes, the only scratch.
//  * kpconv_fwd<NG>: one 256-thread workgroup per (16 queries, 256 output
//    channels; 64, 32 or 16 when the launch would otherwise leave CUs idle).  The input channels go in passes of CCP = 16 NG (16, 32 or 64).
//      stage 0  the tile's neighbour table in LDS: per (query, column) the
//               checked index (24 bits), the row flag (bit 24) and s_j - q;
//               pads (index outside [0, m), columns past k, queries past n)
//               are -1 and nothing of theirs is read.
//      stage 1  per query (4 per wave) KF = h^T F on v_mfma_f32_16x16x4_f32:
//               A[e][j] = h (kernel point e = lane & 15, neighbour
//               4 step + (lane >> 4)), B[j][c] = the neighbour's feature row
//               (channel lane & 15 of each of the NG 16-channel groups, read
//               from global memory: 64-byte segments, the gather itself).  One h
//               per lane and step serves the NG accumulators.  The (K x CCP)
//               block goes to LDS as row q of the tile's (16 x K CCP) image.
//      stage 2  out_tile += KF W on the same instruction: A[q][r] from LDS
//               (row stride = 4 mod 32 words: the 16 x 4 operand reads hit 64
//               different banks), B[r][o] = W[e][c][o] streamed from L2.  A
//               wave owns output tiles w, w + 4, ... of 16 channels; when the
//               block has fewer than three of them the waves split the K CCP
//               rows instead (steps t = slice mod S), so the 32-channel layers
//               keep four waves busy.  Accumulators live through every pass.
//      epilogue the slices' tiles meet in LDS and are added in slice order,
//               divided by max(1, count) and stored, rows coalesced.
//    No atomics; the order of every sum depends on the sizes only.
//  * neighbor_max: one wave per query row, the row's checked indices in LDS,
//    lanes over channels.
#include "pcr_internal.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kTq = 16;          // queries per workgroup
constexpr int kThreads = 256;
constexpr int kOTile = 256;      // output channels per workgroup at most (4 waves x 4 tiles x 16)
constexpr int kMaxKp = 16;
constexpr int kMaxNb = 256;
constexpr int kMaxCh = 2048;
constexpr int kMaxPoolCh = 4096;
constexpr int kMaxRows = 1 << 24;
constexpr int kLdsTarget = 78 * 1024;   // two workgroups per CU: the pass is narrowed to stay below
constexpr int kLdsMax = 96 * 1024;      // k = 256 with K = 16 needs 80.3 KiB at the narrowest pass
constexpr int kRedFloats = kTq * kOTile;
constexpr int kPad = -1;
constexpr int kFlagBit = 1 << 24;
constexpr int kIdxMask = kFlagBit - 1;

struct ConvArgs {
    const float *q, *s, *f, *kp, *w;
    const void *inds;
    const unsigned char *flags;
    float *out;
    float extent;
    int n, m, k, K, cin, cout, wide, constant;
    int kpad, ldk;   // table columns (k rounded up to 4), LDS row stride of the KF image
    int otile;       // output channels per workgroup: 256, 64, 32 or 16
};

__device__ __forceinline__ long long load_index(const void *inds, int wide, size_t at) {
    return wide ? static_cast<const long long *>(inds)[at] : (long long)static_cast<const int *>(inds)[at];
}

__global__ __launch_bounds__(256) void kpconv_row_flags(const float *f, int m, int c, unsigned char *flags) {
    const int row = blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= m) return;
    const float *p = f + (size_t)row * c;
    float s = 0.0f;
    for (int ch = 0; ch < c; ++ch) s = s + p[ch];
    flags[row] = s > 0.0f ? 1 : 0;
}

template <int NG>
__global__ __launch_bounds__(kThreads) void kpconv_fwd(ConvArgs a) {
    constexpr int CCP = 16 * NG;
    constexpr int UN = NG == 4 ? 2 : 4;   // stage 1 steps in flight
    extern __shared__ __attribute__((aligned(16))) char dsm[];
    float4 *nb = reinterpret_cast<float4 *>(dsm);                       // [16][kpad]
    float *kf = reinterpret_cast<float *>(dsm + (size_t)kTq * a.kpad * sizeof(float4));  // [16][ldk] / red
    __shared__ int cnt_s[kTq], end_s[kTq];

    const int tid = threadIdx.x, l = tid & 63, wv = tid >> 6, lc = l & 15, lg = l >> 4;
    const int q0 = blockIdx.x * kTq, o0 = blockIdx.y * a.otile;
    const int n = a.n, m = a.m, k = a.k, K = a.K, cin = a.cin, cout = a.cout, kpad = a.kpad, ldk = a.ldk;

    // stage 0: the neighbour table
    for (int t = tid; t < kTq * kpad; t += kThreads) {
        const int q = t / kpad, j = t - q * kpad, gi = q0 + q;
        float4 en = make_float4(__int_as_float(kPad), 0.f, 0.f, 0.f);
        if (gi < n && j < k) {
            const long long v = load_index(a.inds, a.wide, (size_t)gi * k + j);
            if (v >= 0 && v < (long long)m) {
                const float *sp = a.s + (size_t)v * 3, *qp = a.q + (size_t)gi * 3;
                const int code = (int)v | (a.flags[v] ? kFlagBit : 0);
                en = make_float4(__int_as_float(code), sp[0] - qp[0], sp[1] - qp[1], sp[2] - qp[2]);
            }
        }
        nb[t] = en;
    }
    __syncthreads();
    // per query: the count of flagged real neighbours and one past the last real column
    for (int qq = 0; qq < 4; ++qq) {
        const int q = 4 * wv + qq;
        int cnt = 0, end = 0;
        for (int j0 = 0; j0 < kpad; j0 += 64) {
            const int j = j0 + l;
            const int code = j < kpad ? __float_as_int(nb[q * kpad + j].x) : kPad;
            const unsigned long long real = __ballot(code >= 0);
            cnt += __popcll(__ballot(code >= 0 && (code & kFlagBit)));
            if (real) end = j0 + 64 - __clzll(real);
        }
        if (l == 0) { cnt_s[q] = cnt; end_s[q] = end; }
    }
    __syncthreads();

    // the lane's kernel point (stage 1: e = lane & 15)
    float kx = 0.f, ky = 0.f, kz = 0.f;
    const bool e_ok = lc < K;
    if (e_ok) { kx = a.kp[lc * 3 + 0]; ky = a.kp[lc * 3 + 1]; kz = a.kp[lc * 3 + 2]; }

    // stage 2 work split
    const int ntile = (min(a.otile, cout - o0) + 15) >> 4;  // 1 .. 16
    const int S = ntile >= 3 ? 1 : 4 / ntile;               // K-slices: 1, 2 or 4
    const int wpt = 4 / S;                                   // waves across the tiles
    const int tile0 = wv % wpt, slice = wv / wpt;
    f32x4 acc2[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) acc2[u] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int c0 = 0; c0 < cin; c0 += CCP) {
        // stage 1
        for (int qq = 0; qq < 4; ++qq) {
            const int q = 4 * wv + qq;
            const float4 *nbq = nb + q * kpad;
            const int nst = (end_s[q] + 3) >> 2;
            f32x4 acc[NG];
#pragma unroll
            for (int g = 0; g < NG; ++g) acc[g] = f32x4{0.f, 0.f, 0.f, 0.f};
            // UN steps' gathers are issued before their MFMAs; the chain stays in column order
            for (int st = 0; st < nst; st += UN) {
                float h[UN], b[UN][NG];
#pragma unroll
                for (int x = 0; x < UN; ++x) {
                    const float4 en = st + x < nst ? nbq[4 * (st + x) + lg] : make_float4(__int_as_float(kPad), 0.f, 0.f, 0.f);
                    const int code = __float_as_int(en.x);
                    const bool real = code >= 0;
                    h[x] = 0.0f;
                    if (real && e_ok) {
                        if (a.constant) {
                            h[x] = 1.0f;
                        } else {
                            const float dx = en.y - kx, dy = en.z - ky, dz = en.w - kz;
                            const float d2 = ((dx * dx + dy * dy) + dz * dz) + 1e-8f;
                            h[x] = fmaxf(1.0f - sqrtf(d2) / a.extent, 0.0f);
                        }
                    }
                    const float *frow = a.f + (size_t)(code & kIdxMask) * cin + c0 + lc;
#pragma unroll
                    for (int g = 0; g < NG; ++g) b[x][g] = (real && c0 + 16 * g + lc < cin) ? frow[16 * g] : 0.0f;
                }
#pragma unroll
                for (int x = 0; x < UN; ++x)
                    if (st + x < nst)
#pragma unroll
                        for (int g = 0; g < NG; ++g)
                            acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(h[x], b[x][g], acc[g], 0, 0, 0);
            }
            // D: column c = lane & 15, row e = 4 (lane >> 4) + r
#pragma unroll
            for (int g = 0; g < NG; ++g)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int e = 4 * lg + r;
                    if (e < K) kf[q * ldk + e * CCP + 16 * g + lc] = acc[g][r];
                }
        }
        __syncthreads();
        // stage 2: rows r = e CCP + c of this pass against W[e][c0 + c][o]
        // step t = (e, cs): rows e CCP + 4 cs .. + 3; only the groups of four that hold a channel below C_in
        const int cleft = cin - c0, cw4 = (min(CCP, cleft) + 3) >> 2, nT = K * cw4;
        const int inv = 65536 / cw4 + 1;   // t / cw4 = t inv >> 16 for t < 256, cw4 <= 16
        const float *ka = kf + lc * ldk + lg;
        for (int tb = slice; tb < nT; tb += 4 * S) {   // four steps' loads of W in flight
            float av[4], b[4][4];
#pragma unroll
            for (int x = 0; x < 4; ++x) {
                const int t = tb + x * S;
                const bool live = t < nT;   // a dead step multiplies 0 by 0
                const int tt = live ? t : 0, e = (tt * inv) >> 16, cs = tt - e * cw4, c = 4 * cs + lg;
                av[x] = live ? ka[e * CCP + 4 * cs] : 0.0f;
                const bool c_ok = live && c < cleft;
                const float *wrow = a.w + ((size_t)e * cin + (c0 + c)) * cout + o0 + lc;
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int tile = tile0 + wpt * u;
                    b[x][u] = (c_ok && tile < ntile && o0 + 16 * tile + lc < cout) ? wrow[16 * tile] : 0.0f;
                }
            }
#pragma unroll
            for (int x = 0; x < 4; ++x)
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (tile0 + wpt * u < ntile)
                        acc2[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[x], b[x][u], acc2[u], 0, 0, 0);
        }
        __syncthreads();   // the pass's readers are done: stage 1 (or the epilogue) may write
    }

    // epilogue: red[slice][q][col] over the KF image; D: column o = lane & 15, row q = 4 (lane >> 4) + r
    const int ncols = ntile * 16;
    float *red = kf;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int tile = tile0 + wpt * u;
        if (tile < ntile)
#pragma unroll
            for (int r = 0; r < 4; ++r) red[(slice * kTq + 4 * lg + r) * ncols + 16 * tile + lc] = acc2[u][r];
    }
    __syncthreads();
    for (int t = tid; t < kTq * ncols; t += kThreads) {
        const int q = t / ncols, col = t - q * ncols, gi = q0 + q, o = o0 + col;
        float s = red[q * ncols + col];
        for (int sl = 1; sl < S; ++sl) s = s + red[(sl * kTq + q) * ncols + col];
        if (gi < n && o < cout) a.out[(size_t)gi * cout + o] = s / (float)max(1, cnt_s[q]);
    }
}

// one wave per query row; 4 rows per workgroup
__global__ __launch_bounds__(256) void neighbor_max(const float *feats, const void *inds, int wide, int n, int m,
                                                    int k, int c, float *out) {
    __shared__ int row_s[4][kMaxNb];
    const int l = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int i = blockIdx.x * 4 + wv;
    int *row = row_s[wv];
    if (i < n)
        for (int j = l; j < k; j += 64) {
            const long long v = load_index(inds, wide, (size_t)i * k + j);
            row[j] = (v >= 0 && v < (long long)m) ? (int)v : kPad;
        }
    __syncthreads();
    if (i >= n) return;
    for (int ch = l; ch < c; ch += 64) {
        float best = 0.0f;
        for (int j = 0; j < k; ++j) {
            const int v = row[j];
            const float x = v >= 0 ? feats[(size_t)v * c + ch] : 0.0f;
            best = (j == 0 || x > best) ? x : best;
        }
        out[(size_t)i * c + ch] = best;
    }
}

int check_index_args(const char *who, int width, int n, int m, int k) {
    PCR_REQUIRE(width == 4 || width == 8, PCR_ERR_ARG, "%s: index width %d (must be 4 or 8 bytes)", who, width);
    PCR_REQUIRE(n >= 0 && n <= kMaxRows, PCR_ERR_ARG, "%s: n=%d outside 0..%d", who, n, kMaxRows);
    PCR_REQUIRE(m >= 1 && m <= kMaxRows, PCR_ERR_ARG, "%s: m=%d outside 1..%d", who, m, kMaxRows);
    PCR_REQUIRE(k >= 1 && k <= kMaxNb, PCR_ERR_ARG, "%s: k=%d outside 1..%d", who, k, kMaxNb);
    return PCR_OK;
}

template <int NG>
int launch_conv(const ConvArgs &a, size_t lds, hipStream_t s) {
    static const hipError_t attr = hipFuncSetAttribute((const void *)kpconv_fwd<NG>,
                                                       hipFuncAttributeMaxDynamicSharedMemorySize, kLdsMax);
    PCR_HIP_CHECK(attr);
    const dim3 grid((unsigned)((a.n + kTq - 1) / kTq), (unsigned)((a.cout + a.otile - 1) / a.otile));
    hipLaunchKernelGGL(kpconv_fwd<NG>, grid, dim3(kThreads), lds, s, a);
    PCR_LAUNCH_CHECK();
    return PCR_OK;
}

// LDS bytes of a workgroup with NG channel groups per pass
size_t conv_lds(int kpad, int K, int ng, int *ldk) {
    *ldk = (K * 16 * ng + 31) / 32 * 32 + 4;
    const size_t image = (size_t)kTq * (*ldk);
    return (size_t)kTq * kpad * sizeof(float4) + sizeof(float) * (image > (size_t)kRedFloats ? image : kRedFloats);
}

}  // namespace

extern "C" int pcr_kpconv_forward(const float *q_pts, const float *s_pts, const float *s_feats,
                                  const void *neigh_inds, int32_t index_width, int32_t n, int32_t m, int32_t k,
                                  const float *kernel_points, const float *weights, int32_t K, int32_t c_in,
                                  int32_t c_out, float kp_extent, int32_t influence, void *row_flags, float *out,
                                  pcr_stream_t stream) {
    pcr::clear_error();
    int rc = check_index_args("kpconv_forward", index_width, n, m, k);
    if (rc != PCR_OK) return rc;
    PCR_REQUIRE(K >= 1 && K <= kMaxKp, PCR_ERR_ARG, "kpconv_forward: K=%d outside 1..%d", K, kMaxKp);
    PCR_REQUIRE(c_in >= 1 && c_in <= kMaxCh, PCR_ERR_ARG, "kpconv_forward: c_in=%d outside 1..%d", c_in, kMaxCh);
    PCR_REQUIRE(c_out >= 1 && c_out <= kMaxCh, PCR_ERR_ARG, "kpconv_forward: c_out=%d outside 1..%d", c_out,
                kMaxCh);
    PCR_REQUIRE(influence == PCR_KP_LINEAR || influence == PCR_KP_CONSTANT, PCR_ERR_ARG,
                "kpconv_forward: influence=%d (0 linear, 1 constant)", influence);
    PCR_REQUIRE(influence == PCR_KP_CONSTANT || kp_extent > 0.0f, PCR_ERR_ARG,
                "kpconv_forward: KP_extent=%g (must be > 0)", (double)kp_extent);
    if (n == 0) return PCR_OK;
    PCR_REQUIRE(q_pts && s_pts && s_feats && neigh_inds && kernel_points && weights && row_flags && out,
                PCR_ERR_ARG, "kpconv_forward: null pointer");
    hipStream_t s = pcr::as_stream(stream);
    ConvArgs a;
    a.q = q_pts; a.s = s_pts; a.f = s_feats; a.kp = kernel_points; a.w = weights; a.inds = neigh_inds;
    a.flags = static_cast<const unsigned char *>(row_flags); a.out = out; a.extent = kp_extent;
    a.n = n; a.m = m; a.k = k; a.K = K; a.cin = c_in; a.cout = c_out; a.wide = index_width == 8 ? 1 : 0;
    a.constant = influence == PCR_KP_CONSTANT ? 1 : 0;
    a.kpad = (k + 3) / 4 * 4;
    // the widest pass that keeps two workgroups on a CU
    int ng = c_in <= 16 ? 1 : c_in <= 32 ? 2 : 4;
    size_t lds = conv_lds(a.kpad, K, ng, &a.ldk);
    while (ng > 1 && lds > (size_t)kLdsTarget) { ng >>= 1; lds = conv_lds(a.kpad, K, ng, &a.ldk); }
    PCR_REQUIRE(lds <= (size_t)kLdsMax, PCR_ERR_ARG, "kpconv_forward: LDS plan of %zu bytes", lds);
    // a launch that leaves CUs idle takes narrower blocks of output channels (stage 1 is
    // repeated per block, stage 2 is what gets shared out); a function of the sizes only
    const int qtiles = (n + kTq - 1) / kTq;
    for (a.otile = kOTile; a.otile > 16 && qtiles * ((c_out + a.otile - 1) / a.otile) < pcr::kCUs;)
        a.otile = a.otile == kOTile ? 64 : a.otile / 2;
    hipLaunchKernelGGL(kpconv_row_flags, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, s, s_feats, m, c_in,
                       static_cast<unsigned char *>(row_flags));
    PCR_LAUNCH_CHECK();
    switch (ng) {
        case 1: return launch_conv<1>(a, lds, s);
        case 2: return launch_conv<2>(a, lds, s);
        default: return launch_conv<4>(a, lds, s);
    }
}

extern "C" int pcr_neighbor_max(const float *feats, const void *inds, int32_t index_width, int32_t n, int32_t m,
                                int32_t k, int32_t c, float *out, pcr_stream_t stream) {
    pcr::clear_error();
    int rc = check_index_args("neighbor_max", index_width, n, m, k);
    if (rc != PCR_OK) return rc;
    PCR_REQUIRE(c >= 1 && c <= kMaxPoolCh, PCR_ERR_ARG, "neighbor_max: c=%d outside 1..%d", c, kMaxPoolCh);
    if (n == 0) return PCR_OK;
    PCR_REQUIRE(feats && inds && out, PCR_ERR_ARG, "neighbor_max: null pointer");
    hipLaunchKernelGGL(neighbor_max, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, pcr::as_stream(stream), feats,
                       inds, index_width == 8 ? 1 : 0, n, m, k, c, out);
    PCR_LAUNCH_CHECK();
    return PCR_OK;
}
