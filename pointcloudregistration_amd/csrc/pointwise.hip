// The point-wise (kernel size 1) convolution family of ROPNet, fused for
// inference: a Conv1d weight times channel-major (B, C, N) clouds, GroupNorm over
// (cloud, channel group, all points), the per-channel and per-cloud bias, the
// (Leaky)ReLU, the residual add behind it and the max over points
// (CG.py's PointNet, TFMR.py's OverlapAttentionBlock and conv_fuse).  The operand
// column [src_0 - sub_0 | ... | src_4 - sub_4] is subtracted and concatenated
// while its tile is staged into LDS: no (B, sum c_s, N) tensor exists in global
// memory.  Contract and numerics: include/pcr_api.h; f64 restatement with the
// derived bounds: tests/pointwise_ref.py; measurements: DESIGN.md "Point-wise
// convolutions".
//
// Kernels.
//  pointwise_gemm   unary_gemm with the roles swapped: a workgroup owns 128 output
//                   channels x 64 points of one cloud, a wave 32 channels (two
//                   32x32 accumulators, the points' halves); W is the A operand.
//                   The inputs go by in chunks of 32: the next chunk's weights
//                   (128 x 32) and points (32 x 64, a row of X contiguous over
//                   points) are fetched into registers while the MFMAs run on
//                   this one's LDS image, tails +0.  The tile's y then goes
//                   through LDS channel-major: coalesced rows to out (without a
//                   norm finished there), and a thread per channel walks the
//                   points in order for the f64 partials and the tile's maximum.
//  pointwise_small  pass 1 for n <= 4 on the VALU: the same fmaf chain, so the same
//                   bytes; a workgroup owns 64 channels, a wave one point, the weights
//                   128 inputs at a time through LDS.
//  norm_finalize_groups  norm_finalize.h.
//  pointwise_apply  out = act(fmaf(y, A, Bc)) + res in place, a wave a channel's
//                   64 points; the tile's maximum.
//  pointwise_max    cmax[b][o] = the tiles' maxima in tile order from -inf.
// LDS: W tile 128 x 34 (the 32 lanes of a half read rows 34 words apart), X tile
// 32 x 96 (the half that reads input k + 1 sits 96 = 32 mod 64 banks on); the y
// tile (128 x 65) takes their place: 33280 bytes a workgroup.
#include <math.h>

#include "norm_finalize.h"
#include "pcr_internal.h"
#include "wave.h"
#include "workspace.h"

namespace {

using pcr::cdiv64;
using pcr::FinArgs;
using pcr::kFinRuns;
using pcr::kFinThreads;
using pcr::norm_finalize_groups;
using pcr::WsLayout;
using pcr::f32x16;
using pcr::tile_row;

constexpr int kThreads = 256;
constexpr int kTile = 64;         // points per tile: the statistics' tile
constexpr int kChan = 128;        // output channels per workgroup, 32 per wave
constexpr int kChunk = 32;        // inputs staged at a time
constexpr int kWLd = kChunk + 2;  // weight tile's leading dimension
constexpr int kXLd = kTile + 32;  // point tile's
constexpr int kYLd = kTile + 1;   // y tile's
constexpr int kSrc = PCR_POINTWISE_MAX_SOURCES;
constexpr int kMaxN = 1 << 22;
constexpr int kMaxCin = 8192;
constexpr int kMaxCout = 2048;
constexpr int kMaxB = 65535;
constexpr int kXPer = kChunk * kTile / kThreads;  // 8 staged point elements per thread
constexpr int kSmallN = 4;                        // up to here pass 1 runs on the VALU (pointwise_small)
constexpr int kSmallO = 64;                       // its output channels per workgroup
constexpr int kSmallK = 128;                      // its inputs staged at a time
constexpr int kSmallLd = kSmallK + 1;
constexpr int kSmallWPer = kSmallO * kSmallK / kThreads;  // 32 staged weight elements per thread
constexpr int kWPer = kChan * kChunk / kThreads;  // 16 staged weight elements

struct Args {
    const float *src[kSrc], *sub[kSrc];
    long long sb[kSrc], sc[kSrc], ub[kSrc], uc[kSrc];  // batch and channel strides of src and sub
    int start[kSrc + 1];                               // first input of source s; start[nsrc] = cin
    const float *w, *bias, *cbias, *res, *coef;
    float *out, *y, *tmax;
    double *part;  // (b, tiles, cout, 2)
    long long rb, rc, ob, oc, wld;
    int nsrc, n, cin, cout, tiles;
    int norm, act, want_max;
    float slope;
};

// input k of point i of cloud b; the caller has checked k < cin and i < n
__device__ __forceinline__ float operand(const Args &a, int b, int k, int i) {
    int s = 0;
    while (s + 1 < a.nsrc && k >= a.start[s + 1]) ++s;
    const int c = k - a.start[s];
    const float v = a.src[s][b * a.sb[s] + c * a.sc[s] + i];
    return a.sub[s] ? __fsub_rn(v, a.sub[s][b * a.ub[s] + c * a.uc[s] + i]) : v;
}

__device__ __forceinline__ float activate(const Args &a, float pre, int b, int o, int i) {
    float z = a.act ? (pre > 0.0f ? pre : __fmul_rn(a.slope, pre)) : pre;
    if (a.res) z = __fadd_rn(z, a.res[b * a.rb + o * a.rc + i]);
    return z;
}

// grid (tiles, ceil(cout / 128), b)
__global__ __launch_bounds__(kThreads) void pointwise_gemm(Args a) {
    __shared__ __attribute__((aligned(16))) float lds[kChan * kYLd];
    float *Ws = lds, *Xs = lds + kChan * kWLd;  // 128 x 34 and 32 x 96, then Ys 128 x 65 over both

    const int tid = threadIdx.x, l = tid & 63, hh = l >> 5, lr = l & 31;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i0 = blockIdx.x * kTile, o0 = blockIdx.y * kChan, b = blockIdx.z;
    const int cin = a.cin, cout = a.cout;
    const int pts = min(kTile, a.n - i0);

    // weights: thread (col, q) holds column col of the chunk, rows q + 8 j; points: thread (l, wid) holds
    // point l of the tile, inputs wid + 4 j
    const int col = tid & 31, q = tid >> 5;
    const int omax = cout - 1 - o0;  // the workgroup's last weight row that exists (>= 0)
    const int wld = (int)a.wld;
    const bool pin = l < pts;
    float xr[kXPer], wr[kWPer];
    auto fetch = [&](int k0) {
        // a chunk that lies whole inside one source goes through one uniform base; the chunk with a seam
        // or the tail takes the checked path element by element
        int s = -1;
        for (int t = 0; t < a.nsrc; ++t)
            if (k0 >= a.start[t] && k0 + kChunk <= a.start[t + 1]) s = t;
        if (s >= 0) {
            const long long cs = a.sc[s];
            const float *p = a.src[s] + b * a.sb[s] + (k0 - a.start[s] + wid) * cs + i0 + l;
            if (a.sub[s]) {
                const long long cu = a.uc[s];
                const float *u = a.sub[s] + b * a.ub[s] + (k0 - a.start[s] + wid) * cu + i0 + l;
#pragma unroll
                for (int j = 0; j < kXPer; ++j) xr[j] = pin ? __fsub_rn(p[4 * j * cs], u[4 * j * cu]) : 0.0f;
            } else {
#pragma unroll
                for (int j = 0; j < kXPer; ++j) xr[j] = pin ? p[4 * j * cs] : 0.0f;
            }
        } else {
#pragma unroll
            for (int j = 0; j < kXPer; ++j) {
                const int k = k0 + wid + 4 * j;
                xr[j] = pin && k < cin ? operand(a, b, k, i0 + l) : 0.0f;
            }
        }
        const int k = k0 + col;
        if (k0 + kChunk <= cin) {
            const float *wb = a.w + (size_t)o0 * a.wld + k0;  // uniform; the offsets stay below 128 * 8192
#pragma unroll
            for (int j = 0; j < kWPer; ++j) {  // a row past cout: the last row's address, +0 staged
                const int r = q + 8 * j;
                const float v = wb[(unsigned)(min(r, omax) * wld + col)];
                wr[j] = r <= omax ? v : 0.0f;
            }
        } else {
#pragma unroll
            for (int j = 0; j < kWPer; ++j) {
                const int o = o0 + q + 8 * j;
                wr[j] = o < cout && k < cin ? a.w[(size_t)o * a.wld + k] : 0.0f;
            }
        }
    };

    f32x16 acc[2];
#pragma unroll
    for (int pt = 0; pt < 2; ++pt)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[pt][r] = 0.0f;
    const bool live = o0 + wid * 32 < cout;  // wave-uniform: a wave whose channels are all past cout only stages

    fetch(0);
    for (int k0 = 0; k0 < cin; k0 += kChunk) {
#pragma unroll
        for (int j = 0; j < kWPer; ++j) Ws[(q + 8 * j) * kWLd + col] = wr[j];
#pragma unroll
        for (int j = 0; j < kXPer; ++j) Xs[(wid + 4 * j) * kXLd + l] = xr[j];
        __syncthreads();
        if (k0 + kChunk < cin) fetch(k0 + kChunk);
        if (live) {
            const float *wp = Ws + (wid * 32 + lr) * kWLd + hh, *x0 = Xs + hh * kXLd + lr, *x1 = x0 + 32;
#pragma unroll
            for (int k = 0; k < kChunk; k += 2) {
                const float wv = wp[k];
                acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(wv, x0[k * kXLd], acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(wv, x1[k * kXLd], acc[1], 0, 0, 0);
            }
        }
        __syncthreads();  // every wave has read the chunk: the next one, or the y tile, takes its place
    }

    float *Ys = lds;
    if (live) {
#pragma unroll
        for (int pt = 0; pt < 2; ++pt)
#pragma unroll
            for (int r = 0; r < 16; ++r) Ys[(wid * 32 + tile_row(r, hh)) * kYLd + pt * 32 + lr] = acc[pt][r];
    }
    __syncthreads();

    const int nch = min(kChan, cout - o0);
    for (int e = tid; e < kChan * kTile; e += kThreads) {
        const int c = e >> 6, p = e & (kTile - 1), o = o0 + c, i = i0 + p;
        if (c < nch && p < pts) {
            float v = Ys[c * kYLd + p];
            if (a.y) a.y[((size_t)b * cout + o) * a.n + i] = v;
            if (a.bias) v = __fadd_rn(v, a.bias[o]);
            if (a.cbias) v = __fadd_rn(v, a.cbias[(size_t)b * cout + o]);
            if (!a.norm) v = activate(a, v, b, o, i);
            Ys[c * kYLd + p] = v;  // the statistics are of y with its biases, the maximum of the final values
            if (a.out) a.out[b * a.ob + o * a.oc + i] = v;
        }
    }
    __syncthreads();
    if (tid < nch) {  // points past the cloud's last take no part
        const size_t at = ((size_t)b * a.tiles + blockIdx.x) * cout + o0 + tid;
        if (a.norm) {
            double s = 0.0, ss = 0.0;
            for (int p = 0; p < pts; ++p) {
                const double d = (double)Ys[tid * kYLd + p];
                s += d;
                ss += d * d;
            }
            a.part[at * 2] = s;
            a.part[at * 2 + 1] = ss;
        } else if (a.want_max) {
            float m = -INFINITY;
            for (int p = 0; p < pts; ++p) m = fmaxf(m, Ys[tid * kYLd + p]);
            a.tmax[at] = m;
        }
    }
}

// n <= 4 (the CG's per-cloud products are n = 1): pass 1 on the VALU, the SAME chain -- fmaf(w, x, acc) over the
// inputs ascending from +0, the tail padded with +0 to the tile path's multiple of 32 -- so the bytes are the
// tile path's (test_pointwise_gpu compares them).  A workgroup owns 64 output channels of one cloud, wave p the
// point p; the weights go by 128 inputs at a time through LDS (rows 129 apart: a lane per channel reads
// conflict-free), the next chunk in registers meanwhile.  grid (ceil(cout / 64), b)
__global__ __launch_bounds__(kThreads) void pointwise_small(Args a) {
    __shared__ float Ws[kSmallO * kSmallLd];
    __shared__ float Xs[kSmallN * kSmallK];
    const int tid = threadIdx.x, ol = tid & 63, p = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int o0 = blockIdx.x * kSmallO, b = blockIdx.y, o = o0 + ol;
    const int cin = a.cin, cout = a.cout, n = a.n;
    const int col = tid & (kSmallK - 1), r0 = tid >> 7;  // weights: column col of the chunk, rows r0 + 2 j
    float wr[kSmallWPer], xr[2];
    auto fetch = [&](int k0) {
        const int k = k0 + col;
#pragma unroll
        for (int j = 0; j < kSmallWPer; ++j) {
            const int oo = o0 + r0 + 2 * j;
            wr[j] = oo < cout && k < cin ? a.w[(size_t)oo * a.wld + k] : 0.0f;
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {  // element e of the 4 x 128 point tile: point e / 128, input e % 128
            const int e = tid + kThreads * j, pe = e >> 7, ke = k0 + (e & (kSmallK - 1));
            xr[j] = pe < n && ke < cin ? operand(a, b, ke, pe) : 0.0f;
        }
    };
    float acc = 0.0f;
    fetch(0);
    for (int k0 = 0; k0 < cin; k0 += kSmallK) {
#pragma unroll
        for (int j = 0; j < kSmallWPer; ++j) Ws[(r0 + 2 * j) * kSmallLd + col] = wr[j];
#pragma unroll
        for (int j = 0; j < 2; ++j) Xs[tid + kThreads * j] = xr[j];
        __syncthreads();
        if (k0 + kSmallK < cin) fetch(k0 + kSmallK);
        if (p < n) {
            const int kend = min(kSmallK, (cin - k0 + kChunk - 1) / kChunk * kChunk);  // the tile path's padding
            const float *wp = Ws + ol * kSmallLd, *xp = Xs + p * kSmallK;
            for (int k = 0; k < kend; ++k) acc = fmaf(wp[k], xp[k], acc);
        }
        __syncthreads();
    }
    float *Vs = Xs;  // the points' values of each channel: [p][channel]
    if (p < n && o < cout) {
        float v = acc;
        if (a.y) a.y[((size_t)b * cout + o) * n + p] = v;
        if (a.bias) v = __fadd_rn(v, a.bias[o]);
        if (a.cbias) v = __fadd_rn(v, a.cbias[(size_t)b * cout + o]);
        if (!a.norm) v = activate(a, v, b, o, p);
        if (a.out) a.out[b * a.ob + o * a.oc + p] = v;
        Vs[p * kSmallO + ol] = v;
    }
    __syncthreads();
    if (p == 0 && o < cout) {
        const size_t at = (size_t)b * cout + o;  // one tile
        if (a.norm) {
            double s = 0.0, ss = 0.0;
            for (int q = 0; q < n; ++q) {
                const double d = (double)Vs[q * kSmallO + ol];
                s += d;
                ss += d * d;
            }
            a.part[at * 2] = s;
            a.part[at * 2 + 1] = ss;
        } else if (a.want_max) {
            float m = -INFINITY;
            for (int q = 0; q < n; ++q) m = fmaxf(m, Vs[q * kSmallO + ol]);
            a.tmax[at] = m;
        }
    }
}

// grid (tiles, ceil(cout / 128), b): wave w takes channels o0 + 32 w .., a lane one point of the tile
__global__ __launch_bounds__(kThreads) void pointwise_apply(Args a) {
    const int l = threadIdx.x & 63, wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int i = blockIdx.x * kTile + l, b = blockIdx.z;
    const int o1 = min(a.cout, (int)blockIdx.y * kChan + wid * 32 + 32);
    const bool pin = i < a.n;
    for (int o = blockIdx.y * kChan + wid * 32; o < o1; ++o) {
        const float *cf = a.coef + ((size_t)b * a.cout + o) * 2;
        float v = -INFINITY;
        if (pin) {
            float *at = a.out + b * a.ob + o * a.oc + i;
            v = activate(a, fmaf(*at, cf[0], cf[1]), b, o, i);
            *at = v;
        }
        if (a.want_max) {
            v = pcr::wave_max(v);
            if (l == 0) a.tmax[((size_t)b * a.tiles + blockIdx.x) * a.cout + o] = v;
        }
    }
}

// a thread per (cloud, channel): the tiles' maxima in tile order
__global__ __launch_bounds__(kThreads) void pointwise_max(const float *tmax, float *cmax, int b, int tiles, int cout) {
    const size_t at = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (at >= (size_t)b * cout) return;
    const size_t cl = at / cout, o = at - cl * cout;
    float m = -INFINITY;
    for (int t = 0; t < tiles; ++t) m = fmaxf(m, tmax[(cl * tiles + t) * cout + o]);
    cmax[at] = m;
}

int sizes_check(const char *who, int b, int n, int cout) {
    PCR_REQUIRE(b >= 0 && b <= kMaxB, PCR_ERR_ARG, "%s: b=%d outside 0..%d", who, b, kMaxB);
    PCR_REQUIRE(n >= 0 && n <= kMaxN, PCR_ERR_ARG, "%s: n=%d outside 0..%d", who, n, kMaxN);
    PCR_REQUIRE(cout >= 1 && cout <= kMaxCout, PCR_ERR_ARG, "%s: cout=%d outside 1..%d", who, cout, kMaxCout);
    return PCR_OK;
}

struct Scratch { float *coef; double *part; };

// A | Bc (b, cout, 2); partials (b, ceil(n / 64), cout, 2) f64, whose place the tiles' maxima take once the
// partials are finalized (or, without a norm, from the start)
WsLayout layout(Scratch &s, int b, int n, int cout) {
    WsLayout l(16);
    l.take(s.coef, (size_t)b * cout * 2);
    l.take(s.part, (size_t)b * cdiv64(n, kTile) * cout * 2);
    return l;
}

}  // namespace

extern "C" int64_t pcr_pointwise_scratch_bytes(int32_t b, int32_t n, int32_t cout) {
    pcr::clear_error();
    if (sizes_check("pointwise_scratch_bytes", b, n, cout) != PCR_OK) return -1;
    Scratch s;
    const WsLayout l = layout(s, b, n, cout);
    if (!l.ok()) {
        pcr::set_error("pointwise_scratch_bytes: the size overflows");
        return -1;
    }
    return (int64_t)l.bytes();
}

extern "C" int pcr_pointwise_forward(const pcr_pointwise_args *u, void *scratch, pcr_stream_t stream) {
    pcr::clear_error();
    PCR_REQUIRE(u, PCR_ERR_ARG, "pointwise_forward: null args");
    const int b = u->b, n = u->n, cout = u->cout, gw = u->gw;
    int rc = sizes_check("pointwise_forward", b, n, cout);
    if (rc != PCR_OK) return rc;
    PCR_REQUIRE(u->nsrc >= 1 && u->nsrc <= kSrc, PCR_ERR_ARG, "pointwise_forward: nsrc=%d outside 1..%d", u->nsrc,
                kSrc);
    long long cin = 0;
    for (int s = 0; s < u->nsrc; ++s) {
        PCR_REQUIRE(u->c[s] >= 1 && u->c[s] <= kMaxCin, PCR_ERR_ARG, "pointwise_forward: source %d has c=%d outside 1..%d",
                    s, u->c[s], kMaxCin);
        cin += u->c[s];
    }
    PCR_REQUIRE(cin <= kMaxCin, PCR_ERR_ARG, "pointwise_forward: cin=%lld above %d", cin, kMaxCin);
    PCR_REQUIRE(gw >= 0 && (gw == 0 || cout % gw == 0), PCR_ERR_ARG,
                "pointwise_forward: gw=%d: the group width must divide cout=%d", gw, cout);
    PCR_REQUIRE(u->eps >= 0.0 && u->eps == u->eps, PCR_ERR_ARG, "pointwise_forward: eps=%g must be >= 0", u->eps);
    PCR_REQUIRE(u->slope >= -1.0f && u->slope <= 1.0f, PCR_ERR_ARG, "pointwise_forward: slope=%g outside -1..1",
                (double)u->slope);
    PCR_REQUIRE(gw || !(u->gamma || u->beta || u->stats), PCR_ERR_ARG,
                "pointwise_forward: gamma, beta or stats without a norm");
    if (b == 0 || n == 0) return PCR_OK;
    PCR_REQUIRE(u->w && scratch, PCR_ERR_ARG, "pointwise_forward: null pointer (w and scratch are required)");
    PCR_REQUIRE(u->out || (u->cmax && !gw), PCR_ERR_ARG,
                "pointwise_forward: out is null (allowed only with cmax and without a norm)");
    Scratch sc;
    const WsLayout l = layout(sc, b, n, cout);
    PCR_REQUIRE(l.bind(scratch), PCR_ERR_ARG, "pointwise_forward: scratch is not 16-byte aligned");
    hipStream_t s = pcr::as_stream(stream);

    Args a;
    a.start[0] = 0;
    for (int t = 0; t < kSrc; ++t) {
        const bool in = t < u->nsrc;
        PCR_REQUIRE(!in || u->src[t], PCR_ERR_ARG, "pointwise_forward: source %d is null", t);
        a.src[t] = in ? u->src[t] : nullptr;
        a.sub[t] = in ? u->sub[t] : nullptr;
        a.sb[t] = in ? u->src_bs[t] : 0; a.sc[t] = in ? u->src_cs[t] : 0;
        a.ub[t] = in ? u->sub_bs[t] : 0; a.uc[t] = in ? u->sub_cs[t] : 0;
        a.start[t + 1] = a.start[t] + (in ? u->c[t] : 0);
    }
    a.w = u->w; a.bias = u->bias; a.cbias = u->cbias; a.res = u->res; a.coef = sc.coef;
    a.out = u->out; a.y = u->y; a.tmax = reinterpret_cast<float *>(sc.part); a.part = sc.part;
    PCR_REQUIRE(u->w_ld >= cin && u->w_ld <= kMaxCin, PCR_ERR_ARG,
                "pointwise_forward: w_ld=%lld outside cin=%lld..%d", (long long)u->w_ld, cin, kMaxCin);
    a.wld = u->w_ld;
    a.rb = u->res_bs; a.rc = u->res_cs; a.ob = u->out_bs; a.oc = u->out_cs;
    a.nsrc = u->nsrc; a.n = n; a.cin = (int)cin; a.cout = cout; a.tiles = (int)cdiv64(n, kTile);
    a.norm = gw ? 1 : 0; a.act = u->act ? 1 : 0; a.want_max = u->cmax ? 1 : 0; a.slope = u->slope;
    const dim3 grid((unsigned)a.tiles, (unsigned)cdiv64(cout, kChan), (unsigned)b);

    if (n <= kSmallN)
        hipLaunchKernelGGL(pointwise_small, dim3((unsigned)cdiv64(cout, kSmallO), (unsigned)b), dim3(kThreads), 0, s, a);
    else
        hipLaunchKernelGGL(pointwise_gemm, grid, dim3(kThreads), 0, s, a);
    PCR_LAUNCH_CHECK();
    if (gw) {
        FinArgs f;
        f.part = sc.part; f.gamma = u->gamma; f.beta = u->beta; f.coef = sc.coef; f.stats = u->stats;
        f.count = (double)n; f.eps = u->eps; f.tiles = a.tiles; f.C = cout; f.g = gw;
        hipLaunchKernelGGL(norm_finalize_groups, dim3((unsigned)(cout / gw), (unsigned)b), dim3(kFinThreads * kFinRuns),
                           0, s, f);
        PCR_LAUNCH_CHECK();
        hipLaunchKernelGGL(pointwise_apply, grid, dim3(kThreads), 0, s, a);
        PCR_LAUNCH_CHECK();
    }
    if (u->cmax) {
        hipLaunchKernelGGL(pointwise_max, dim3((unsigned)cdiv64((long long)b * cout, kThreads)), dim3(kThreads), 0, s,
                           a.tmax, u->cmax, b, a.tiles, cout);
        PCR_LAUNCH_CHECK();
    }
    return PCR_OK;
}
