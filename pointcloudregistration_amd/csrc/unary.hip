// The unary family of NgeNet's KPConv blocks and decoder, fused for inference:
// rows times an nn.Linear weight, InstanceNorm over the whole stacked cloud, the
// residual add and the LeakyReLU (UnaryBlock, BatchNormBlock, the add of
// ResnetBottleneckBlock, NearestUpsampleBlock + cat + UnaryBlock).  The operand
// row [x0[g0[i]] | x1[i]] is gathered and concatenated while its tile is staged
// into LDS: no (n, c0 + c1) or (n, c0) tensor exists in global memory.
// Contract and numerics: include/pcr_api.h; f64 restatement with the derived
// bounds: tests/unary_ref.py; the passes' bytes: DESIGN.md "Unary blocks".
//
// Kernels.
//  unary_gemm     a workgroup owns 64 rows x 128 output channels, a wave one
//                 block of 32 channels (two 32x32 accumulators, the rows' halves).
//                 The inputs go by in chunks of 32: the next chunk's rows (64 x 32)
//                 and weight rows (128 x 32) are fetched into registers while the
//                 MFMAs run on this one's LDS image, tails zero-filled, so c0 + c1
//                 and cout need be multiples of nothing and no row need be aligned.
//                 The tile's y then goes through LDS row-major: coalesced rows to
//                 out (with norm = 0 finished there), and a thread per channel
//                 walks the rows in order for the f64 partials.
//  unary_rows     w = NULL: a thread per channel walks a tile's rows where they are.
//  norm_finalize  norm_finalize.h, the rule pcr_group_mlp uses.
//  unary_apply    out = act(fmaf(y, a, b) + res) element by element, y read from out
//                 (or, w = NULL, from the rows).
// LDS: both staged tiles have leading dimension 34: the 32 lanes of a half read
// rows 34 words apart, 32 distinct even banks, the other half the odd ones.  The
// y tile (64 x 136, the two lane halves' rows 4 x 136 = 32 banks apart) takes the
// staging tiles' place: 34 KiB a workgroup; its 244 registers a lane allow two to a CU.
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
using pcr::norm_finalize;
using pcr::WsLayout;
using pcr::f32x16;
using pcr::tile_row;

constexpr int kThreads = 256;
constexpr int kTile = 64;        // rows per tile: the statistics' tile
constexpr int kChan = 128;       // output channels per workgroup, 32 per wave
constexpr int kChunk = 32;       // inputs staged at a time
constexpr int kLd = kChunk + 2;  // staged tiles' leading dimension
constexpr int kYLd = kChan + 8;  // y tile's
constexpr int kMaxN = 1 << 22;
constexpr int kMaxCin = 2048;
constexpr int kMaxCout = 1024;
constexpr int kXPer = kTile * kChunk / kThreads;  // 8 staged row elements per thread
constexpr int kWPer = kChan * kChunk / kThreads;  // 16 staged weight elements

struct Args {
    const float *x0, *x1, *w, *bias, *res, *coef;
    const int32_t *g0;
    float *out, *y;
    double *part;  // (tiles, cout, 2)
    long long ld0, ld1;
    int n, m0, c0, c1, cout;
    int norm, act;
    float slope;
};

// the x0 row of output row i, or -1 for a row of zeros
__device__ __forceinline__ long long source_row(const Args &a, int i) {
    if (i >= a.n) return -1;
    if (!a.g0) return i;
    const int g = a.g0[i];
    return g >= 0 && g < a.m0 ? g : -1;
}

// element k of output row i's operand row, whose x0 row is g
__device__ __forceinline__ float row_elem(const Args &a, int i, long long g, int k) {
    if (k < a.c0) return g >= 0 ? a.x0[g * a.ld0 + k] : 0.0f;
    if (k < a.c0 + a.c1 && i < a.n) return a.x1[i * a.ld1 + (k - a.c0)];
    return 0.0f;
}

__device__ __forceinline__ float finish(const Args &a, float v, size_t at, int o) {
    if (a.norm) v = fmaf(v, a.coef[2 * o], a.coef[2 * o + 1]);
    else if (a.bias) v = __fadd_rn(v, a.bias[o]);
    if (a.res) v = __fadd_rn(v, a.res[at]);
    if (a.act) v = v > 0.0f ? v : __fmul_rn(a.slope, v);
    return v;
}

__global__ __launch_bounds__(kThreads) void unary_gemm(Args a) {
    __shared__ __attribute__((aligned(16))) float lds[kTile * kYLd];
    __shared__ long long gs[kTile];
    float *Xs = lds, *Ws = lds + kTile * kLd;  // 64 x 34 and 128 x 34, then Ys 64 x 136 over both

    const int tid = threadIdx.x, l = tid & 63, hh = l >> 5, lr = l & 31;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int row0 = blockIdx.x * kTile, o0 = blockIdx.y * kChan;
    const int kdim = a.c0 + a.c1, cout = a.cout;
    const int rows = min(kTile, a.n - row0);

    if (tid < kTile) gs[tid] = source_row(a, row0 + tid);
    __syncthreads();

    // thread (col, q): column col of the chunk, rows q + 8 j of either tile
    const int col = tid & 31, q = tid >> 5;
    // A chunk that lies whole inside x0, inside x1 or inside the weight rows is fetched through row
    // pointers made once (null: a row of zeros) and a 32-bit offset from a uniform base; only the chunk
    // with the seam or a tail takes the checked path element by element (the address arithmetic of that
    // path on every chunk cost as much as the chunk's MFMAs)
    long long grow[kXPer];
    const float *p0[kXPer], *p1[kXPer];
#pragma unroll
    for (int j = 0; j < kXPer; ++j) {
        const int i = row0 + q + 8 * j;
        grow[j] = gs[q + 8 * j];
        p0[j] = grow[j] >= 0 ? a.x0 + grow[j] * a.ld0 + col : nullptr;
        p1[j] = a.x1 && i < a.n ? a.x1 + i * a.ld1 + col : nullptr;
    }
    const int omax = cout - 1 - o0;  // the workgroup's last weight row that exists (>= 0)
    float xr[kXPer], wr[kWPer];
    auto fetch = [&](int k0) {
        const int k = k0 + col;
        if (k0 + kChunk <= a.c0) {
#pragma unroll
            for (int j = 0; j < kXPer; ++j) xr[j] = p0[j] ? p0[j][k0] : 0.0f;
        } else if (k0 >= a.c0 && k0 + kChunk <= kdim) {
#pragma unroll
            for (int j = 0; j < kXPer; ++j) xr[j] = p1[j] ? p1[j][k0 - a.c0] : 0.0f;
        } else {
#pragma unroll
            for (int j = 0; j < kXPer; ++j) xr[j] = row_elem(a, row0 + q + 8 * j, grow[j], k);
        }
        if (k0 + kChunk <= kdim) {
            const float *wb = a.w + (size_t)o0 * kdim + k0;  // uniform; the offsets stay below 128 * 2048
#pragma unroll
            for (int j = 0; j < kWPer; ++j) {  // a row past cout: the last row's address, +0 staged
                const int r = q + 8 * j;
                const float v = wb[(unsigned)(min(r, omax) * kdim + col)];
                wr[j] = r <= omax ? v : 0.0f;
            }
        } else {
#pragma unroll
            for (int j = 0; j < kWPer; ++j) {
                const int o = o0 + q + 8 * j;
                wr[j] = o < cout && k < kdim ? a.w[(size_t)o * kdim + k] : 0.0f;
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
    for (int k0 = 0; k0 < kdim; k0 += kChunk) {
#pragma unroll
        for (int j = 0; j < kXPer; ++j) Xs[(q + 8 * j) * kLd + col] = xr[j];
#pragma unroll
        for (int j = 0; j < kWPer; ++j) Ws[(q + 8 * j) * kLd + col] = wr[j];
        __syncthreads();
        if (k0 + kChunk < kdim) fetch(k0 + kChunk);
        if (live) {
            const float *h0 = Xs + lr * kLd + hh, *h1 = h0 + 32 * kLd, *wp = Ws + (wid * 32 + lr) * kLd + hh;
#pragma unroll
            for (int k = 0; k < kChunk; k += 2) {
                const float b = wp[k];
                acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(h0[k], b, acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(h1[k], b, acc[1], 0, 0, 0);
            }
        }
        __syncthreads();  // every wave has read the chunk: the next one, or the y tile, takes its place
    }

    float *Ys = lds;
    if (live) {
#pragma unroll
        for (int pt = 0; pt < 2; ++pt)
#pragma unroll
            for (int r = 0; r < 16; ++r) Ys[(pt * 32 + tile_row(r, hh)) * kYLd + wid * 32 + lr] = acc[pt][r];
    }
    __syncthreads();

    const int nch = min(kChan, cout - o0);
    for (int i = tid; i < kTile * kChan; i += kThreads) {
        const int r = i >> 7, c = i & (kChan - 1);
        if (r < rows && c < nch) {
            const size_t at = (size_t)(row0 + r) * cout + o0 + c;
            float v = Ys[r * kYLd + c];
            if (a.y) a.y[at] = v;
            if (!a.norm) v = finish(a, v, at, o0 + c);
            a.out[at] = v;
        }
    }
    if (a.norm && tid < nch) {  // rows past the cloud's last take no part
        double s = 0.0, ss = 0.0;
        for (int r = 0; r < rows; ++r) {
            const double d = (double)Ys[r * kYLd + tid];
            s += d;
            ss += d * d;
        }
        double *p = a.part + ((size_t)blockIdx.x * cout + o0 + tid) * 2;
        p[0] = s;
        p[1] = ss;
    }
}

// w = NULL: the statistics (and the optional y) of the rows themselves; grid (tiles, ceil(cout / 256))
__global__ __launch_bounds__(kThreads) void unary_rows(Args a) {
    __shared__ long long gs[kTile];
    const int tid = threadIdx.x, row0 = blockIdx.x * kTile, c = blockIdx.y * kThreads + tid;
    const int rows = min(kTile, a.n - row0);
    if (tid < kTile) gs[tid] = source_row(a, row0 + tid);
    __syncthreads();
    if (c >= a.cout) return;
    double s = 0.0, ss = 0.0;
    for (int r = 0; r < rows; ++r) {
        const float v = row_elem(a, row0 + r, gs[r], c);
        if (a.y) a.y[(size_t)(row0 + r) * a.cout + c] = v;
        const double d = (double)v;
        s += d;
        ss += d * d;
    }
    if (a.norm) {
        double *p = a.part + ((size_t)blockIdx.x * a.cout + c) * 2;
        p[0] = s;
        p[1] = ss;
    }
}

// one element per thread; rows: y is read from the operand rows (w = NULL), else from out
__global__ __launch_bounds__(kThreads) void unary_apply(Args a, int from_rows) {
    const size_t at = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (at >= (size_t)a.n * a.cout) return;
    const int i = (int)(at / a.cout), o = (int)(at - (size_t)i * a.cout);
    const float v = from_rows ? row_elem(a, i, source_row(a, i), o) : a.out[at];
    a.out[at] = finish(a, v, at, o);
}

int sizes_check(const char *who, int n, int cout) {
    PCR_REQUIRE(n >= 0 && n <= kMaxN, PCR_ERR_ARG, "%s: n=%d outside 0..%d", who, n, kMaxN);
    PCR_REQUIRE(cout >= 1 && cout <= kMaxCout, PCR_ERR_ARG, "%s: cout=%d outside 1..%d", who, cout, kMaxCout);
    return PCR_OK;
}

struct Scratch { float *coef; double *part; };

// a | b (cout, 2); partials (ceil(n / 64), cout, 2) f64
WsLayout layout(Scratch &s, int n, int cout) {
    WsLayout l(16);
    l.take(s.coef, (size_t)cout * 2);
    l.take(s.part, (size_t)cdiv64(n, kTile) * cout * 2);
    return l;
}

}  // namespace

extern "C" int64_t pcr_unary_scratch_bytes(int32_t n, int32_t cout) {
    pcr::clear_error();
    if (sizes_check("unary_scratch_bytes", n, cout) != PCR_OK) return -1;
    Scratch s;
    const WsLayout l = layout(s, n, cout);
    if (!l.ok()) {
        pcr::set_error("unary_scratch_bytes: the size overflows");
        return -1;
    }
    return (int64_t)l.bytes();
}

extern "C" int pcr_unary_forward(const pcr_unary_args *u, void *scratch, pcr_stream_t stream) {
    pcr::clear_error();
    PCR_REQUIRE(u, PCR_ERR_ARG, "unary_forward: null args");
    const int n = u->n, cout = u->cout, kdim = u->c0 + u->c1;
    int rc = sizes_check("unary_forward", n, cout);
    if (rc != PCR_OK) return rc;
    PCR_REQUIRE(u->c0 >= 1 && u->c1 >= 0 && u->c0 <= kMaxCin && u->c1 <= kMaxCin && kdim <= kMaxCin, PCR_ERR_ARG,
                "unary_forward: c0=%d, c1=%d: c0 >= 1, c1 >= 0 and c0 + c1 <= %d", u->c0, u->c1, kMaxCin);
    PCR_REQUIRE(u->m0 >= 1 || n == 0, PCR_ERR_ARG, "unary_forward: m0=%d must be >= 1", u->m0);
    PCR_REQUIRE(!u->norm || n == 0 || n >= 2, PCR_ERR_ARG,
                "unary_forward: n=%d: the norm needs at least two rows", n);
    PCR_REQUIRE(u->eps >= 0.0 && u->eps == u->eps, PCR_ERR_ARG, "unary_forward: eps=%g must be >= 0", u->eps);
    PCR_REQUIRE(u->slope >= -1.0f && u->slope <= 1.0f, PCR_ERR_ARG, "unary_forward: slope=%g outside -1..1",
                (double)u->slope);
    PCR_REQUIRE(!(u->bias && u->norm), PCR_ERR_ARG, "unary_forward: bias together with norm");
    PCR_REQUIRE(!(u->stats && !u->norm), PCR_ERR_ARG, "unary_forward: stats without norm");
    PCR_REQUIRE(u->w || cout == kdim, PCR_ERR_ARG, "unary_forward: w is null and cout=%d is not c0 + c1 = %d", cout,
                kdim);
    PCR_REQUIRE(u->g0 || u->m0 == n || n == 0, PCR_ERR_ARG, "unary_forward: g0 is null and m0=%d is not n=%d", u->m0,
                n);
    PCR_REQUIRE(u->x1 || u->c1 == 0, PCR_ERR_ARG, "unary_forward: x1 is null and c1=%d", u->c1);
    PCR_REQUIRE(u->ld0 >= u->c0 && (u->c1 == 0 || u->ld1 >= u->c1), PCR_ERR_ARG,
                "unary_forward: ld0=%lld, ld1=%lld: a row stride below its width", (long long)u->ld0,
                (long long)u->ld1);
    if (n == 0) return PCR_OK;
    PCR_REQUIRE(u->x0 && u->out && scratch, PCR_ERR_ARG,
                "unary_forward: null pointer (x0, out and scratch are required)");
    Scratch sc;
    const WsLayout l = layout(sc, n, cout);
    PCR_REQUIRE(l.bind(scratch), PCR_ERR_ARG, "unary_forward: scratch is not 16-byte aligned");
    hipStream_t s = pcr::as_stream(stream);

    Args a;
    a.x0 = u->x0; a.x1 = u->c1 ? u->x1 : nullptr; a.w = u->w; a.bias = u->bias; a.res = u->res; a.coef = sc.coef;
    a.g0 = u->g0; a.out = u->out; a.y = u->y; a.part = sc.part;
    a.ld0 = u->ld0; a.ld1 = u->ld1;
    a.n = n; a.m0 = u->m0; a.c0 = u->c0; a.c1 = u->c1; a.cout = cout;
    a.norm = u->norm ? 1 : 0; a.act = u->act ? 1 : 0; a.slope = u->slope;
    const unsigned tiles = (unsigned)cdiv64(n, kTile);
    const unsigned blocks = (unsigned)cdiv64((long long)n * cout, kThreads);

    if (a.w) {
        hipLaunchKernelGGL(unary_gemm, dim3(tiles, (unsigned)cdiv64(cout, kChan)), dim3(kThreads), 0, s, a);
        PCR_LAUNCH_CHECK();
    } else if (a.norm || a.y) {
        hipLaunchKernelGGL(unary_rows, dim3(tiles, (unsigned)cdiv64(cout, kThreads)), dim3(kThreads), 0, s, a);
        PCR_LAUNCH_CHECK();
    }
    if (a.norm) {
        FinArgs f;
        f.part = sc.part; f.gamma = f.beta = nullptr; f.coef = sc.coef; f.stats = u->stats;
        f.count = (double)n; f.eps = u->eps; f.tiles = (int)tiles; f.C = cout; f.g = 1;
        hipLaunchKernelGGL(norm_finalize, dim3((unsigned)cdiv64(cout, kFinThreads)), dim3(kFinThreads * kFinRuns), 0, s,
                           f);
        PCR_LAUNCH_CHECK();
    }
    if (a.norm || !a.w) {
        hipLaunchKernelGGL(unary_apply, dim3(blocks), dim3(kThreads), 0, s, a, a.w ? 0 : 1);
        PCR_LAUNCH_CHECK();
    }
    return PCR_OK;
}
