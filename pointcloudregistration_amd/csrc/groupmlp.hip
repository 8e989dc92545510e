// The consumers of the grouping front ends, fused for inference: the edge conv
// of NgeNet's GCN (Conv2d(2C -> C') -> InstanceNorm2d -> LeakyReLU -> max over
// the k neighbours) and the grouped local-feature MLP behind NgeNet's PPF and
// ROPNet's LocalFeatue (up to three Conv2d 1x1 -> Instance/GroupNorm -> ReLU,
// then the max over the K group members).  No (B, N, k, 2C) or (B, C, K, N)
// tensor exists in global memory.  Contract and numerics: include/pcr_api.h;
// f64 restatement with the derived bounds: tests/groupmlp_ref.py.
//
// Both rest on two identities (DESIGN.md "Edge conv and grouped MLP"):
//  * y -> act(fmaf(y, a, b)) is monotone per channel, so the max over the
//    neighbours of the normalised, activated values is that map applied to the
//    max (a >= 0) or the min (a < 0) of the raw y: the last layer needs only
//    sum y and sum y^2 per channel and max / min per (point, channel);
//  * W [f_i ; f_j - f_i] = (Wa f_i - Wb f_i) + Wb f_j: the edge conv is one
//    per-point product and a gather-reduce over the neighbour rows.
//
// Kernels.
//  tile_gemm      (device) 64 rows of an LDS tile times weight rows streamed
//                 from L2, on v_mfma_f32_32x32x2_f32: a wave owns the channel
//                 blocks wid, wid + 4, ... (up to four, 128 accumulator
//                 registers), so a layer's whole 64 x 512 output is in
//                 registers before the tile it was computed from is overwritten.
//  group_mlp_tile one 64-row tile of one cloud through the first L layers
//                 (layer 1 on the VALU, its weights held in the lanes), the
//                 earlier layers normalised with finished coefficients; the
//                 L-th layer's raw y goes to LDS row-major, from where a thread
//                 per channel walks the rows in order: f64 sum and sum of
//                 squares to the tile's partial, max / min per group to scratch.
//  edge_gemm      R = P - Q and Q for 64 points and 128 channels per workgroup.
//  edge_reduce    per point and channel the kk neighbours in order.
//  norm_finalize  (norm_finalize.h, shared with unary.hip) per (cloud, channel):
//                 the partials in 16 runs of consecutive tiles,
//                 each in ascending order, the runs' sums in run order;
//                 mean / var / rstd in f64, a and b rounded once.
//  norm_output    out = act(fmaf(max or min, a, b)), either layout (the
//                 channel-major one through a 32 x 32 LDS transpose).
// LDS: the activation tile is row-major with leading dimension c + 2 (the A
// operand's 32 lanes of a half hit 32 banks, as in pointnet_heads); at c = 512
// that is 128.5 KiB + 4.25 KiB of inputs: one workgroup per CU, one wave per
// SIMD, kept busy by eight independent accumulators.
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
constexpr int kTile = 64;       // rows per tile
constexpr int kMaxC = 512;      // widest layer
constexpr int kMaxCin = 16;     // group channels
constexpr int kMaxK = 128;      // group members
constexpr int kMaxKK = 63;      // edge neighbours (pcr_knn_graph's limit)
constexpr int kMaxN = 1 << 20;  // norm_output: gridDim.y = n / 32
constexpr int kMaxB = 65535;    // gridDim.y
constexpr int kXLd = kMaxCin + 1;
constexpr int kWaveBlk = kMaxC / 32 / 4;  // channel blocks per wave
constexpr int kEdgePts = 8;     // points per edge_reduce workgroup: its statistics tile

__device__ __forceinline__ float act(float v, float slope) {
    return v > 0.0f ? v : (slope == 0.0f ? 0.0f : __fmul_rn(v, slope));
}

// the value lane `lane` (wave-uniform) holds
__device__ __forceinline__ float bcast(float v, int lane) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}

// acc[j] = the 64 rows of Hs (leading dimension ld, kdim columns) times the weight row rowp[j] of
// this lane's channel, j < nact (wave-uniform): per element one fmaf chain over k ascending from
// +0 (k-step t adds columns 2 t, then 2 t + 1).  A unit of work is one block j and one 128-byte
// line of its weight rows (32 columns, 8 float4 per lane): a line is consumed by the unit that
// fetched it, so the four waves' lines in flight (16 KiB) stay in L1, and the next unit's line
// is requested before this unit's 32 MFMAs.  kdim is a multiple of 32.
constexpr int kLine = 32;

__device__ __forceinline__ void load_line(float4 (&v)[kLine / 4], const float *p) {
#pragma unroll
    for (int q = 0; q < kLine / 4; ++q) v[q] = reinterpret_cast<const float4 *>(p)[q];
}

template <int NB>
__device__ __forceinline__ void tile_gemm(const float *Hs, int ld, const float *(&rowp)[NB], int nact,
                                          int kdim, int lr, int hh, f32x16 (&acc)[NB][2]) {
#pragma unroll
    for (int j = 0; j < NB; ++j)
#pragma unroll
        for (int pt = 0; pt < 2; ++pt)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[j][pt][r] = 0.0f;
    float4 nxt[kLine / 4];
#pragma unroll
    for (int q = 0; q < kLine / 4; ++q) nxt[q] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (nact > 0) load_line(nxt, rowp[0]);
    const float *h0 = Hs + lr * ld + hh, *h1 = h0 + 32 * ld;
#pragma unroll
    for (int j = 0; j < NB; ++j) {
        if (j >= nact) break;
        for (int k0 = 0; k0 < kdim; k0 += kLine) {
            float4 cur[kLine / 4];
#pragma unroll
            for (int q = 0; q < kLine / 4; ++q) cur[q] = nxt[q];
            if (k0 + kLine < kdim) load_line(nxt, rowp[j] + k0 + kLine);
            else if (j + 1 < NB && j + 1 < nact) load_line(nxt, rowp[j + 1 < NB ? j + 1 : j]);
#pragma unroll
            for (int q = 0; q < kLine / 4; ++q) {
                const int k = k0 + 4 * q;
                const float a00 = h0[k], a01 = h1[k], a10 = h0[k + 2], a11 = h1[k + 2];
                const float b0 = hh ? cur[q].y : cur[q].x, b1 = hh ? cur[q].w : cur[q].z;
                acc[j][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a00, b0, acc[j][0], 0, 0, 0);
                acc[j][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a01, b0, acc[j][1], 0, 0, 0);
                acc[j][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a10, b1, acc[j][0], 0, 0, 0);
                acc[j][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a11, b1, acc[j][1], 0, 0, 0);
            }
        }
    }
}

struct MlpArgs {
    const float *x;        // (b, n, K, cin)
    const float *w[3];     // (c_l, c_{l-1})
    const float *coef[3];  // (b, c_l, 2): a, b of the layers before the L-th
    int c[3];
    int cin, n, K, L;      // L: the layers this pass computes
    int final;             // the L-th layer is the net's last: keep max / min
    float slope;
    float *y;              // (b, n, K, c_L) pre-norm, or null
    double *part;          // (b, tiles, c_L, 2)
    float *mx, *mn;        // (b, n S, c_L)
    int tiles, ppt, S;     // tiles per cloud; points per tile (K <= 64); tiles per point (K > 64)
};

__global__ __launch_bounds__(kThreads) void group_mlp_tile(MlpArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float *Xs = lds;                 // kTile x kXLd
    float *Hs = lds + kTile * kXLd;  // kTile x (c + 2), one layer's tile at a time

    const int tid = threadIdx.x, l = tid & 63, hh = l >> 5, lr = l & 31;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int t = blockIdx.x, b = blockIdx.y;
    const int n = a.n, K = a.K, cin = a.cin, L = a.L;

    // the tile's rows of the cloud's (n K) list, and its max / min groups: a function of (n, K) only
    int row0, rows, seg, slot0;
    if (a.S == 1) {
        const int p0 = t * a.ppt, np = min(a.ppt, n - p0);
        row0 = p0 * K; rows = np * K; seg = K; slot0 = p0;
    } else {
        const int p = t / a.S, s = t - p * a.S;
        row0 = p * K + s * kTile; rows = min(kTile, K - s * kTile); seg = rows; slot0 = t;
    }
    const size_t grow0 = (size_t)b * n * K + row0;

    {   // a row past the tile's last is staged as +0 and kept out of every statistic below
        const float *xg = a.x + grow0 * cin;
        for (int i = tid; i < kTile * cin; i += kThreads) {
            const int r = i / cin, e = i - r * cin;
            Xs[r * kXLd + e] = r < rows ? xg[i] : 0.0f;
        }
    }
    __syncthreads();

    {   // layer 1 on the VALU: thread (wave w, row l) makes channels w c1 / 4 .. .  Lane i of the wave
        // holds the weights (and a, b) of the wave's channels i and 64 + i; a channel's are broadcast
        // by readlane: loads inside the channel loop ran one memory latency each, 28 us per tile
        float xr[kMaxCin];
#pragma unroll
        for (int e = 0; e < kMaxCin; ++e) xr[e] = e < cin ? Xs[l * kXLd + e] : 0.0f;
        const int c1 = a.c[0], per = c1 >> 2, ld = c1 + 2;
        const float *cf = a.coef[0] + (size_t)b * c1 * 2;
        float wreg[2][kMaxCin], ca[2] = {1.0f, 1.0f}, cb[2] = {0.0f, 0.0f};
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int c = wid * per + min(h * 64 + l, per - 1);  // a lane past the wave's channels repeats the last
            const float *wr = a.w[0] + (size_t)c * cin;
#pragma unroll
            for (int e = 0; e < kMaxCin; ++e) wreg[h][e] = wr[min(e, cin - 1)];
            if (L > 1) { ca[h] = cf[2 * c]; cb[h] = cf[2 * c + 1]; }
        }
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int cnt = min(64, per - h * 64);
            for (int cc = 0; cc < cnt; ++cc) {
                float y = 0.0f;
#pragma unroll
                for (int e = 0; e < kMaxCin; ++e)
                    if (e < cin) y = fmaf(bcast(wreg[h][e], cc), xr[e], y);
                if (L > 1) y = act(fmaf(y, bcast(ca[h], cc), bcast(cb[h], cc)), a.slope);
                Hs[l * ld + wid * per + h * 64 + cc] = y;
            }
        }
    }
    __syncthreads();

    for (int li = 1; li < L; ++li) {
        const int kdim = a.c[li - 1], co = a.c[li], nblk = co >> 5;
        const int nact = wid < nblk ? (nblk - wid + 3) >> 2 : 0;
        const float *rowp[kWaveBlk];
#pragma unroll
        for (int j = 0; j < kWaveBlk; ++j)
            rowp[j] = a.w[li] + (size_t)((j < nact ? wid + 4 * j : 0) * 32 + lr) * kdim;
        f32x16 acc[kWaveBlk][2];
        tile_gemm<kWaveBlk>(Hs, kdim + 2, rowp, nact, kdim, lr, hh, acc);
        __syncthreads();  // every wave has read the input tile: the output takes its place
        const bool last = li == L - 1;
        const int ld = co + 2;
        const float *cf = a.coef[li] + (size_t)b * co * 2;
#pragma unroll
        for (int j = 0; j < kWaveBlk; ++j)
            if (j < nact) {
                const int o = (wid + 4 * j) * 32 + lr;
                float ca = 1.0f, cb = 0.0f;
                if (!last) { ca = cf[2 * o]; cb = cf[2 * o + 1]; }
#pragma unroll
                for (int pt = 0; pt < 2; ++pt)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        float v = acc[j][pt][r];
                        if (!last) v = act(fmaf(v, ca, cb), a.slope);
                        Hs[(pt * 32 + tile_row(r, hh)) * ld + o] = v;
                    }
            }
        __syncthreads();
    }

    // Hs holds the L-th layer's raw y, row-major
    const int C = a.c[L - 1], ld = C + 2;
    if (a.y) {
        float *yg = a.y + grow0 * C;
        for (int i = tid; i < rows * C; i += kThreads) {
            const int r = i / C, c = i - r * C;
            yg[i] = Hs[r * ld + c];
        }
    }
    const int nseg = rows / seg;
    for (int c = tid; c < C; c += kThreads) {
        double s = 0.0, ss = 0.0;
        for (int q = 0; q < nseg; ++q) {
            float mx = -INFINITY, mn = INFINITY;
            for (int k = 0; k < seg; ++k) {
                const float v = Hs[(q * seg + k) * ld + c];
                const double d = (double)v;
                s += d;
                ss += d * d;
                mx = fmaxf(mx, v);
                mn = fminf(mn, v);
            }
            if (a.final) {
                const size_t at = ((size_t)b * n * a.S + slot0 + q) * C + c;
                a.mx[at] = mx;
                a.mn[at] = mn;
            }
        }
        double *p = a.part + (((size_t)b * a.tiles + t) * C + c) * 2;
        p[0] = s;
        p[1] = ss;
    }
}

struct EdgeArgs {
    const float *f; long long sb, sp, sc;  // element (batch, point, channel)
    const int32_t *idx;                    // (b, n, kk)
    const float *w;                        // (co, 2 c)
    float *rq;                             // (b, n, 2 co): R | Q
    float *mx, *mn;                        // (b, n, co)
    double *part;                          // (b, tiles, co, 2)
    int n, kk, c, co, tiles;
};

__global__ __launch_bounds__(kThreads) void edge_gemm(EdgeArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];  // kTile x (c + 2)
    const int tid = threadIdx.x, l = tid & 63, hh = l >> 5, lr = l & 31;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int p0 = blockIdx.x * kTile, b = blockIdx.y;
    const int n = a.n, c = a.c, co = a.co, ld = c + 2;
    const float *fb = a.f + b * a.sb;
    // a point past n repeats the last one and is not stored
    if (a.sc == 1) {
        for (int i = tid; i < kTile * c; i += kThreads) {
            const int r = i / c, e = i - r * c;
            lds[r * ld + e] = fb[min(p0 + r, n - 1) * a.sp + e];
        }
    } else {
        for (int i = tid; i < kTile * c; i += kThreads) {
            const int e = i >> 6, r = i & 63;
            lds[r * ld + e] = fb[min(p0 + r, n - 1) * a.sp + e * a.sc];
        }
    }
    __syncthreads();
    const int cb = blockIdx.z * 4 + wid;  // a wave's one channel block: P and Q, four accumulators
    if (cb < (co >> 5)) {
        const int o = cb * 32 + lr;
        const float *rowp[2];
        rowp[0] = a.w + (size_t)o * 2 * c;  // Wa
        rowp[1] = rowp[0] + c;              // Wb
        f32x16 acc[2][2];
        tile_gemm<2>(lds, ld, rowp, 2, c, lr, hh, acc);
#pragma unroll
        for (int pt = 0; pt < 2; ++pt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int p = p0 + pt * 32 + tile_row(r, hh);
                if (p < n) {
                    float *dst = a.rq + ((size_t)b * n + p) * 2 * co + o;
                    dst[0] = __fsub_rn(acc[0][pt][r], acc[1][pt][r]);
                    dst[co] = acc[1][pt][r];
                }
            }
    }
}

__global__ __launch_bounds__(kThreads) void edge_reduce(EdgeArgs a) {
    __shared__ int js[kEdgePts * kMaxKK];
    const int tid = threadIdx.x, t = blockIdx.x, b = blockIdx.y;
    const int n = a.n, kk = a.kk, co = a.co;
    const int p0 = t * kEdgePts, np = min(kEdgePts, n - p0);
    for (int i = tid; i < np * kk; i += kThreads)
        js[i] = min(max(a.idx[((size_t)b * n + p0) * kk + i], 0), n - 1);
    __syncthreads();
    const float *rq = a.rq + (size_t)b * n * 2 * co;
    for (int c = tid; c < co; c += kThreads) {
        double s = 0.0, ss = 0.0;
        for (int q = 0; q < np; ++q) {
            const float ri = rq[(size_t)(p0 + q) * 2 * co + c];
            float mx = -INFINITY, mn = INFINITY;
            for (int j = 0; j < kk; ++j) {
                const float y = __fadd_rn(ri, rq[(size_t)js[q * kk + j] * 2 * co + co + c]);
                const double d = (double)y;
                s += d;
                ss += d * d;
                mx = fmaxf(mx, y);
                mn = fminf(mn, y);
            }
            const size_t at = ((size_t)b * n + p0 + q) * co + c;
            a.mx[at] = mx;
            a.mn[at] = mn;
        }
        double *p = a.part + (((size_t)b * a.tiles + t) * co + c) * 2;
        p[0] = s;
        p[1] = ss;
    }
}

struct OutArgs {
    const float *mx, *mn;  // (b, n S, C)
    const float *coef;     // (b, C, 2)
    float *out;            // (b, n, C) or (b, C, n)
    int n, S, C, channels_first;
    float slope;
};

__global__ __launch_bounds__(kThreads) void norm_output(OutArgs a) {
    __shared__ float ts[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int c0 = blockIdx.x * 32, p0 = blockIdx.y * 32, b = blockIdx.z;
    const int n = a.n, C = a.C, S = a.S;
    {
        const int c = c0 + tx;
        const float ca = a.coef[((size_t)b * C + c) * 2], cb = a.coef[((size_t)b * C + c) * 2 + 1];
        const float *src = ca >= 0.0f ? a.mx : a.mn;
        for (int i = ty; i < 32; i += 8) {
            const int p = p0 + i;
            if (p >= n) break;
            const float *m = src + ((size_t)b * n + p) * S * C + c;
            float v = m[0];
            for (int s = 1; s < S; ++s) v = ca >= 0.0f ? fmaxf(v, m[(size_t)s * C]) : fminf(v, m[(size_t)s * C]);
            v = act(fmaf(v, ca, cb), a.slope);
            if (a.channels_first) ts[i][tx] = v;
            else a.out[((size_t)b * n + p) * C + c] = v;
        }
    }
    if (!a.channels_first) return;
    __syncthreads();
    const int p = p0 + tx;
    if (p < n)
        for (int i = ty; i < 32; i += 8) a.out[((size_t)b * C + c0 + i) * n + p] = ts[tx][i];
}

hipError_t lds_attr() {  // both MFMA kernels take their tile as dynamic LDS past the 64 KiB default
    static const hipError_t e = [] {
        const int most = (int)sizeof(float) * kTile * (kXLd + kMaxC + 2);
        hipError_t r = hipFuncSetAttribute((const void *)group_mlp_tile, hipFuncAttributeMaxDynamicSharedMemorySize, most);
        if (r != hipSuccess) return r;
        return hipFuncSetAttribute((const void *)edge_gemm, hipFuncAttributeMaxDynamicSharedMemorySize, most);
    }();
    return e;
}

bool width_ok(int c) { return c >= 32 && c <= kMaxC && (c & 31) == 0; }

int finalize_and_output(const FinArgs &f, const OutArgs *o, int b, hipStream_t s) {
    hipLaunchKernelGGL(norm_finalize, dim3((unsigned)cdiv64(f.C, kFinThreads), (unsigned)b), dim3(kFinThreads * kFinRuns), 0, s, f);
    PCR_LAUNCH_CHECK();
    if (o) {
        hipLaunchKernelGGL(norm_output, dim3((unsigned)(o->C / 32), (unsigned)cdiv64(o->n, 32), (unsigned)b),
                           dim3(kThreads), 0, s, *o);
        PCR_LAUNCH_CHECK();
    }
    return PCR_OK;
}

// ---- edge conv ------------------------------------------------------------------------------

int edge_check(const char *who, int b, int n, int kk, int c, int co) {
    PCR_REQUIRE(b >= 0 && b <= kMaxB, PCR_ERR_ARG, "%s: b=%d outside 0..%d", who, b, kMaxB);
    PCR_REQUIRE(n >= 2 && n <= kMaxN, PCR_ERR_ARG, "%s: n=%d outside 2..%d", who, n, kMaxN);
    PCR_REQUIRE(kk >= 1 && kk <= kMaxKK, PCR_ERR_ARG, "%s: kk=%d outside 1..%d", who, kk, kMaxKK);
    PCR_REQUIRE(width_ok(c) && width_ok(co), PCR_ERR_ARG,
                "%s: c=%d, co=%d: widths must be multiples of 32 in 32..%d", who, c, co, kMaxC);
    return PCR_OK;
}

struct EdgeScratch { float *rq, *mx, *mn, *coef; double *part; };

// R|Q (b, n, 2 co), max and min (b, n, co), a|b (b, co, 2), partials (b, ceil(n / 8), co, 2) f64: no term in kk
WsLayout edge_layout(EdgeScratch &e, int b, int n, int c, int co) {
    WsLayout l(16);
    const size_t pn = (size_t)b * n;
    l.take(e.rq, pn * 2 * co);
    l.take(e.mx, pn * co);
    l.take(e.mn, pn * co);
    l.take(e.coef, (size_t)b * co * 2);
    l.take(e.part, (size_t)b * cdiv64(n, kEdgePts) * co * 2);
    return l;
}

// ---- grouped MLP ----------------------------------------------------------------------------

struct Tiling { int tiles, ppt, S; };

Tiling tiling(int n, int K) {
    Tiling t;
    if (K <= kTile) { t.ppt = kTile / K; t.S = 1; t.tiles = (int)cdiv64(n, t.ppt); }
    else { t.ppt = 1; t.S = (int)cdiv64(K, kTile); t.tiles = n * t.S; }
    return t;
}

int mlp_check(const char *who, int b, int n, int K, int cin, int layers, const int *width) {
    PCR_REQUIRE(b >= 0 && b <= kMaxB, PCR_ERR_ARG, "%s: b=%d outside 0..%d", who, b, kMaxB);
    PCR_REQUIRE(n >= 2 && n <= kMaxN, PCR_ERR_ARG, "%s: n=%d outside 2..%d", who, n, kMaxN);
    PCR_REQUIRE(K >= 1 && K <= kMaxK, PCR_ERR_ARG, "%s: K=%d outside 1..%d", who, K, kMaxK);
    PCR_REQUIRE(cin >= 1 && cin <= kMaxCin, PCR_ERR_ARG, "%s: cin=%d outside 1..%d", who, cin, kMaxCin);
    PCR_REQUIRE(layers >= 1 && layers <= 3, PCR_ERR_ARG, "%s: layers=%d outside 1..3", who, layers);
    for (int i = 0; i < layers; ++i)
        PCR_REQUIRE(width_ok(width[i]), PCR_ERR_ARG, "%s: width %d of layer %d: widths must be multiples of 32 in 32..%d",
                    who, width[i], i + 1, kMaxC);
    return PCR_OK;
}

struct MlpScratch { float *coef[3], *mx, *mn; double *part; };

// a|b per layer (b, c_l, 2); max and min (b, n ceil(K / 64), c_L); partials (b, tiles, max c_l, 2) f64
WsLayout mlp_layout(MlpScratch &m, int b, int n, int K, int layers, const int *width) {
    WsLayout l(16);
    const Tiling t = tiling(n, K);
    int cmax = 0;
    for (int i = 0; i < 3; ++i) {
        m.coef[i] = nullptr;
        if (i < layers) {
            l.take(m.coef[i], (size_t)b * width[i] * 2);
            cmax = width[i] > cmax ? width[i] : cmax;
        }
    }
    const size_t slots = (size_t)b * n * t.S;
    l.take(m.mx, slots * width[layers - 1]);
    l.take(m.mn, slots * width[layers - 1]);
    l.take(m.part, (size_t)b * t.tiles * cmax * 2);
    return l;
}

}  // namespace

extern "C" int64_t pcr_edge_conv_scratch_bytes(int32_t b, int32_t n, int32_t kk, int32_t c, int32_t co) {
    pcr::clear_error();
    if (edge_check("edge_conv_scratch_bytes", b, n, kk, c, co) != PCR_OK) return -1;
    EdgeScratch e;
    const WsLayout l = edge_layout(e, b, n, c, co);
    if (!l.ok()) {
        pcr::set_error("edge_conv_scratch_bytes: the size overflows");
        return -1;
    }
    return (int64_t)l.bytes();
}

extern "C" int pcr_edge_conv(const float *feats, int64_t f_sb, int64_t f_sp, int64_t f_sc, const int32_t *idx,
                             int32_t b, int32_t n, int32_t kk, int32_t c, int32_t co, const float *w, double eps,
                             float slope, int32_t channels_first, float *out, float *rq, double *stats,
                             void *scratch, pcr_stream_t stream) {
    pcr::clear_error();
    int rc = edge_check("edge_conv", b, n, kk, c, co);
    if (rc != PCR_OK) return rc;
    if (b == 0) return PCR_OK;
    PCR_REQUIRE(feats && idx && w && out && scratch, PCR_ERR_ARG,
                "edge_conv: null pointer (feats, idx, w, out and scratch are required)");
    PCR_REQUIRE(eps >= 0.0 && eps == eps, PCR_ERR_ARG, "edge_conv: eps=%g must be >= 0", eps);
    EdgeScratch e;
    const WsLayout l = edge_layout(e, b, n, c, co);
    PCR_REQUIRE(l.bind(scratch), PCR_ERR_ARG, "edge_conv: scratch is not 16-byte aligned");
    PCR_HIP_CHECK(lds_attr());
    hipStream_t s = pcr::as_stream(stream);

    EdgeArgs a;
    a.f = feats; a.sb = f_sb; a.sp = f_sp; a.sc = f_sc; a.idx = idx; a.w = w;
    a.rq = rq ? rq : e.rq; a.mx = e.mx; a.mn = e.mn; a.part = e.part;
    a.n = n; a.kk = kk; a.c = c; a.co = co; a.tiles = (int)cdiv64(n, kEdgePts);
    hipLaunchKernelGGL(edge_gemm, dim3((unsigned)cdiv64(n, kTile), (unsigned)b, (unsigned)cdiv64(co, 128)), dim3(kThreads),
                       sizeof(float) * kTile * (c + 2), s, a);
    PCR_LAUNCH_CHECK();
    hipLaunchKernelGGL(edge_reduce, dim3((unsigned)a.tiles, (unsigned)b), dim3(kThreads), 0, s, a);
    PCR_LAUNCH_CHECK();

    FinArgs f;
    f.part = e.part; f.gamma = f.beta = nullptr; f.coef = e.coef; f.stats = stats;
    f.count = (double)n * kk; f.eps = eps; f.tiles = a.tiles; f.C = co; f.g = 1;
    OutArgs o;
    o.mx = e.mx; o.mn = e.mn; o.coef = e.coef; o.out = out;
    o.n = n; o.S = 1; o.C = co; o.channels_first = channels_first; o.slope = slope;
    return finalize_and_output(f, &o, b, s);
}

extern "C" int64_t pcr_group_mlp_scratch_bytes(int32_t b, int32_t n, int32_t K, int32_t layers, int32_t c1,
                                               int32_t c2, int32_t c3) {
    pcr::clear_error();
    const int width[3] = {c1, c2, c3};
    if (mlp_check("group_mlp_scratch_bytes", b, n, K, 1, layers, width) != PCR_OK) return -1;
    MlpScratch m;
    const WsLayout l = mlp_layout(m, b, n, K, layers, width);
    if (!l.ok()) {
        pcr::set_error("group_mlp_scratch_bytes: the size overflows");
        return -1;
    }
    return (int64_t)l.bytes();
}

extern "C" int pcr_group_mlp(const float *x, int32_t b, int32_t n, int32_t K, int32_t cin,
                             const pcr_group_mlp_net *net, int32_t group, double eps, float slope,
                             int32_t channels_first, float *out, void *scratch, pcr_stream_t stream) {
    pcr::clear_error();
    PCR_REQUIRE(net, PCR_ERR_ARG, "group_mlp: null net");
    const int layers = net->layers;
    int rc = mlp_check("group_mlp", b, n, K, cin, layers, net->width);
    if (rc != PCR_OK) return rc;
    PCR_REQUIRE(group == 1 || group == 32, PCR_ERR_ARG, "group_mlp: group=%d: 1 (instance) or 32 channels", group);
    PCR_REQUIRE(eps >= 0.0 && eps == eps, PCR_ERR_ARG, "group_mlp: eps=%g must be >= 0", eps);
    if (b == 0) return PCR_OK;
    PCR_REQUIRE(x && out && scratch, PCR_ERR_ARG, "group_mlp: null pointer (x, out and scratch are required)");
    for (int i = 0; i < layers; ++i)
        PCR_REQUIRE(net->w[i], PCR_ERR_ARG, "group_mlp: null weight of layer %d", i + 1);
    MlpScratch m;
    const WsLayout l = mlp_layout(m, b, n, K, layers, net->width);
    PCR_REQUIRE(l.bind(scratch), PCR_ERR_ARG, "group_mlp: scratch is not 16-byte aligned");
    PCR_HIP_CHECK(lds_attr());
    hipStream_t s = pcr::as_stream(stream);
    const Tiling t = tiling(n, K);

    MlpArgs a;
    a.x = x;
    for (int i = 0; i < 3; ++i) {
        a.w[i] = i < layers ? net->w[i] : nullptr;
        a.coef[i] = m.coef[i];
        a.c[i] = i < layers ? net->width[i] : 0;
    }
    a.cin = cin; a.n = n; a.K = K; a.slope = slope;
    a.part = m.part; a.mx = m.mx; a.mn = m.mn;
    a.tiles = t.tiles; a.ppt = t.ppt; a.S = t.S;
    for (int L = 1; L <= layers; ++L) {
        const int C = net->width[L - 1];
        int cmax = 0;
        for (int i = 0; i < L; ++i) cmax = net->width[i] > cmax ? net->width[i] : cmax;
        a.L = L; a.final = L == layers; a.y = net->y[L - 1];
        hipLaunchKernelGGL(group_mlp_tile, dim3((unsigned)t.tiles, (unsigned)b), dim3(kThreads),
                           sizeof(float) * kTile * (kXLd + cmax + 2), s, a);
        PCR_LAUNCH_CHECK();
        FinArgs f;
        f.part = m.part; f.gamma = net->gamma[L - 1]; f.beta = net->beta[L - 1]; f.coef = m.coef[L - 1];
        f.stats = net->stats[L - 1]; f.count = (double)n * K; f.eps = eps; f.tiles = t.tiles; f.C = C; f.g = group;
        OutArgs o;
        o.mx = m.mx; o.mn = m.mn; o.coef = m.coef[L - 1]; o.out = out;
        o.n = n; o.S = t.S; o.C = C; o.channels_first = channels_first; o.slope = slope;
        rc = finalize_and_output(f, L == layers ? &o : nullptr, b, s);
        if (rc != PCR_OK) return rc;
    }
    return PCR_OK;
}
