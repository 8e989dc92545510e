// Softmax attention without the score matrix: NgeNet's Cross_Attention and
// overlap scores (c2p-net/ngenet/models/information_interactive.py:165-214,
// NgeNet.py:170-179) and ROPNet's OverlapAttentionBlock (ROPNet/src/models/
// TFMR.py:76-106).  Contract and numerics: include/pcr_api.h.
//
// One tile routine serves every kernel.  A 256-thread workgroup owns 128
// positions of the LANE side (a wave 32 of them, one per lane and lane half)
// and walks the REGISTER side in tiles of 32:
//  * the lane side's operand (d channels) is loaded once and stays in
//    registers: lane (lr, hh) holds channels 2 t + hh of position lr;
//  * per tile the register side's operand [d][32] and its values [64][32 + 4]
//    go through LDS (the next tile's global loads fly while this one computes);
//  * S^T = X Y^T on v_mfma_f32_32x32x2_f32 with the register side on the
//    MFMA's rows: a lane ends with the 16 scores of ITS position against rows
//    (r & 3) + 8 (r >> 2) + 4 hh of the tile, so a row reduction is 15 in-lane
//    operations and one __shfl_xor(32), never a serial lane loop;
//  * the weights are then, as they sit, the B operand of the second MFMA
//    (register r is k-step r: lanes hh = 0 / 1 hold its two k), whose A operand
//    is a float4 of the value tile: out^T[channel][position] accumulates in two
//    32x32 tiles (64 channels) with no lane movement and no LDS round trip.
// Kernels:
//  * attn<0>: lane side = queries, register side = keys.  Online softmax, one
//    rescale per tile (exact expf; no deferred-rescale threshold).  64 value
//    channels per workgroup (wider dv: more workgroups, each repeating the
//    scores); dv <= 4 takes plain FMAs instead of the second MFMA.  Where the
//    grid is far below the chip the keys are split over workgroups; their
//    (O, max, sum) partials go to the caller's scratch and attn_combine folds
//    them in split order.
//  * attn<1>: the offset form's sweep 1.  As attn<0> without values, scores
//    scaled per lane (r_i); writes the rows' maxima and sums.
//  * attn<2>: the offset form's sweep 2.  Lane side = columns j (x_k),
//    register side = rows i (x_q, x_v, r_i, the row statistics): P_ij =
//    expf(a_ij - max_i) * (1 / sum_i), c_j and V P accumulate over all i.
// Padding: positions past the end of the lane side repeat the last one and are
// not stored.  A register-side position past the end repeats the last one's
// operand, its value is staged as +0 and its weight is exactly +0: in attn<0>
// and attn<1> its score is set to -inf and expf(-inf - max) = +0, the maximum
// being finite because every tile holds a real position (so no -inf - -inf);
// in attn<2> its row is staged as scale 0, max 0, 1 / sum 0.  Channels past d
// are +0 on the LANE side only; the register side re-reads channel 0 there and
// the product is 0 x finite.  So a non-finite value in channel 0 of the
// register-side operand reaches the scores of its position through the padded
// channels as well: that position's row or column is unspecified anyway
// (pcr_api.h, non-finite inputs).
#include <math.h>

#include <algorithm>

#include "pcr_internal.h"
#include "wave.h"

namespace {

using pcr::cdiv64;
using pcr::f32x16;
using pcr::tile_row;

constexpr int kThreads = 256;
constexpr int kLaneTile = 128;   // lane-side positions per workgroup
constexpr int kRegTile = 32;     // register-side positions per tile
constexpr int kDvTile = 64;      // value channels per workgroup (two 32x32 accumulators)
constexpr int kVLd = kRegTile + 4;  // value rows: 16-byte aligned, 9 slots
constexpr int kNarrow = 4;       // dv up to here: FMAs, no second MFMA
constexpr int kMaxSplit = 16;
constexpr int kMaxD = 256;
constexpr int kMaxPos = 1 << 24;

struct AttnArgs {
    const float *y; long long ysb, ysh, ysc;  // lane-side operand
    const float *x; long long xsb, xsh, xsc;  // register-side operand
    const float *v; long long vsb, vsh, vsc;  // values over the register side
    float *out; long long osb, osh, osc;
    const float *rs; long long rsb;           // per-row scale of the offset form, or null
    float *stat;                              // offset form: (b, 2, n) maxima | sums
    float *part;                              // key split: O (split, bh, dv, nl), then (split, bh, 2, nl)
    int h, nl, nr, d, dv;
    float scale;
    int nlt, ndvc, nsplit, tps;               // lane tiles, dv chunks, splits, tiles per split
};

template <int MODE, int DQ, bool NARROW>
__global__ __launch_bounds__(kThreads) void attn(AttnArgs a) {
    constexpr bool kValues = MODE != 1;
    constexpr int kXU = DQ / 8;                       // staged x elements per thread
    constexpr int kVU = NARROW ? 1 : kDvTile / 8;     // staged value elements per thread
    __shared__ float Xs[DQ * kRegTile];
    __shared__ __attribute__((aligned(16))) float Vs[kValues ? (NARROW ? kNarrow * kRegTile : kDvTile * kVLd) : 4];
    __shared__ __attribute__((aligned(16))) float Ss[MODE == 2 ? 3 * kRegTile : 4];  // max | 1 / sum | scale

    const int tid = threadIdx.x, l = tid & 63, wid = tid >> 6, hh = l >> 5, lr = l & 31;
    int bid = blockIdx.x;
    const int lt = bid % a.nlt; bid /= a.nlt;
    const int dvc = bid % a.ndvc; bid /= a.ndvc;
    const int sp = bid % a.nsplit; bid /= a.nsplit;
    const int bat = bid / a.h, head = bid % a.h;
    const int d = a.d, dv = a.dv, nl = a.nl, nr = a.nr;
    const int ch0 = dvc * kDvTile;
    const int pos = lt * kLaneTile + wid * 32 + lr;   // the lane's position
    const int posc = min(pos, nl - 1);

    const float *yb = a.y + bat * a.ysb + head * a.ysh;
    const float *xb = a.x + bat * a.xsb + head * a.xsh;
    const float *vb = kValues ? a.v + bat * a.vsb + head * a.vsh : nullptr;

    float yq[DQ / 2];
#pragma unroll
    for (int t = 0; t < DQ / 2; ++t) {  // no branches: a channel past d reads channel 0 ...
        const int c = 2 * t + hh;
        yq[t] = yb[(c < d ? c : 0) * a.ysc + posc];
    }
    {   // ... and is set to +0 here, which is what keeps channels past d out of every score.  The
        // compare is against an opaque copy of d: one shared with the loads above would keep
        // DQ / 2 lane masks alive across them, more than there are scalar registers.
        int dz = d;
        asm volatile("" : "+s"(dz));
#pragma unroll
        for (int t = 0; t < DQ / 2; ++t) yq[t] = 2 * t + hh < dz ? yq[t] : 0.0f;
    }
    float lane_scale = a.scale;
    if (MODE == 1) lane_scale = a.rs ? a.rs[bat * a.rsb + posc] : 1.0f;

    const int ntiles = (nr + kRegTile - 1) / kRegTile;
    const int tile0 = sp * a.tps, tile1 = min(ntiles, tile0 + a.tps);

    // staging: element tid + 256 u is row (tid >> 5) + 8 u, column tid & 31
    const int sx = tid & 31, srow = tid >> 5;
    const long long xstep = 8 * a.xsc;
    float xr[kXU], vr[kVU], st_m = 0.0f, st_l = 0.0f, st_r = 0.0f;
    auto load = [&](int tile) {
        const int r0 = tile * kRegTile;
        const int j = min(r0 + sx, nr - 1);
        const float *x0 = xb + j, *xp = x0 + srow * a.xsc;
        // opaque copies (here and in store): compares against d / dv proper are hoisted out of the
        // tile loop as 2 * (kXU + kVU) scalar registers of lane masks, more than there are
        int dl = d, dvl = dv;
        asm volatile("" : "+s"(dl), "+s"(dvl));
#pragma unroll
        for (int u = 0; u < kXU; ++u) {  // no branches, and a running pointer in place of kXU row offsets;
            xr[u] = *(srow + 8 * u < dl ? xp : x0);  // a row past d reads row 0: yq is +0 there
            xp += xstep;
        }
        if (kValues) {
            const bool in = r0 + sx < nr;
#pragma unroll
            for (int u = 0; u < kVU; ++u) {
                const int c = ch0 + srow + 8 * u;
                const bool ok = in && c < dvl && (!NARROW || srow < kNarrow);
                vr[u] = vb[(ok ? c : 0) * a.vsc + j];
            }
        }
        if (MODE == 2 && tid < kRegTile) {
            const int i = r0 + tid;
            const bool in = i < nr;
            const float *sb = a.stat + (size_t)bat * 2 * nr;
            st_m = in ? sb[i] : 0.0f;
            st_l = in ? sb[nr + i] : INFINITY;
            st_r = in ? (a.rs ? a.rs[bat * a.rsb + i] : 1.0f) : 0.0f;
        }
    };
    auto store = [&](int tile) {
        int dvl = dv;
        asm volatile("" : "+s"(dvl));
        const bool in = tile * kRegTile + sx < nr;
#pragma unroll
        for (int u = 0; u < kXU; ++u)
            Xs[(srow + 8 * u) * kRegTile + sx] = xr[u];
        if (kValues) {
            if (NARROW) {
                if (srow < kNarrow) Vs[srow * kRegTile + sx] = (in && srow < dvl) ? vr[0] : 0.0f;
            } else {
#pragma unroll
                for (int u = 0; u < kVU; ++u)  // values past nr or dv: +0, whatever was read
                    Vs[(srow + 8 * u) * kVLd + sx] = (in && ch0 + srow + 8 * u < dvl) ? vr[u] : 0.0f;
            }
        }
        if (MODE == 2 && tid < kRegTile) {
            Ss[tid] = st_m;
            Ss[kRegTile + tid] = 1.0f / st_l;
            Ss[2 * kRegTile + tid] = st_r;
        }
    };

    f32x16 O[2];
    float on[kNarrow];
#pragma unroll
    for (int r = 0; r < 16; ++r) { O[0][r] = 0.0f; O[1][r] = 0.0f; }
#pragma unroll
    for (int c = 0; c < kNarrow; ++c) on[c] = 0.0f;
    float m_run = -INFINITY, l_run = 0.0f;   // MODE 2: l_run is the lane's share of c_j

    if (tile0 < tile1) load(tile0);
    for (int tile = tile0; tile < tile1; ++tile) {
        store(tile);
        __syncthreads();
        if (tile + 1 < tile1) load(tile + 1);
        const int r0 = tile * kRegTile;

        f32x16 s;
#pragma unroll
        for (int r = 0; r < 16; ++r) s[r] = 0.0f;
#pragma unroll
        for (int t = 0; t < DQ / 2; ++t)
            s = __builtin_amdgcn_mfma_f32_32x32x2f32(Xs[(2 * t + hh) * kRegTile + lr], yq[t], s, 0, 0, 0);

        float p[16];
        if (MODE == 2) {
            float psum = 0.0f;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const float4 mx = *reinterpret_cast<const float4 *>(Ss + 8 * g + 4 * hh);
                const float4 il = *reinterpret_cast<const float4 *>(Ss + kRegTile + 8 * g + 4 * hh);
                const float4 rs = *reinterpret_cast<const float4 *>(Ss + 2 * kRegTile + 8 * g + 4 * hh);
                const float mxe[4] = {mx.x, mx.y, mx.z, mx.w}, ile[4] = {il.x, il.y, il.z, il.w};
                const float rse[4] = {rs.x, rs.y, rs.z, rs.w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int r = 4 * g + e;
                    // a row past nr was staged as scale 0, max 0, 1 / sum 0: expf(0) * 0 = +0
                    p[r] = expf(s[r] * rse[e] - mxe[e]) * ile[e];
                    psum = psum + p[r];
                }
            }
            l_run = l_run + psum;
        } else {
            float tv[16], mloc = -INFINITY;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const bool in = r0 + tile_row(r, hh) < nr;
                tv[r] = in ? s[r] * lane_scale : -INFINITY;
                mloc = fmaxf(mloc, tv[r]);
            }
            mloc = fmaxf(mloc, __shfl_xor(mloc, 32, 64));  // a tile holds a real row: finite on finite data
            const float m_new = fmaxf(m_run, mloc);
            const float alpha = expf(m_run - m_new);       // first tile: expf(-inf) = 0
            float psum = 0.0f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                p[r] = expf(tv[r] - m_new);  // a row past nr: expf(-inf) = +0, m_new being finite
                psum = psum + p[r];
            }
            l_run = l_run * alpha + psum;
            m_run = m_new;
            if (MODE == 0) {
                if (NARROW) {
#pragma unroll
                    for (int c = 0; c < kNarrow; ++c) on[c] = on[c] * alpha;
                } else {
#pragma unroll
                    for (int r = 0; r < 16; ++r) { O[0][r] = O[0][r] * alpha; O[1][r] = O[1][r] * alpha; }
                }
            }
        }

        if (kValues) {
            if (NARROW) {
#pragma unroll
                for (int c = 0; c < kNarrow; ++c) {  // channels past dv: +0 values, not stored
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const float4 vv = *reinterpret_cast<const float4 *>(Vs + c * kRegTile + 8 * g + 4 * hh);
                        on[c] = on[c] + p[4 * g + 0] * vv.x;
                        on[c] = on[c] + p[4 * g + 1] * vv.y;
                        on[c] = on[c] + p[4 * g + 2] * vv.z;
                        on[c] = on[c] + p[4 * g + 3] * vv.w;
                    }
                }
            } else {
#pragma unroll
                for (int dt = 0; dt < 2; ++dt) {
                    if (ch0 + 32 * dt < dv) {
#pragma unroll
                        for (int g = 0; g < 4; ++g) {
                            const float4 vv =
                                *reinterpret_cast<const float4 *>(Vs + (32 * dt + lr) * kVLd + 8 * g + 4 * hh);
                            O[dt] = __builtin_amdgcn_mfma_f32_32x32x2f32(vv.x, p[4 * g + 0], O[dt], 0, 0, 0);
                            O[dt] = __builtin_amdgcn_mfma_f32_32x32x2f32(vv.y, p[4 * g + 1], O[dt], 0, 0, 0);
                            O[dt] = __builtin_amdgcn_mfma_f32_32x32x2f32(vv.z, p[4 * g + 2], O[dt], 0, 0, 0);
                            O[dt] = __builtin_amdgcn_mfma_f32_32x32x2f32(vv.w, p[4 * g + 3], O[dt], 0, 0, 0);
                        }
                    }
                }
            }
        }
        __syncthreads();  // the tile's readers are done: the next store pass may go
    }

    // the other lane half holds the same position's other rows
    const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
    if (MODE == 1) {
        if (hh == 0 && pos < nl) {
            float *sb = a.stat + (size_t)bat * 2 * nl;
            sb[pos] = m_run;
            sb[nl + pos] = l_tot;
        }
        return;
    }
    const bool split = MODE == 0 && a.nsplit > 1;
    const size_t bh = (size_t)bat * a.h + head;
    float *ob = a.out + bat * a.osb + head * a.osh;
    long long osc = a.osc;
    if (split) {
        const size_t nbh = (size_t)gridDim.x / ((size_t)a.nlt * a.ndvc * a.nsplit) ;
        ob = a.part + (((size_t)sp * nbh + bh) * dv) * nl;
        osc = nl;
        if (hh == 0 && pos < nl && dvc == 0) {
            float *ml = a.part + (size_t)a.nsplit * nbh * dv * nl + (((size_t)sp * nbh + bh) * 2) * nl;
            ml[pos] = m_run;
            ml[nl + pos] = l_tot;
        }
    }
    const float den = MODE == 2 ? 1e-9f + l_tot : l_tot;
    if (NARROW) {
#pragma unroll
        for (int c = 0; c < kNarrow; ++c) {
            const float o = on[c] + __shfl_xor(on[c], 32, 64);
            if (hh == 0 && pos < nl && c < dv) ob[c * osc + pos] = split ? o : o / den;
        }
    } else {
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int c = ch0 + 32 * dt + tile_row(r, hh);
                if (pos < nl && c < dv) ob[c * osc + pos] = split ? O[dt][r] : O[dt][r] / den;
            }
    }
}

// one thread per (batch, head, channel, query): the splits' partials in split order
__global__ __launch_bounds__(256) void attn_combine(const float *part, float *out, long long osb, long long osh,
                                                    long long osc, int h, int n, int dv, int nsplit, int nbh) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int c = blockIdx.y, bh = blockIdx.z;
    if (i >= n) return;
    const float *ml = part + (size_t)nsplit * nbh * dv * n;
    float mx = -INFINITY;
#pragma unroll
    for (int s = 0; s < kMaxSplit; ++s)
        if (s < nsplit) mx = fmaxf(mx, ml[(((size_t)s * nbh + bh) * 2) * n + i]);
    float den = 0.0f, o = 0.0f;
#pragma unroll
    for (int s = 0; s < kMaxSplit; ++s) {
        if (s < nsplit) {
            const float *p = ml + (((size_t)s * nbh + bh) * 2) * n;
            const float w = expf(p[i] - mx);
            den = den + w * p[n + i];
            o = o + w * part[(((size_t)s * nbh + bh) * dv + c) * n + i];
        }
    }
    out[(bh / h) * osb + (bh % h) * osh + c * osc + i] = o / den;
}

struct Plan {
    int nlt, ndvc, nsplit, tps;
    long long blocks;
};

// the launch shape of attn<0>: depends on the sizes only
Plan plan_attention(int b, int h, int n, int m, int dv) {
    Plan p;
    p.nlt = (int)cdiv64(n, kLaneTile);
    p.ndvc = dv <= kNarrow ? 1 : (int)cdiv64(dv, kDvTile);
    const long long base = (long long)b * h * p.nlt * p.ndvc;
    const int ntiles = (int)cdiv64(m, kRegTile);
    int want = 1;
    if (base > 0 && base <= 64 && ntiles >= 8) want = (int)std::min<long long>({256 / base, kMaxSplit, ntiles / 4});
    p.tps = (int)cdiv64(ntiles, std::max(want, 1));
    p.nsplit = (int)cdiv64(ntiles, p.tps);
    p.blocks = base * p.nsplit;
    return p;
}

long long attention_scratch_floats(int b, int h, int n, int dv, const Plan &p) {
    return p.nsplit > 1 ? (long long)p.nsplit * b * h * (dv + 2) * n : 0;
}

int check_attention(const char *who, int b, int h, int n, int m, int d, int dv) {
    PCR_REQUIRE(b >= 0 && h >= 1, PCR_ERR_ARG, "%s: b=%d, h=%d (b must be >= 0, h >= 1)", who, b, h);
    PCR_REQUIRE(n >= 0 && n <= kMaxPos, PCR_ERR_ARG, "%s: n=%d outside 0..%d", who, n, kMaxPos);
    PCR_REQUIRE(m >= 1 && m <= kMaxPos, PCR_ERR_ARG, "%s: m=%d outside 1..%d", who, m, kMaxPos);
    PCR_REQUIRE(d >= 1 && d <= kMaxD, PCR_ERR_ARG, "%s: d=%d outside 1..%d", who, d, kMaxD);
    PCR_REQUIRE(dv >= 1 && dv <= kMaxD, PCR_ERR_ARG, "%s: dv=%d outside 1..%d", who, dv, kMaxD);
    const long long blocks = (long long)b * h * cdiv64(n, kLaneTile) * cdiv64(dv, kDvTile) * kMaxSplit;
    PCR_REQUIRE(blocks <= 0x7fffffffLL, PCR_ERR_ARG, "%s: b=%d x h=%d x n=%d too large", who, b, h, n);
    return PCR_OK;
}

template <int MODE>
void launch(const AttnArgs &a, bool narrow, long long blocks, hipStream_t s) {
    const dim3 grid((unsigned)blocks), block(kThreads);
    // DQ: the channels the kernel is unrolled for (the smallest that holds d)
#define PCR_ATTN_LAUNCH(DQ)                                                                     \
    do {                                                                                        \
        if (narrow) hipLaunchKernelGGL((attn<MODE, DQ, MODE == 0>), grid, block, 0, s, a);      \
        else hipLaunchKernelGGL((attn<MODE, DQ, false>), grid, block, 0, s, a);                 \
    } while (0)
    if (a.d <= 48) PCR_ATTN_LAUNCH(48);
    else if (a.d <= 64) PCR_ATTN_LAUNCH(64);
    else if (a.d <= 128) PCR_ATTN_LAUNCH(128);
    else PCR_ATTN_LAUNCH(256);
#undef PCR_ATTN_LAUNCH
}

}  // namespace

extern "C" int64_t pcr_attention_scratch_bytes(int32_t b, int32_t h, int32_t n, int32_t m, int32_t d,
                                               int32_t dv) {
    pcr::clear_error();
    if (check_attention("attention_scratch_bytes", b, h, n, m, d, dv) != PCR_OK) return -1;
    if (b == 0 || n == 0) return 0;
    const Plan p = plan_attention(b, h, n, m, dv);
    return (attention_scratch_floats(b, h, n, dv, p) * 4 + 255) / 256 * 256;
}

extern "C" int pcr_attention_forward(const float *q, int64_t q_sb, int64_t q_sh, int64_t q_sc, const float *k,
                                     int64_t k_sb, int64_t k_sh, int64_t k_sc, const float *v, int64_t v_sb,
                                     int64_t v_sh, int64_t v_sc, float *out, int64_t o_sb, int64_t o_sh,
                                     int64_t o_sc, int32_t b, int32_t h, int32_t n, int32_t m, int32_t d,
                                     int32_t dv, float scale, void *scratch, pcr_stream_t stream) {
    pcr::clear_error();
    int rc = check_attention("attention_forward", b, h, n, m, d, dv);
    if (rc != PCR_OK) return rc;
    if (b == 0 || n == 0) return PCR_OK;
    PCR_REQUIRE(q && k && v && out, PCR_ERR_ARG, "attention_forward: null pointer");
    const Plan p = plan_attention(b, h, n, m, dv);
    if (p.nsplit > 1) {
        PCR_REQUIRE(scratch, PCR_ERR_ARG, "attention_forward: null scratch (pcr_attention_scratch_bytes > 0)");
        PCR_REQUIRE(((uintptr_t)scratch & 15) == 0, PCR_ERR_ARG, "attention_forward: scratch is not 16-byte aligned");
    }
    hipStream_t s = pcr::as_stream(stream);
    AttnArgs a;
    a.y = q; a.ysb = q_sb; a.ysh = q_sh; a.ysc = q_sc;
    a.x = k; a.xsb = k_sb; a.xsh = k_sh; a.xsc = k_sc;
    a.v = v; a.vsb = v_sb; a.vsh = v_sh; a.vsc = v_sc;
    a.out = out; a.osb = o_sb; a.osh = o_sh; a.osc = o_sc;
    a.rs = nullptr; a.rsb = 0; a.stat = nullptr; a.part = (float *)scratch;
    a.h = h; a.nl = n; a.nr = m; a.d = d; a.dv = dv; a.scale = scale;
    a.nlt = p.nlt; a.ndvc = p.ndvc; a.nsplit = p.nsplit; a.tps = p.tps;
    launch<0>(a, dv <= kNarrow, p.blocks, s);
    PCR_LAUNCH_CHECK();
    if (p.nsplit > 1) {
        hipLaunchKernelGGL(attn_combine, dim3((unsigned)cdiv64(n, 256), (unsigned)dv, (unsigned)(b * h)), dim3(256), 0, s,
                           (const float *)scratch, out, (long long)o_sb, (long long)o_sh, (long long)o_sc, h, n, dv,
                           p.nsplit, b * h);
        PCR_LAUNCH_CHECK();
    }
    return PCR_OK;
}

extern "C" int64_t pcr_offset_attention_scratch_bytes(int32_t b, int32_t n, int32_t d, int32_t dv) {
    pcr::clear_error();
    if (check_attention("offset_attention_scratch_bytes", b, 1, n, n > 0 ? n : 1, d, dv) != PCR_OK) return -1;
    return ((long long)b * n * 8 + 255) / 256 * 256;
}

extern "C" int pcr_offset_attention_forward(const float *q, int64_t q_sb, int64_t q_sc, const float *k, int64_t k_sb,
                                            int64_t k_sc, const float *v, int64_t v_sb, int64_t v_sc,
                                            const float *row_scale, int64_t r_sb, float *out, int64_t o_sb,
                                            int64_t o_sc, int32_t b, int32_t n, int32_t d, int32_t dv,
                                            void *scratch, pcr_stream_t stream) {
    pcr::clear_error();
    int rc = check_attention("offset_attention_forward", b, 1, n, n > 0 ? n : 1, d, dv);
    if (rc != PCR_OK) return rc;
    if (b == 0 || n == 0) return PCR_OK;
    PCR_REQUIRE(q && k && v && out, PCR_ERR_ARG, "offset_attention_forward: null pointer");
    PCR_REQUIRE(scratch, PCR_ERR_ARG, "offset_attention_forward: null scratch");
    PCR_REQUIRE(((uintptr_t)scratch & 15) == 0, PCR_ERR_ARG,
                "offset_attention_forward: scratch is not 16-byte aligned");
    hipStream_t s = pcr::as_stream(stream);
    AttnArgs a;
    a.v = v; a.vsb = v_sb; a.vsh = 0; a.vsc = v_sc;
    a.out = out; a.osb = o_sb; a.osh = 0; a.osc = o_sc;
    a.rs = row_scale; a.rsb = r_sb; a.stat = (float *)scratch; a.part = nullptr;
    a.h = 1; a.nl = n; a.nr = n; a.d = d; a.dv = dv; a.scale = 1.0f;
    a.nlt = (int)cdiv64(n, kLaneTile); a.nsplit = 1; a.tps = (int)cdiv64(n, kRegTile);
    // sweep 1: rows on the lanes, columns in the registers
    a.y = q; a.ysb = q_sb; a.ysh = 0; a.ysc = q_sc;
    a.x = k; a.xsb = k_sb; a.xsh = 0; a.xsc = k_sc;
    a.ndvc = 1;
    launch<1>(a, false, (long long)b * a.nlt, s);
    PCR_LAUNCH_CHECK();
    // sweep 2: columns on the lanes, rows in the registers
    a.y = k; a.ysb = k_sb; a.ysc = k_sc;
    a.x = q; a.xsb = q_sb; a.xsc = q_sc;
    a.ndvc = (int)cdiv64(dv, kDvTile);
    launch<2>(a, false, (long long)b * a.nlt * a.ndvc, s);
    PCR_LAUNCH_CHECK();
    return PCR_OK;
}
