// The row screens of the mutual path (feature_corres_v5, featnn.hip): one
// direction's top-2 per row of the register operand against every column of
// the streamed image.  Three generations, all live:
//   featnn_row7  S = 3, 4 (32 < D <= 64): 3-term, one column tile at a time;
//   featnn_row8  S <= 2: two column tiles per step; 3-term (the fallback of the
//                1-term screens, and the whole screen with PCR_FEAT_ONE=0) or
//                1-term (PCR_FEAT_ROW9=0); featnn_slicemerge for its column slices;
//   featnn_row9  S <= 2, the default 1-term sweep -- rows stationary (row9_rows)
//                or columns stationary (row9_cols, the default) -- with
//                featnn_regroup9 and featnn_finish9.
#include "featnn_v5.h"
#include "row9_merge.h"
#include <stdlib.h>
#include <string.h>
#include <algorithm>

namespace pcr {
namespace {

// rows (pass 1) and J columns (pass 2) the 1-term screens left to the 3-term
// ones since the last reset (diagnostic, pcr_featnn_fallback_rows)
__device__ unsigned long long g_featnn_fallback_rows[2];

// One row's operand fragments exactly as feat_pack5 / feat_pack5r store them
// (same scale, same operations in the same order), for lane half h: x the
// row's f32 values (DV >= D, zero beyond D).
template <int S>
__device__ __forceinline__ void row_frags(const float *x, int D, int h, int role, int cs,
                                          f16x8 (&out)[2 * S + 1]) {
    constexpr int DV = 16 * S;
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < DV; ++k)
        if (k < D) {
            const double v = (double)x[k];
            acc = acc + v * v;
        }
    _Float16 np[3];
    double wv = acc * __builtin_ldexp(1.0, -cs);
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        np[q] = (_Float16)(float)wv;
        wv = wv - (double)np[q];
    }
    const _Float16 cval = (_Float16)__builtin_ldexpf(1.0f, cs);
    _Float16 s0[DV], s1[DV];
#pragma unroll
    for (int k = 0; k < DV; ++k) {
        const _Float16 hi = (_Float16)x[k];
        const _Float16 lo = (_Float16)(x[k] - (float)hi);
        s0[k] = role == 0 ? (_Float16)(-2.0f * (float)hi) : hi;
        s1[k] = role == 0 ? (_Float16)(-2.0f * (float)lo) : lo;
    }
#pragma unroll
    for (int c = 0; c < 2 * S + 1; ++c) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            _Float16 v0 = (_Float16)0.0f, v1 = (_Float16)0.0f;  // lane halves 0 / 1
            if (c < 2 * S) {
                const int k0 = 16 * (c % S) + j;
                const _Float16 *sg = c < S ? s0 : s1;
                v0 = k0 < D ? sg[k0] : (_Float16)0.0f;
                v1 = k0 + 8 < D ? sg[k0 + 8] : (_Float16)0.0f;
            } else {
                if (j < 3) v0 = role == 0 ? np[j] : cval;
                else if (j < 6) v0 = role == 0 ? cval : np[j - 3];
                else if (j == 6 && role == 1) v0 = (_Float16)32768.0f;  // featnn_row8's biases
                else if (j == 7 && role == 0) v0 = (_Float16)32768.0f;
            }
            out[c][j] = h ? v1 : v0;
        }
    }
}

// RT row tiles per wave share every B fragment read (two MFMAs per ds_read):
// a workgroup covers 8 * RT * 32 rows per pass over the pair's column stream,
// which halves the L2 -> LDS traffic at RT = 2 (at RT = 1 the stream of the
// packed columns ran near the chip's LDS-DMA rate: waves parked ~35 %).
//
// Pass 1's index: the column-tile number packed into the low ctbits mantissa
// bits of every value (one v_and_or) before the top-2 (featnn_row8 does the
// same on two column tiles at a time for S <= 2).
template <int S, int G, bool kIdx, int RT>
__global__ __launch_bounds__(512) void featnn_row7(RowArgs5 a) {
    constexpr int W = 8;              // waves per workgroup, RT 32-row tiles each
    constexpr int NX = 3 * S + 1, NM = 2 * S + 1;  // executed / stored k-chunks
    constexpr int kB = G * NM * 64;   // f16x8 per B buffer
    __shared__ __attribute__((aligned(16))) f16x8 Bs[2 * kB];
    const int b = blockIdx.x, xcd = b & 7, slot = b >> 3;
    const int p = (slot / a.nrb) * 8 + xcd, rb = slot - (slot / a.nrb) * a.nrb;
    if (p >= a.P) return;  // whole block
    const int nr = a.rlist ? a.rcount[p] : count_of(a.n_rows, p, a.Rmax);
    if (rb * W * RT * 32 >= nr) return;  // whole block: no rows here
    const int wid = threadIdx.x >> 6, l = threadIdx.x & 63, h = l >> 5;
    const int m = count_of(a.n_cols, p, a.Cmax);
    const int qt0 = (rb * W + wid) * RT;  // this wave's first row tile
    const int ntc = (m + 31) >> 5;
    const int ngroups = (ntc + G - 1) / G;
    const unsigned ctmask = (1u << a.ctbits) - 1u;
    unsigned keep_r = ~ctmask;
    asm("" : "+v"(keep_r));
    f16x8 A[RT][NM];
#pragma unroll
    for (int t = 0; t < RT; ++t) {
        const int qt = qt0 + t;
        if (a.rlist) {  // gathered rows: lane l holds row slot qt*32 + (l & 31), half h
            const int k = qt * 32 + (l & 31);
            if (k < nr && a.Xr) {
                const int j = a.rlist[(size_t)p * a.Rmax + k];
                const float *xr = a.Xr + ((size_t)p * a.Rmax + j) * a.D;
                const float sc = __uint_as_float(a.sc[p]);
                float x[16 * S];
                if (a.D == 16 * S && ((uintptr_t)xr & 15) == 0) {
#pragma unroll
                    for (int q = 0; q < 4 * S; ++q) {
                        const float4 v = reinterpret_cast<const float4 *>(xr)[q];
                        x[4 * q] = v.x * sc; x[4 * q + 1] = v.y * sc; x[4 * q + 2] = v.z * sc; x[4 * q + 3] = v.w * sc;
                    }
                } else {
#pragma unroll
                    for (int q = 0; q < 16 * S; ++q) x[q] = q < a.D ? xr[q] * sc : 0.0f;
                }
                row_frags<S>(x, a.D, h, a.role, a.cs, A[t]);
            } else if (k < nr) {
                const int j = a.rlist[(size_t)p * a.Rmax + k];
                const f16x8 *qp = a.Ap + ((size_t)p * a.ntr + (j >> 5)) * NM * 64 + (j & 31) + 32 * h;
#pragma unroll
                for (int c = 0; c < NM; ++c) A[t][c] = qp[(size_t)c * 64];
            } else {
#pragma unroll
                for (int c = 0; c < NM; ++c)
#pragma unroll
                    for (int q = 0; q < 8; ++q) A[t][c][q] = (_Float16)0.0f;
            }
        } else {  // padded row tiles (qt < ntr) hold sentinel rows
            const f16x8 *qp = a.Ap + ((size_t)p * a.ntr + qt) * NM * 64 + l;
#pragma unroll
            for (int c = 0; c < NM; ++c) A[t][c] = qp[(size_t)c * 64];
        }
    }
    float b1[RT][16], b2[RT][16];
#pragma unroll
    for (int t = 0; t < RT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) { b1[t][r] = __builtin_inff(); b2[t][r] = __builtin_inff(); }
    const f16x8 *bsrc = a.Bp + (size_t)p * a.ntc * NM * 64 + l;
    auto issue = [&](int grp, int bufi) {
        for (int c = wid; c < G * NM; c += W) {
            const f16x8 *src = bsrc + ((size_t)grp * G * NM + c) * 64;
            __builtin_amdgcn_global_load_lds(
                (const __attribute__((address_space(1))) void *)src,
                (__attribute__((address_space(3))) void *)(Bs + bufi * kB + c * 64), 16, 0, 0);
        }
    };
    // row top-2 of the tile's 16 values per lane, values only (2 VALU per
    // value; pass 1's group code is applied at the group's end, above).
    // No inline asm here: the compiler must see every instruction that touches
    // the accumulators (its MFMA hazard wait states are not placed around
    // inline asm; with asm v_min / v_med3 the first registers of some tiles
    // read stale values).  min(a, b) is written med3(a, b, -FLT_MAX): the min
    // builtin would add a NaN canonicalisation per operand.  A NaN value makes
    // the row's top-2 NaN (uncertified: the exact rescan decides it).
    auto epilogue = [&](const f32x16 (&acc)[RT], unsigned ct) {
        asm("" : "+s"(ct));
#pragma unroll
        for (int t = 0; t < RT; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                float vr = acc[t][r];
                if constexpr (kIdx) vr = __uint_as_float((__float_as_uint(vr) & keep_r) | ct);
                b2[t][r] = __builtin_amdgcn_fmed3f(b1[t][r], b2[t][r], vr);
                b1[t][r] = __builtin_amdgcn_fmed3f(b1[t][r], vr, -3.40282347e+38f);
            }
    };
    // VALU per MFMA slot below: the epilogue spread evenly (denser or sparser
    // spreads measured slower in round 4)
    constexpr int kV = (kIdx ? 48 : 32) * RT / NX + 1;
    issue(0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    for (int grp = 0; grp < ngroups; ++grp) {
        const int buf = grp & 1;
        if (grp + 1 < ngroups) issue(grp + 1, buf ^ 1);
        const f16x8 *Bb = Bs + buf * kB + l;
        f16x8 Bf[2][NM];
        f32x16 acc[2][RT];
#pragma unroll
        for (int c = 0; c < NM; ++c) Bf[0][c] = Bb[c * 64];
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const int cur = g & 1;
#pragma unroll
            for (int t = 0; t < RT; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[cur][t][r] = 0.0f;
#pragma unroll
            for (int c = 0; c < NX; ++c)
#pragma unroll
                for (int t = 0; t < RT; ++t)
                    acc[cur][t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(A[t][amap(c, S)], Bf[cur][bmap(c, S)],
                                                                         acc[cur][t], 0, 0, 0);
            if (g + 1 < G) {
#pragma unroll
                for (int c = 0; c < NM; ++c) Bf[cur ^ 1][c] = Bb[((g + 1) * NM + c) * 64];
            }
            if (g > 0) epilogue(acc[cur ^ 1], (unsigned)(grp * G + g - 1));
#pragma unroll
            for (int c = 0; c < NX; ++c) {
                __builtin_amdgcn_sched_group_barrier(0x008, RT, 0);
                if (g + 1 < G && c < NM) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
                if (g > 0) __builtin_amdgcn_sched_group_barrier(0x002, kV, 0);
            }
            // one scheduling region per tile: the next tile's fragments stay
            // prefetches (without it the scheduler sank them next to their
            // MFMAs: an LDS round trip in front of every MFMA)
            __builtin_amdgcn_sched_barrier(0);
        }
        epilogue(acc[(G - 1) & 1], (unsigned)(grp * G + G - 1));
        // the next group's DMA has landed for every wave, and every wave is done
        // reading this buffer before the group after next overwrites it
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }
    const int lr = l & 31;
#pragma unroll
    for (int t = 0; t < RT; ++t) {
        const int qt = qt0 + t;
        if (qt * 32 >= nr) break;
        if constexpr (kIdx) {
            int i1[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) i1[r] = (int)(__float_as_uint(b1[t][r]) & ctmask) * 32 + lr;
#pragma unroll
            for (int o = 1; o < 32; o <<= 1) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float ob1 = __shfl_xor(b1[t][r], o, 64);
                    const float ob2 = __shfl_xor(b2[t][r], o, 64);
                    const int oi1 = __shfl_xor(i1[r], o, 64);
                    top2_merge(b1[t][r], i1[r], b2[t][r], ob1, oi1, ob2);
                }
            }
            float mb1 = 0.f, mb2 = 0.f;
            int mi1 = 0;
#pragma unroll
            for (int r = 0; r < 16; ++r)
                if (lr == r) { mb1 = b1[t][r]; mb2 = b2[t][r]; mi1 = i1[r]; }
            const int rin = (lr & 3) + 8 * (lr >> 2) + 4 * h;  // this lane's row of the tile
            const int row = qt * 32 + rin;
            const bool own = lr < 16 && row < nr;
            const size_t o = (size_t)p * a.Rmax + row;
            int want = -1;  // certified rows: the winner's column
            if (own && m == 0) {
                a.nn[o] = 0;
                a.v[o] = __builtin_inf();
                a.e[o] = 0.0f;
            } else if (own) {
                const double Gm = (double)__uint_as_float(a.cmax[p]);
                const double qn = (double)a.rnr[(size_t)p * a.ntr * 32 + row];
                const double bnd = bound5(qn, Gm, 16 * NX, a.D);
                const double pk = __builtin_ldexp(1.0, a.ctbits - 23);
                a.v[o] = (double)mb1;
                a.e[o] = (float)((0.5 * bnd + pk * __builtin_fabs((double)mb1)) * (1.0 + 1e-6));
                // uncertified rows too: the screened argmin, which the exact
                // rescan overwrites (featmut_jbuild may read either)
                want = mi1;
                if (!((double)mb2 - (double)mb1 > bnd + pk * (__builtin_fabs((double)mb1) + __builtin_fabs((double)mb2))))
                    a.list[(size_t)p * a.Rmax + atomicAdd(a.count + p, 1)] = row;
            }
            if (own && want >= 0) a.nn[o] = want;
        } else {
#pragma unroll
            for (int o = 1; o < 32; o <<= 1) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float ob1 = __shfl_xor(b1[t][r], o, 64);
                    const float ob2 = __shfl_xor(b2[t][r], o, 64);
                    // second of {b1, b2} u {ob1, ob2} = med3(b1, ob1, min(b2, ob2))
                    // for sorted pairs; NaN stays NaN (uncertified)
                    const float m2 = __builtin_amdgcn_fmed3f(b2[t][r], ob2, -3.40282347e+38f);
                    b2[t][r] = __builtin_amdgcn_fmed3f(b1[t][r], ob1, m2);
                    b1[t][r] = __builtin_amdgcn_fmed3f(b1[t][r], ob1, -3.40282347e+38f);
                }
            }
            float mb1 = 0.f, mb2 = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r)
                if (lr == r) { mb1 = b1[t][r]; mb2 = b2[t][r]; }
            const int k = qt * 32 + (lr & 3) + 8 * (lr >> 2) + 4 * h;
            if (lr >= 16 || k >= nr) continue;
            const int j = a.rlist[(size_t)p * a.Rmax + k];
            // the row's bound beside its values: featmut_resolve gathers one
            // 16-byte record per candidate (rounded up: a bound stays a bound)
            const double e2 = 0.5 * bound5((double)a.rnr[(size_t)p * a.ntr * 32 + j],
                                           (double)__uint_as_float(a.cmax[p]), 16 * NX, a.D);
            a.wq[(size_t)p * a.Rmax + j] = make_float4(m == 0 ? __builtin_inff() : mb1,
                                                       m == 0 ? __builtin_inff() : mb2,
                                                       (float)(e2 * (1.0 + 1e-6)), 0.0f);
        }
    }
}

// Pass 1, round 5 (S <= 2): the row top-2 of TWO column tiles at a time.
//
// featnn_row7 spends 3 VALU per distance (code, med3, min) against 7 MFMAs per
// 32x32 tile: 262 issue cycles per tile beside 224 of MFMA pipe, so the screen
// was bound by SIMD issue.  Here a wave holds RT = 2 row tiles and walks the
// LDS group in steps of two column tiles (c0, c1): each slot (row, column lane)
// takes its pair of values (x, y) at once --
//     t = med3(b1, x, y);  b2 = min(b2, t);  b1 = min3(b1, x, y)
// (the second smallest of {b1, b2, x, y} is min(b2, med3(b1, x, y)) for
// b1 <= b2) -- 2.5 VALU per distance with the tile code, 40 per tile: 226
// issue cycles, i.e. the kernel becomes MFMA-pipe bound.  The top-2 runs on
// the f32 BIT PATTERNS as unsigned integers (v_med3_u32 / v_min3_u32 /
// v_min_u32: no NaN canonicalisation, no inline asm next to the accumulators):
// that order is the float order for non-negative values, so every value is
// shifted up by a bias B = 2^15 -- the row operand's norm chunk carries 1.0 at
// k = 6 (patched in registers) against 2^15 in the column image's (the other
// screens multiply it by 0) -- larger than any screen error (bound5 at the
// split's range |x| < 2^T, D <= 32: < 29,000 in scaled units), so no screened
// value is negative; NaN patterns sort above +inf, so NaN distances never win (as
// in the oracle's strict <), and a pair with a non-finite value is uncertified
// by its bound anyway.  The certification charges the bias's rounding.
// Schedule per step, two phases of 14 MFMAs (accumulators acc[t][c]: 64 VGPRs):
//   A: row tile 0's MFMAs | row tile 1's epilogue of the previous step
//   B: row tile 1's MFMAs | row tile 0's epilogue of this step
// so each phase is 14 MFMAs beside 80 VALU (5.7 per 32-cycle MFMA slot) and no
// accumulator is double-buffered.  The step's B fragments (10 ds_read_b128)
// open phase A, their latency covered by the epilogue's first VALU.
// ---------------------------------------------------------------------------
constexpr int kRow8Head = 24;  // epilogue VALU in front of phase A's first MFMA (the B reads' latency)

// The 1-term screen (round 6, kOne): the row operand is -2 f16(x) and the column
// operand f16(y) -- one k-segment instead of the split's three (hi.hi', hi.lo',
// lo.hi'), so S + 1 MFMAs per 32 x 32 tile instead of 3 S + 1, and the column
// stream carries only the [hi | norms] chunks of the stored image.  Its error
// is larger: with e_x = x - f16(x) (exact in f32),
//   |x.y - f16(x).f16(y)| = |e_x.y + f16(x).e_y| <= |e_x| |y| + (|x| + |e_x|) |e_y|
// by Cauchy-Schwarz; the row's |e_x| is computed here from the row itself, the
// columns' max |e_y| by the pack (emax), and both carry 2^-14 sqrt(D) for f16
// subnormals the MFMA may flush (bound1).  ~4 % of the rows (C4) do not
// certify under it: they are listed for the 3-term screen of the same rows
// (featnn_row8<.., false> over the list, the rows it cannot certify going on to
// the exact rescan as before).  The bias is 2^21 (the row patch 64 against the
// image's 2^15): the 1-term error reaches ~2^20 at the split's range.
// (kRowBias1, featnn_v5.h)
#ifdef PCR_NOSCHED
#define SGB(...) ((void)0)
#else
#define SGB(...) __builtin_amdgcn_sched_group_barrier(__VA_ARGS__)
#endif
#ifndef PCR_VA
#define PCR_VA ((80 - kRow8Head + 2 * NX - 1) / (2 * NX))
#endif
#ifndef PCR_VB
#define PCR_VB ((80 - 16 + 2 * NX - 3) / (2 * NX - 2))
#endif

// The certification and outputs of one screened row (featnn_row8's tail, and
// featnn_finish9's): B1 / B2 the row's smallest and second smallest biased
// value patterns, mi1 the column of B1, rexv the row's |x - f16(x)| (1-term),
// pk the relative truncation of the values' low bits (the column code of
// featnn_row8 pass 1; 0 when the values carry no code).  Returns whether the
// row goes to a.list (the caller appends it)
template <bool kIdx, bool kOne, int NX, bool kCT = false>
__device__ __forceinline__ bool row_tail(const RowArgs5 &a, int p, int row, int m, unsigned B1, unsigned B2,
                                         int mi1, float rexv, double pk, float ctr = 0.0f) {
    constexpr double kBias = kOne ? kRowBias1 : kRowBias;
    constexpr double u = 5.9604644775390625e-08;  // 2^-24
    const double sub = kOne ? sub_term(a.D) : 0.0;
    const float mb1 = __uint_as_float(B1), mb2 = __uint_as_float(B2);
    // this row's screen error bound (2x, as bound5): the split's or the 1-term's,
    // plus the bias's share of the accumulation error, 2 (Kt + 2) u B, doubled.
    // kCT (featnn_row9): the values are ct_j - 2 f16(x).f16(y_j) with the column
    // term ct_j = f32(|y_j|^2 + B) as the MFMA's accumulator input: the f32
    // accumulation over |C| + |products| <= B + G^2 + 2 (q + ex)(G + E), the f16
    // dot error as bound1, and ct_j's own roundings (f32 |y|^2, then + B),
    // u (2 B + G^2).  The row's |x|^2 is not in the values: its own ct (ctr,
    // rounding u (2 B + q^2)) turns a value into a distance, value - (2 B - ctr)
    // (exact: Sterbenz).  B: the pair's (feat_colterms).
    const double qn = (double)a.rnr[(size_t)p * a.ntr * 32 + row];
    const double Gm = (double)__uint_as_float(a.cmax[p]);
    double bnd, bias, ebias = 0.0;
    if constexpr (kCT) {
        const double ex = (double)rexv + sub, E = (double)__uint_as_float(a.cemax[p]) + sub;
        const double B = (double)a.cbias[p];
        bnd = bound_ct(qn, ex, Gm, E, B, 16 * NX);
        bias = 2.0 * B - (double)ctr;
        ebias = u * (2.0 * B + qn * qn) * (1.0 + 0x1p-20);
    } else {
        bnd = (kOne ? bound1(qn, (double)rexv + sub, Gm, (double)__uint_as_float(a.cemax[p]) + sub, 16 * NX)
                    : bound5(qn, Gm, 16 * NX, a.D)) +
              4.0 * (16 * NX + 2) * u * kBias;
        bias = kBias;
    }
    if constexpr (!kIdx) {  // pass 2: the row's biased top-2 values, its bound and the bias, by original row
        const double e2 = 0.5 * bnd + ebias;
        a.wq[(size_t)p * a.Rmax + row] = make_float4(m == 0 ? __builtin_inff() : mb1, m == 0 ? __builtin_inff() : mb2,
                                                     (float)(e2 * (1.0 + 1e-6)), (float)bias);
        // 1-term: a column whose gap the resolve could not use goes to the
        // 3-term screen (a.list; the 3-term pass lists nothing)
        return kOne && m != 0 && a.list &&
               !((double)mb2 - (double)mb1 > 2.0 * e2 * (1.0 + 1e-6) + 1e-6 * (double)mb1);
    }
    const size_t o = (size_t)p * a.Rmax + row;
    if (m == 0) {
        a.nn[o] = 0;
        if (a.nns) a.nns[o] = 0;
        a.v[o] = __builtin_inf();
        a.e[o] = 0.0f;
        return false;
    }
    a.v[o] = (double)mb1 - bias;  // exact (f32 values of a few binades: multiples of mb1's ulp)
    a.e[o] = (float)((0.5 * bnd + ebias + pk * __builtin_fabs((double)mb1)) * (1.0 + 1e-6));
    // the certificate: the top-2 gap against twice the per-value bound, or
    // (1-term) against a bound on the DIFFERENCE of two values' errors.  Only
    // columns j screened within 2 err of the winner j1 can overtake it, and
    // for those the dot-product errors differ by at most
    //   2 |e_x| |y_j - y_j1| + 2 |f16(x)| (|e_yj| + |e_yj1|),
    // |y_j - y_j1| <= sqrt(D_j) + sqrt(D_j1) <= sqrt(b1 + 3 err) + sqrt(b1 + err)
    // (b1 the winner's screened value): the row's nearest columns are much
    // closer together than 2 max|y|.  ~20 % fewer rows to the 3-term screen.
    double thr = bnd;
    if constexpr (kOne) {
        const double ex = (double)rexv + sub, E = (double)__uint_as_float(a.cemax[p]) + sub;
        const double dot = 2.0 * (ex * Gm + (qn + ex) * E);       // bound1's dot-product share
        const double rest = 0.5 * bnd - dot;                        // accumulation, norms, bias
        const double er = 0.5 * bnd + ebias + pk * __builtin_fabs((double)mb2);
        const double b1v = __builtin_fmax((double)mb1 - bias, 0.0);
        const double win = 2.0 * rest + 2.0 * ex * (__builtin_sqrt(b1v + 3.0 * er) + __builtin_sqrt(b1v + er)) +
                           4.0 * (qn + ex) * E;
        thr = __builtin_fmin(bnd, win * (1.0 + 1e-9));
    }
    // uncertified rows too: the screened argmin, which the 3-term pass or
    // the exact rescan overwrites; J is built from the copy in nns, which
    // nothing overwrites while featmut_jbuild reads it
    a.nn[o] = mi1;
    if (a.nns) a.nns[o] = mi1;
    return !((double)mb2 - (double)mb1 > thr + pk * (__builtin_fabs((double)mb1) + __builtin_fabs((double)mb2)));
}

// featnn_row9's early test: a row whose gap between its smallest value and
// the second smallest GROUP minimum -- an upper bound on its true second
// value -- already fails the certificate (row_tail's kCT one, pk = 0) fails it
// whatever the winning group's own second: it goes to the 3-term screen right
// after the sweep (beside the regroup) instead of through the regroup.
template <bool kIdx, int NX>
__device__ __forceinline__ bool one_term_fails(const RowArgs5 &a, int p, int row, unsigned B1, unsigned B2g,
                                               float rexv, float ctr) {
    constexpr double u = 5.9604644775390625e-08;  // 2^-24
    const double sub = sub_term(a.D);
    const double mb1 = (double)__uint_as_float(B1), mb2 = (double)__uint_as_float(B2g);
    const double qn = (double)a.rnr[(size_t)p * a.ntr * 32 + row];
    const double Gm = (double)__uint_as_float(a.cmax[p]);
    const double ex = (double)rexv + sub, E = (double)__uint_as_float(a.cemax[p]) + sub;
    const double B = (double)a.cbias[p];
    const double bnd = bound_ct(qn, ex, Gm, E, B, 16 * NX);
    const double ebias = u * (2.0 * B + qn * qn) * (1.0 + 0x1p-20);
    if constexpr (!kIdx) return !(mb2 - mb1 > (bnd + 2.0 * ebias) * (1.0 + 1e-6) + 1e-6 * mb1);
    const double dot = 2.0 * (ex * Gm + (qn + ex) * E);
    const double rest = 0.5 * bnd - dot;
    const double er = 0.5 * bnd + ebias;
    const double b1v = __builtin_fmax(mb1 - (2.0 * B - (double)ctr), 0.0);
    const double win = 2.0 * rest + 2.0 * ex * (__builtin_sqrt(b1v + 3.0 * er) + __builtin_sqrt(b1v + er)) +
                       4.0 * (qn + ex) * E;
    return !(mb2 - mb1 > __builtin_fmin(bnd, win * (1.0 + 1e-9)));
}

template <int S, int G, bool kIdx, bool kOne>
__global__ __launch_bounds__(512) void featnn_row8(RowArgs5 a) {
    constexpr int W = 8, RT = 2;                   // waves per workgroup, row tiles per wave
    constexpr int NM = 2 * S + 1;                  // stored k-chunks of the packed images
    constexpr int NX = kOne ? S + 1 : 3 * S + 1;   // executed k-chunks (MFMAs per tile)
    constexpr int NB = kOne ? S + 1 : NM;          // chunks per column tile in LDS / per row tile in registers
    constexpr int kB = G * NB * 64;                // f16x8 per B buffer
    constexpr double kBias = kOne ? kRowBias1 : kRowBias;
    static_assert(G % 2 == 0 && S <= 2, "column tiles in pairs; two row tiles fit up to S = 2");
    constexpr int kMerge = W * 64 * 17 * 8 / 16;  // the row merge's (b1, b2) slots, in f16x8
    __shared__ __attribute__((aligned(16))) f16x8 Bs[2 * kB > kMerge ? 2 * kB : kMerge];
    const int b = blockIdx.x, xcd = b & 7, slot = b >> 3;
    // pair-major (a pair's row blocks back to back on its XCD, sharing its
    // column image in that L2) or, for the short lists the 3-term screens
    // take from the 1-term ones (one block per pair, the rest exit at once),
    // row-block-major: pair-major placed the working blocks 16 apart in an
    // XCD's dispatch order, and they piled onto a few of its CUs (3x slower)
    const int ppx = (a.P + 7) >> 3;
    // row-block-major blocks also split the columns into a.csl slices (list
    // mode at small batches: a pair's short list is one block per slice)
    const int rbs = a.rbmajor ? slot / ppx : 0, csl = a.rbmajor ? a.csl : 1, sl = rbs % csl;
    const int p = a.rbmajor ? (slot % ppx) * 8 + xcd : (slot / a.nrb) * 8 + xcd;
    const int rb = a.rbmajor ? rbs / csl : slot - (slot / a.nrb) * a.nrb;
    if (p >= a.P) return;  // whole block
    // the rows: in order (pass 1) or the listed ones rlist[p][0 .. rcount[p])
    // (pass 2: J; the 3-term passes behind a 1-term one: the rows it left)
    const int *rl = a.rlist ? a.rlist + (size_t)p * a.Rmax : nullptr;
    const int nr = rl ? a.rcount[p] : count_of(a.n_rows, p, a.Rmax);
    if (a.fbdiag && rb == 0 && sl == 0 && threadIdx.x == 0 && nr > 0)
        atomicAdd(&g_featnn_fallback_rows[a.fbdiag - 1], (unsigned long long)nr);
    if (rb * W * RT * 32 >= nr) return;  // whole block: no rows here
    const int wid = threadIdx.x >> 6, l = threadIdx.x & 63, h = l >> 5;
    const int m = count_of(a.n_cols, p, a.Cmax);
    const int qt0 = (rb * W + wid) * RT;  // this wave's first row tile
    const int ntc = (m + 31) >> 5;
    const int ngall = (ntc + G - 1) / G;
    // this slice's column groups [g0, ngroups)
    const int g0 = (int)((long long)ngall * sl / csl), ngroups = (int)((long long)ngall * (sl + 1) / csl);
    const unsigned ctmask = (1u << a.ctbits) - 1u;
    unsigned keep = ~ctmask;
    asm("" : "+v"(keep));  // a VGPR operand: one v_and_or_b32 per code with the SGPR tile number
    // the row operand built from the f32 rows (one 128-byte row per lane, the
    // operands exactly as the pack stores them: the packed row image is not read)
    f16x8 A[RT][NB];
    float rex[RT];  // kOne: the row's |x - f16(x)| (rounded up)
    {
        const float sc = __uint_as_float(a.sc[p]);
#pragma unroll
        for (int t = 0; t < RT; ++t) {
            const int k = (qt0 + t) * 32 + (l & 31);
            const int row = rl ? (k < nr ? rl[k] : 0) : k;
            float x[16 * S];
            const float *xr = a.Xr + ((size_t)p * a.Rmax + row) * a.D;
            if (k < nr && a.D == 16 * S && ((uintptr_t)xr & 15) == 0) {
#pragma unroll
                for (int q = 0; q < 4 * S; ++q) {
                    const float4 v = reinterpret_cast<const float4 *>(xr)[q];
                    x[4 * q] = v.x * sc; x[4 * q + 1] = v.y * sc; x[4 * q + 2] = v.z * sc; x[4 * q + 3] = v.w * sc;
                }
            } else if (k < nr) {
#pragma unroll
                for (int q = 0; q < 16 * S; ++q) x[q] = q < a.D ? xr[q] * sc : 0.0f;
            } else {
#pragma unroll
                for (int q = 0; q < 16 * S; ++q) x[q] = 0.0f;  // rows past the count write nothing
            }
            f16x8 fr[NM];
            row_frags<S>(x, a.D, h, a.role, a.cs, fr);
#pragma unroll
            for (int c = 0; c < NB; ++c) A[t][c] = fr[kOne ? (c < S ? c : 2 * S) : c];
            // the bias (see above): 1.0 (3-term) or 64 (1-term) opposite the image's 2^15
            const _Float16 bv = (_Float16)(kOne ? 64.0f : 1.0f);
            if (h == 0) {
                if (a.role == 0) A[t][NB - 1][6] = bv;
                else A[t][NB - 1][7] = bv;
            }
            if constexpr (kOne) {
                double ea = 0.0;
#pragma unroll
                for (int q = 0; q < 16 * S; ++q) {
                    const double e = (double)(x[q] - (float)(_Float16)x[q]);
                    ea = ea + e * e;
                }
                rex[t] = split_err_norm(ea);
                asm volatile("" : "+v"(rex[t]));  // here, not sunk to its use after the loop (the rows stay live)
            } else {
                rex[t] = 0.0f;
            }
        }
    }
    unsigned b1[RT][16], b2[RT][16];
#pragma unroll
    for (int t = 0; t < RT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) { b1[t][r] = 0x7f800000u; b2[t][r] = 0x7f800000u; }
    const f16x8 *bsrc = a.Bp + (size_t)p * a.ntc * NM * 64 + l;
    auto issue = [&](int grp, int bufi) {
        for (int c = wid; c < G * NB; c += W) {
            const int g = c / NB, cc = c - g * NB;
            const int sch = kOne ? (cc < S ? cc : 2 * S) : cc;  // the stored chunk
            const f16x8 *src = bsrc + ((size_t)(grp * G + g) * NM + sch) * 64;
            __builtin_amdgcn_global_load_lds(
                (const __attribute__((address_space(1))) void *)src,
                (__attribute__((address_space(3))) void *)(Bs + bufi * kB + c * 64), 16, 0, 0);
        }
    };
    // row tile t's slots take the values of column tiles ct (x) and ct + 1 (y)
    auto epilogue = [&](const f32x16 (&x)[2], int t, unsigned ct) {
        asm("" : "+s"(ct));
        const unsigned ct1 = ct + 1u;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            // pass 1: the tile numbers in the low bits; pass 2: values only
            const unsigned cx = kIdx ? (__float_as_uint(x[0][r]) & keep) | ct : __float_as_uint(x[0][r]);
            const unsigned cy = kIdx ? (__float_as_uint(x[1][r]) & keep) | ct1 : __float_as_uint(x[1][r]);
            // the median as v_med3_f32 (the same order on these non-negative
            // patterns; an integer median shares min(b1, cx) with the min3
            // below and costs a v_min more)
            const unsigned md = __float_as_uint(
                __builtin_amdgcn_fmed3f(__uint_as_float(b1[t][r]), __uint_as_float(cx), __uint_as_float(cy)));
            b2[t][r] = umin2(b2[t][r], md);
            b1[t][r] = umin2(b1[t][r], umin2(cx, cy));
            asm("" : "+v"(b2[t][r]));  // no b2 min chain across steps (it held 32 more VGPRs and spilled)
        }
    };
    // executed chunk c -> the register / LDS chunk holding its operands
    auto ach = [](int c) { return kOne ? c : amap(c, S); };
    auto bch = [](int c) { return kOne ? c : bmap(c, S); };
    f32x16 acc[RT][2];
    // the first phase A finds a harmless pending epilogue: +inf with code 0
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[1][c][r] = __builtin_inff();
    unsigned pend = 0u;
    const f32x16 zero = {};
    // VALU per phase (two tiles' epilogues): 80; spread over the phase's MFMAs
    constexpr int kVA = PCR_VA;
    constexpr int kVB = PCR_VB;
    if (g0 < ngroups) issue(g0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    for (int grp = g0; grp < ngroups; ++grp) {
        const int buf = (grp - g0) & 1;
        if (grp + 1 < ngroups) issue(grp + 1, buf ^ 1);
        const f16x8 *Bb = Bs + buf * kB + l;
        // the step's B fragments, read in MFMA order (the first MFMAs wait for
        // the first reads only): the group's first step reads them at its
        // start, every later step at the end of the previous step's phase B
        f16x8 Bf[2][NB];
#pragma unroll
        for (int c = 0; c < NB; ++c)
#pragma unroll
            for (int u = 0; u < 2; ++u) Bf[u][c] = Bb[(u * NB + c) * 64];
#pragma unroll
        for (int st = 0; st < G / 2; ++st) {
            const unsigned ct = (unsigned)(grp * G + 2 * st);
            // phase A
#pragma unroll
            for (int c = 0; c < NX; ++c)
#pragma unroll
                for (int u = 0; u < 2; ++u)
                    acc[0][u] = __builtin_amdgcn_mfma_f32_32x32x16_f16(A[0][ach(c)], Bf[u][bch(c)],
                                                                       c == 0 ? zero : acc[0][u], 0, 0, 0);
            epilogue(acc[1], 1, pend);
            if (st == 0) SGB(0x100, 2 * NB, 0);
            SGB(0x002, kRow8Head, 0);
#pragma unroll
            for (int i = 0; i < 2 * NX; ++i) {
                SGB(0x008, 1, 0);
                SGB(0x002, kVA, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
            // phase B
#pragma unroll
            for (int c = 0; c < NX; ++c)
#pragma unroll
                for (int u = 0; u < 2; ++u)
                    acc[1][u] = __builtin_amdgcn_mfma_f32_32x32x16_f16(A[1][ach(c)], Bf[u][bch(c)],
                                                                       c == 0 ? zero : acc[1][u], 0, 0, 0);
            epilogue(acc[0], 0, ct);
            if (st + 1 < G / 2) {  // the next step's fragments, behind this phase's last MFMA
#pragma unroll
                for (int c = 0; c < NB; ++c)
#pragma unroll
                    for (int u = 0; u < 2; ++u) Bf[u][c] = Bb[((2 * st + 2 + u) * NB + c) * 64];
            }
            SGB(0x008, 2, 0);
#pragma unroll
            for (int i = 0; i < 2 * NX - 2; ++i) {
                SGB(0x002, kVB, 0);
                SGB(0x008, 1, 0);
            }
            if (st + 1 < G / 2) SGB(0x100, 2 * NB, 0);
            SGB(0x002, 16, 0);
            __builtin_amdgcn_sched_barrier(0);
            pend = ct;
        }
        // the next group's DMA has landed for every wave, and every wave is done
        // reading this buffer before the group after next overwrites it
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }
    epilogue(acc[1], 1, pend);
    // Row merge through LDS (the B buffers are free): each lane stores its 16
    // slots (b1, b2), then lane L takes row L & 31 and half of its 32 column
    // lanes (16 entries in column order: on equal patterns -- same value, same
    // tile code -- the lower column lane stays), and the two halves combine by
    // one exchange.  Unsigned order = the screen's order (all values >= 0 or
    // +inf).  Stride 17: the stores and the row reads spread over the banks.
    uint2 *tl = reinterpret_cast<uint2 *>(Bs) + (size_t)wid * 64 * 17;
    const int R = l & 31, hR = (R >> 2) & 1, rR = (R & 3) + 4 * (R >> 3), j0 = 16 * h;
#pragma unroll
    for (int t = 0; t < RT; ++t) {  // every wave runs both (the barriers), rows past nr write nothing
        const int qt = qt0 + t;
        __syncthreads();  // (t = 0: every wave is past its last B read; t = 1: the row reads)
#pragma unroll
        for (int r = 0; r < 16; ++r) tl[l * 17 + r] = make_uint2(b1[t][r], b2[t][r]);
        __syncthreads();
        unsigned B1 = 0x7f800000u, B2 = 0x7f800000u;
        int jw = j0;
#pragma unroll
        for (int jj = 0; jj < 16; ++jj) {
            const uint2 e = tl[(hR * 32 + j0 + jj) * 17 + rR];
            B2 = umin2(umin2(B2, e.y), umax2(B1, e.x));
            const bool take = e.x < B1;
            B1 = take ? e.x : B1;
            jw = take ? j0 + jj : jw;
        }
        {   // lanes L < 32 hold column lanes 0..15: the partner's (16..31) win strictly below
            const unsigned o1 = (unsigned)__shfl_xor((int)B1, 32, 64), o2 = (unsigned)__shfl_xor((int)B2, 32, 64);
            const int oj = __shfl_xor(jw, 32, 64);
            B2 = umin2(umin2(B2, o2), umax2(B1, o1));
            const bool take = o1 < B1;
            B1 = take ? o1 : B1;
            jw = take ? oj : jw;
        }
        const int mi1 = (int)(B1 & ctmask) * 32 + jw;
        const int k = qt * 32 + R;
        if (h != 0 || k >= nr) continue;
        const int row = rl ? rl[k] : k;  // the original row index
        if (csl > 1) {  // this slice's partial, merged by featnn_slicemerge
            a.part[((size_t)p * csl + sl) * a.Rmax + k] = make_uint4(B1, B2, (unsigned)mi1, 0u);
            continue;
        }
        if (row_tail<kIdx, kOne, NX>(a, p, row, m, B1, B2, mi1, rex[t], __builtin_ldexp(1.0, a.ctbits - 23)))
            a.list[(size_t)p * a.Rmax + atomicAdd(a.count + p, 1)] = row;
    }
}

// featnn_row8's column slices (list mode, csl > 1) merged: per listed row the
// smallest B1 over the slices (the values carry the column tile code: no two
// are equal across slices), B2 the second smallest of the union, then the
// row's certification and outputs as the unsliced kernel's tail
template <int S, bool kIdx>
__global__ __launch_bounds__(256) void featnn_slicemerge(RowArgs5 a) {
    constexpr int NX = 3 * S + 1;
    const int p = blockIdx.y, k = blockIdx.x * 256 + threadIdx.x;
    const int *rl = a.rlist + (size_t)p * a.Rmax;
    if (k >= a.rcount[p]) return;
    unsigned B1 = 0x7f800000u, B2 = 0x7f800000u, mi = 0u;
    for (int s2 = 0; s2 < a.csl; ++s2) {
        const uint4 q = a.part[((size_t)p * a.csl + s2) * a.Rmax + k];
        B2 = umin2(umin2(B2, q.y), umax2(B1, q.x));
        mi = q.x < B1 ? q.z : mi;
        B1 = umin2(B1, q.x);
    }
    const int row = rl[k];
    if (row_tail<kIdx, false, NX>(a, p, row, count_of(a.n_cols, p, a.Cmax), B1, B2, (int)mi, 0.0f,
                                  __builtin_ldexp(1.0, a.ctbits - 23)))
        a.list[(size_t)p * a.Rmax + atomicAdd(a.count + p, 1)] = row;
}

// ---------------------------------------------------------------------------
// Round 6: the 1-term screens without a per-value index (featnn_row9, then
// featnn_regroup9).  featnn_row8 spends 2.5 VALU per screened value -- the
// column code OR-ed into the low bits (1) and the running top-2 (1.5) -- i.e.
// 40 VALU per 32 x 32 tile beside 3 MFMAs (96 pipe cycles): the 1-term pass
// is VALU-issue bound (~190 issue cycles per tile).  featnn_row9 swaps the
// MFMA's operands (the column fragments as A, the row's as B: the tile's
// transpose), so a lane holds ONE row and 16 columns of each column tile
// (register r: column 8 (r / 4) + 4 h + (r % 4), h the lane half).  A lane's
// 32 values of a step (two column tiles) form a group, and the sweep keeps
// per lane only
//   B1 -- the smallest value,
//   B2 -- the second smallest GROUP minimum,
//   I  -- the step of B1's group:
// 16 v_min3 + 5 VALU per step and row tile (10.5 per tile): the loop is
// MFMA-pipe bound.  The lane halves merge at the end (a row's other half is
// another set of groups).  What the sweep does not know -- the argmin's column
// and the second smallest value INSIDE the winning group -- featnn_regroup9
// recovers by re-running the identical MFMA chain (same operands, same order:
// bit-identical values) for the winning step only: a pair's rows bucketed by
// that step, one 32-row tile per bucket segment (~1 % of the sweep's MFMAs).
// Then second = min(B2, the group's own second) exactly, the values carry no
// code bits (pk = 0), and the certification and outputs are featnn_row8's
// (row_tail, its kCT bound).
// The norms are not an MFMA: the columns' terms ct_j = f32(|y_j|^2 + B)
// (feat_colterms, B the pair's) are the MFMA chain's accumulator input, so a
// tile costs S = 2 MFMAs instead of S + 1 and the values are ct_j - 2 x.y_j
// (the row's |x|^2 left out: a constant per row).  A lane's 16 C values per
// column tile come from the LDS copy of the group's terms or by DPP row
// broadcasts of one float per lane (see the sweep).
// ---------------------------------------------------------------------------

// min of a lane's 32 values of one step (two column tiles): three v_min3 chains
__device__ __forceinline__ unsigned group_min32(const f32x16 &x, const f32x16 &y) {
    unsigned c0 = umin2(umin2(fbits(x[0]), fbits(x[1])), fbits(x[2]));
    unsigned c1 = umin2(umin2(fbits(x[11]), fbits(x[12])), fbits(x[13]));
    unsigned c2 = umin2(umin2(fbits(y[6]), fbits(y[7])), fbits(y[8]));
#pragma unroll
    for (int r = 3; r < 11; r += 2) c0 = umin2(umin2(c0, fbits(x[r])), fbits(x[r + 1]));
    c1 = umin2(umin2(c1, fbits(x[14])), fbits(x[15]));
#pragma unroll
    for (int r = 0; r < 6; r += 2) c1 = umin2(umin2(c1, fbits(y[r])), fbits(y[r + 1]));
#pragma unroll
    for (int r = 9; r < 15; r += 2) c2 = umin2(umin2(c2, fbits(y[r])), fbits(y[r + 1]));
    c2 = umin2(c2, fbits(y[15]));
    return umin2(umin2(c0, c1), c2);
}

// What follows a sweep, either form, for one row (lane half h of row slot k
// holds its half's B1, B2, I): the row's two lane halves -- the smaller B1 wins
// (the lower half on a tie: a zero gap, uncertified either way), the second
// smallest of the union.  The row goes to its winning step's bucket as (row,
// B1, B2, half); a row that one_term_fails, or past a full bucket, goes to the
// 3-term screen's list instead (and its record is marked for featnn_finish9
// to skip)
template <int S, bool kIdx>
__device__ __forceinline__ void row9_settle(const RowArgs5 &a, int p, const int *rl, int nr, int k, int h,
                                            unsigned B1, unsigned B2, unsigned I) {
    const int nst = a.ntc >> 1;
    const unsigned o1 = (unsigned)__shfl_xor((int)B1, 32, 64);
    const unsigned o2 = (unsigned)__shfl_xor((int)B2, 32, 64);
    const unsigned oi = (unsigned)__shfl_xor((int)I, 32, 64);
    const unsigned s2 = umin2(umax2(B1, o1), umin2(B2, o2));
    const bool mine = B1 < o1 || (B1 == o1 && h == 0);
    const unsigned w1 = mine ? B1 : o1;
    const unsigned wst = min(mine ? I : oi, (unsigned)(nst - 1));
    if (h == 0 && k < nr) {
        // re-read, not kept from the operand build across the sweep (registers)
        const int row = rl ? reinterpret_cast<const volatile int *>(rl)[k] : k;
        const size_t bk = (size_t)p * nst + wst;
        const bool early = one_term_fails<kIdx, S>(a, p, row, w1, s2, a.rre[(size_t)p * a.ntr * 32 + row],
                                                   a.rct[(size_t)p * a.ntr * 32 + row]);
        const int rank = early ? a.bcap : atomicAdd(a.bcnt + bk, 1);
        if (rank < a.bcap) {
            a.blist[bk * a.bcap + rank] = make_uint4((unsigned)row, w1, s2, mine ? 0u : 1u);
        } else {
            // (a zero counter, B1 and no column yet: featnn_thresh9's inputs)
            a.rec[(size_t)p * a.Rmax + row] = make_uint4(0u, w1, 0xffffffffu, 1u);
            a.list[(size_t)p * a.Rmax + atomicAdd(a.count + p, 1)] = row;
        }
    }
}

// The sweep, rows stationary: a wave keeps RT = 2 row tiles in registers and the
// block streams the column groups through LDS.
template <int S, int G, bool kIdx>
__device__ __forceinline__ void row9_rows(const RowArgs5 &a) {
    constexpr int W = 8, RT = 2;          // waves per workgroup, row tiles per wave
    constexpr int NB = S;                 // executed chunks: the f16 segment (a tile's first NB of a.ich stored)
    constexpr int kT = G * NB * 64;       // f16x8 of a B buffer's fragments
    constexpr int kB = kT + G * 8;        // + the group's column terms (G x 32 floats)
    static_assert(G % 8 == 0 && S <= 2, "column tiles in pairs; the terms in whole 1 KB DMA pieces");
    constexpr int kTC = G / 8;            // the group's terms: 1 KB pieces
    __shared__ __attribute__((aligned(16))) f16x8 Bs[2 * kB];
    const int b = blockIdx.x, xcd = b & 7, slot = b >> 3;
    const int ppx = (a.P + 7) >> 3;
    const int p = a.rbmajor ? (slot % ppx) * 8 + xcd : (slot / a.nrb) * 8 + xcd;
    const int rb = a.rbmajor ? slot / ppx : slot - (slot / a.nrb) * a.nrb;
    if (p >= a.P) return;  // whole block
    const int *rl = a.rlist ? a.rlist + (size_t)p * a.Rmax : nullptr;
    const int nr = rl ? a.rcount[p] : count_of(a.n_rows, p, a.Rmax);
    if (rb * W * RT * 32 >= nr) return;  // whole block: no rows here
    const int wid = threadIdx.x >> 6, l = threadIdx.x & 63, h = l >> 5;
    const int m = count_of(a.n_cols, p, a.Cmax);
    const int qt0 = (rb * W + wid) * RT;  // this wave's first row tile
    const int ntc = (m + 31) >> 5;
    const int ngroups = (ntc + G - 1) / G;
    f16x8 A[RT][NB];
#pragma unroll
    for (int t = 0; t < RT; ++t) {
        const int k = (qt0 + t) * 32 + (l & 31);
        row_operand<S, kIdx ? 0 : 1>(a, p, rl ? (k < nr ? rl[k] : 0) : (k < nr ? k : 0), k < nr, h, A[t]);
    }
    // per row tile: B1, B2, I as above; pm the min of the current step's
    // first column tile (the group's first half)
    unsigned B1[RT], B2[RT], I[RT], pm[RT];
#pragma unroll
    for (int t = 0; t < RT; ++t) { B1[t] = 0x7f800000u; B2[t] = 0x7f800000u; I[t] = 0u; pm[t] = 0x7f800000u; }
    const int nm = a.ich;  // the image's tile stride in chunks
    const f16x8 *bsrc = a.Bp + (size_t)p * a.ntc * nm * 64 + l;
    const float *csrc = a.cct + (size_t)p * a.ntc * 32 + 4 * l;
    auto issue = [&](int grp, int bufi) {
        for (int c = wid; c < G * NB + kTC; c += W) {
            if (c >= G * NB) {  // the group's column terms: G x 128 B, 16 B per lane and piece
                const int tc = c - G * NB;
                __builtin_amdgcn_global_load_lds(
                    (const __attribute__((address_space(1))) void *)(csrc + (size_t)grp * G * 32 + tc * 256),
                    (__attribute__((address_space(3))) void *)(Bs + bufi * kB + kT + tc * 64), 16, 0, 0);
                continue;
            }
            const int g = c / NB, cc = c - g * NB;
            const f16x8 *src = bsrc + ((size_t)(grp * G + g) * nm + cc) * 64;
            __builtin_amdgcn_global_load_lds(
                (const __attribute__((address_space(1))) void *)src,
                (__attribute__((address_space(3))) void *)(Bs + bufi * kB + c * 64), 16, 0, 0);
        }
    };
    // min of a lane's 16 values of one column tile and c0 (two v_min3 chains)
    auto min16 = [](const f32x16 &x, unsigned c0) {
        unsigned c1 = umin2(umin2(fbits(x[8]), fbits(x[9])), fbits(x[10]));
        c0 = umin2(umin2(c0, fbits(x[0])), fbits(x[1]));
        c1 = umin2(umin2(c1, fbits(x[11])), fbits(x[12]));
        c0 = umin2(umin2(c0, fbits(x[2])), fbits(x[3]));
        c1 = umin2(umin2(c1, fbits(x[13])), fbits(x[14]));
        c0 = umin2(umin2(c0, fbits(x[4])), fbits(x[5]));
        c0 = umin2(umin2(c0, fbits(x[6])), fbits(x[7]));
        return umin2(umin2(c1, fbits(x[15])), c0);
    };
    // row tile t's group of step st closed by its second column tile y
    auto close = [&](const f32x16 &y, int t, unsigned st) {
        const unsigned mn = min16(y, pm[t]);
        // 2nd smallest of {B1, B2, mn}: their median (the full pattern, so it
        // selects to one v_med3_u32)
        const unsigned n2 = umax2(umin2(B1[t], B2[t]), umin2(umax2(B1[t], B2[t]), mn));
        I[t] = mn < B1[t] ? st : I[t];
        B1[t] = umin2(B1[t], mn);
        B2[t] = n2;
    };
    // A tile's 16 column terms per lane (the MFMA's C): registers [0, 4 KL) as
    // KL ds_read_b128 of the LDS copy, the rest from ONE float per lane -- lane
    // l holds column 8 (n / 4) + (n % 4) + 4 h of the tile (n = l % 16), so the
    // DPP row broadcast of row position r gives every lane its register r's
    // column (one v_mov_dpp per register).  Measured (C4, featnn_bench alone):
    // pass 1 1.15 ms with KL = 0, 1.19 with KL = 4 (4 KB of LDS reads per wave
    // and column tile), the mixes 1.21 - 1.24; pass 2 0.77 with KL = 4 against
    // 0.80 with KL = 0.
    const int cl = 8 * ((l & 15) >> 2) + (l & 3) + 4 * h;
#ifndef PCR_CT_LDS1
#define PCR_CT_LDS1 0
#endif
#ifndef PCR_CT_LDS2
#define PCR_CT_LDS2 4
#endif
    constexpr int KL = kIdx ? PCR_CT_LDS1 : PCR_CT_LDS2;
    constexpr int kCR = KL + (KL < 4 ? 1 : 0), kCV = 16 - 4 * KL;  // LDS reads / VALU per tile's terms
    // registers [4 KL, 16) of a tile's terms from the lane's float v
    auto cterms = [&](f32x16 &c, int v) {
#define PCR_BC(r) if ((r) >= 4 * KL) c[r] = __int_as_float(__builtin_amdgcn_mov_dpp(v, 0x150 + (r), 0xf, 0xf, false))
        PCR_BC(0); PCR_BC(1); PCR_BC(2); PCR_BC(3); PCR_BC(4); PCR_BC(5); PCR_BC(6); PCR_BC(7);
        PCR_BC(8); PCR_BC(9); PCR_BC(10); PCR_BC(11); PCR_BC(12); PCR_BC(13); PCR_BC(14); PCR_BC(15);
#undef PCR_BC
    };
    // Schedule per step (two column tiles u = 0, 1; both row tiles in each
    // phase), so one tile's 16 column terms are live at a time:
    //   A: tile u = 0's 4 MFMAs (C = its terms) | the previous step's closes
    //   B: tile u = 1's 4 MFMAs                  | this step's first halves (pm)
    // Each phase reads the next phase's fragments and terms behind its MFMAs.
    f32x16 acc[RT][2];
    // the first phase A closes a harmless pending group: +inf
#pragma unroll
    for (int t = 0; t < RT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][1][r] = __builtin_inff();
    unsigned pend = 0u;
    issue(0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    for (int grp = 0; grp < ngroups; ++grp) {
        const int buf = grp & 1;
        if (grp + 1 < ngroups) issue(grp + 1, buf ^ 1);
        const f16x8 *Bb = Bs + buf * kB + l;
        const float *Cb = reinterpret_cast<const float *>(Bs + buf * kB + kT);
        const int *Cv = reinterpret_cast<const int *>(Cb) + cl;
        auto cnext = [&](int u) {
            f32x16 c;
#pragma unroll
            for (int j = 0; j < KL; ++j) {
                const float4 v = *reinterpret_cast<const float4 *>(Cb + 32 * u + 8 * j + 4 * h);
                c[4 * j] = v.x; c[4 * j + 1] = v.y; c[4 * j + 2] = v.z; c[4 * j + 3] = v.w;
            }
            if constexpr (KL < 4) cterms(c, Cv[32 * u]);
            return c;
        };
        f16x8 Bf[NB];
        f32x16 Cf;
#pragma unroll
        for (int c = 0; c < NB; ++c) Bf[c] = Bb[c * 64];
        Cf = cnext(0);
        __builtin_amdgcn_sched_barrier(0);  // the group's first reads: a region of their own
#pragma unroll
        for (int st = 0; st < G / 2; ++st) {
            const unsigned stp = (unsigned)(grp * (G / 2) + st);
            // phase A
#pragma unroll
            for (int c = 0; c < NB; ++c)
#pragma unroll
                for (int t = 0; t < RT; ++t)
                    acc[t][0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(Bf[c], A[t][c], c == 0 ? Cf : acc[t][0], 0, 0, 0);
#pragma unroll
            for (int t = 0; t < RT; ++t) close(acc[t][1], t, pend);
#pragma unroll
            for (int c = 0; c < NB; ++c) Bf[c] = Bb[((2 * st + 1) * NB + c) * 64];
            Cf = cnext(2 * st + 1);
            SGB(0x002, 2, 0);
#pragma unroll
            for (int i = 0; i < NB * RT; ++i) {
                SGB(0x008, 1, 0);
                SGB(0x002, 5, 0);
            }
            SGB(0x100, NB + kCR, 0);
            SGB(0x002, 6 + kCV, 0);
            __builtin_amdgcn_sched_barrier(0);
            // phase B
#pragma unroll
            for (int c = 0; c < NB; ++c)
#pragma unroll
                for (int t = 0; t < RT; ++t)
                    acc[t][1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(Bf[c], A[t][c], c == 0 ? Cf : acc[t][1], 0, 0, 0);
#pragma unroll
            for (int t = 0; t < RT; ++t) pm[t] = min16(acc[t][0], 0x7f800000u);
            if (st + 1 < G / 2) {
#pragma unroll
                for (int c = 0; c < NB; ++c) Bf[c] = Bb[((2 * st + 2) * NB + c) * 64];
                Cf = cnext(2 * st + 2);
            }
#pragma unroll
            for (int i = 0; i < NB * RT; ++i) {
                SGB(0x008, 1, 0);
                SGB(0x002, 4, 0);
            }
            if (st + 1 < G / 2) SGB(0x100, NB + kCR, 0);
            if (st + 1 < G / 2 && kCV) SGB(0x002, kCV, 0);
            __builtin_amdgcn_sched_barrier(0);
            pend = stp;
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }
#pragma unroll
    for (int t = 0; t < RT; ++t) close(acc[t][1], t, pend);
#pragma unroll
    for (int t = 0; t < RT; ++t)
        row9_settle<S, kIdx>(a, p, rl, nr, (qt0 + t) * 32 + (l & 31), h, B1[t], B2[t], I[t]);
}

// The sweep, columns stationary (S <= 2): the loop above turned inside out.  A
// workgroup still owns 16 row tiles of one pair, but its W waves split the
// column steps (wave w takes steps w, w + W, ...) and every wave runs over all
// 16 row tiles:
//   - the block's row operands sit in LDS as [row tile][chunk][lane] (32 KB at
//     S = 2, built once; a wave reads a row tile's with S ds_read_b128, one
//     row tile ahead);
//   - a step's column fragments go from the packed image straight to registers
//     (each is read by one wave of the block: no LDS copy), its two tiles'
//     terms as one float per lane and 16 DPP row broadcasts each -- once per
//     step, shared by the 16 row tiles, where the rows-stationary loop redoes
//     them for every pair of row tiles; the next step's are loaded meanwhile;
//   - per row tile the identical MFMA chains, one group_min32 over both
//     column tiles (no pm) and the close; the accumulators alternate between
//     two sets, so a row tile's minima issue under the next one's MFMAs.
// No barrier and no LDS write inside the loop.  The waves' triples merge
// through LDS at the end (row9_merge.h: bit-identical to one wave taking every
// step in order), W row tiles per round, and wave w settles row tiles
// [w NT / W, (w + 1) NT / W) as the loop above does.
// Registers: Cf 32, Bf 16 + 18 (the next step's), B1 / B2 / I 48, acc 64,
// A 16: two waves per SIMD.
template <int S, int G, bool kIdx, int W>
__device__ __forceinline__ void row9_cols(const RowArgs5 &a) {
    constexpr int NT = 16, RT = NT / W;   // row tiles per workgroup; settled per wave
    constexpr int NB = S;
    constexpr int kOp = NT * NB * 64;     // f16x8 of the row operands
    constexpr int kMg = W * W * 3 * 16;   // f16x8 of a merge round: [wave][row tile of the round][B1, B2, I][lane]
    static_assert(G % 2 == 0 && NT % W == 0 && S <= 2, "column tiles in pairs; whole row tiles per wave");
    __shared__ __attribute__((aligned(16))) f16x8 As[kOp > kMg ? kOp : kMg];
    const int b = blockIdx.x, xcd = b & 7, slot = b >> 3;
    const int ppx = (a.P + 7) >> 3;
    const int p = a.rbmajor ? (slot % ppx) * 8 + xcd : (slot / a.nrb) * 8 + xcd;
    const int rb = a.rbmajor ? slot / ppx : slot - (slot / a.nrb) * a.nrb;
    if (p >= a.P) return;  // whole block
    const int *rl = a.rlist ? a.rlist + (size_t)p * a.Rmax : nullptr;
    const int nr = rl ? a.rcount[p] : count_of(a.n_rows, p, a.Rmax);
    if (rb * NT * 32 >= nr) return;  // whole block: no rows here
    // (uniform: the step loop's control stays scalar)
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), l = threadIdx.x & 63, h = l >> 5;
    const int m = count_of(a.n_cols, p, a.Cmax);
    const int ntc = (m + 31) >> 5;
    const int nsteps = (ntc + G - 1) / G * (G / 2);  // the rows-stationary loop's, padding tiles included
    f16x8 *Asl = As + l;
#pragma unroll
    for (int t = 0; t < RT; ++t) {
        const int tt = wid * RT + t;
        const int k = (rb * NT + tt) * 32 + (l & 31);
        f16x8 A[NB];
        row_operand<S, kIdx ? 0 : 1>(a, p, rl ? (k < nr ? rl[k] : 0) : (k < nr ? k : 0), k < nr, h, A);
#pragma unroll
        for (int c = 0; c < NB; ++c) Asl[(tt * NB + c) * 64] = A[c];
    }
    __syncthreads();
    unsigned B1[NT], B2[NT], I[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) { B1[t] = kRow9Inf; B2[t] = kRow9Inf; I[t] = 0u; }
    const int nm = a.ich;  // the image's tile stride in chunks
    const f16x8 *bsrc = a.Bp + (size_t)p * a.ntc * nm * 64 + l;
    // lane l's column of a tile's terms (the DPP row broadcast of row position
    // r then gives every lane its register r's column, as in the loop above)
    const int *csrc = reinterpret_cast<const int *>(a.cct + (size_t)p * a.ntc * 32) + 8 * ((l & 15) >> 2) + (l & 3) + 4 * h;
    auto load = [&](int st, f16x8 (&Bf)[2][NB], int (&cv)[2]) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
#pragma unroll
            for (int c = 0; c < NB; ++c) Bf[u][c] = bsrc[((size_t)(2 * st + u) * nm + c) * 64];
            cv[u] = csrc[(2 * st + u) * 32];
        }
    };
    auto cterms = [](f32x16 &c, int v) {
#define PCR_BC(r) c[r] = __int_as_float(__builtin_amdgcn_mov_dpp(v, 0x150 + (r), 0xf, 0xf, false))
        PCR_BC(0); PCR_BC(1); PCR_BC(2); PCR_BC(3); PCR_BC(4); PCR_BC(5); PCR_BC(6); PCR_BC(7);
        PCR_BC(8); PCR_BC(9); PCR_BC(10); PCR_BC(11); PCR_BC(12); PCR_BC(13); PCR_BC(14); PCR_BC(15);
#undef PCR_BC
    };
    f16x8 Bf[2][NB], Ar[2][NB];
    int cv[2];
    f32x16 acc[2][2];  // [row tile parity][column tile of the step]
    if (wid < nsteps) {
        load(wid, Bf, cv);
#pragma unroll
        for (int c = 0; c < NB; ++c) Ar[0][c] = Asl[c * 64];
    }
    for (int st = wid; st < nsteps; st += W) {
        f32x16 Cf[2];
        cterms(Cf[0], cv[0]);
        cterms(Cf[1], cv[1]);
        f16x8 Bn[2][NB];
        int cn[2];
        load(st + W < nsteps ? st + W : st, Bn, cn);  // (the last step: its own again)
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int cur = t & 1;
#pragma unroll
            for (int c = 0; c < NB; ++c)
#pragma unroll
                for (int u = 0; u < 2; ++u)
                    acc[cur][u] = __builtin_amdgcn_mfma_f32_32x32x16_f16(Bf[u][c], Ar[cur][c],
                                                                         c == 0 ? Cf[u] : acc[cur][u], 0, 0, 0);
#pragma unroll
            for (int c = 0; c < NB; ++c) Ar[cur ^ 1][c] = Asl[(((t + 1) % NT) * NB + c) * 64];
            if (t > 0)
                row9_close(B1[t - 1], B2[t - 1], I[t - 1], group_min32(acc[cur ^ 1][0], acc[cur ^ 1][1]), (unsigned)st);
            // 2 NB MFMAs beside the row tile before's 20 VALU; the next row
            // tile's operand behind the first MFMA (its registers are free then)
            SGB(0x008, 1, 0);
            SGB(0x100, NB, 0);
#pragma unroll
            for (int i = 1; i < 2 * NB; ++i) {
                SGB(0x002, 20 / (2 * NB), 0);
                SGB(0x008, 1, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        // the step's last row tile closes here, not under the next step's first
        // MFMAs: carried round the loop, the compiler moved its 32 accumulators
        // out of the terms' registers behind a wait for the last MFMA
        row9_close(B1[NT - 1], B2[NT - 1], I[NT - 1], group_min32(acc[1][0], acc[1][1]), (unsigned)st);
#pragma unroll
        for (int u = 0; u < 2; ++u) {
#pragma unroll
            for (int c = 0; c < NB; ++c) Bf[u][c] = Bn[u][c];
            cv[u] = cn[u];
        }
    }
    // the waves' triples of a row tile and lane merged, W row tiles per round:
    // round r takes row tiles RT j + r (j = 0 .. W - 1), wave j merges row tile
    // RT j + r over the waves in order
    unsigned *mg = reinterpret_cast<unsigned *>(As) + l;
    unsigned M1[RT], M2[RT], MI[RT];
#pragma unroll
    for (int r = 0; r < RT; ++r) {
        __syncthreads();  // every wave is past its operand reads (r = 0) / the round before's reads
#pragma unroll
        for (int j = 0; j < W; ++j) {
            unsigned *q = mg + (wid * W + j) * 3 * 64;
            q[0] = B1[RT * j + r];
            q[64] = B2[RT * j + r];
            q[128] = I[RT * j + r];
        }
        __syncthreads();
        M1[r] = kRow9Inf; M2[r] = kRow9Inf; MI[r] = 0u;
#pragma unroll
        for (int w = 0; w < W; ++w) {
            const unsigned *q = mg + (w * W + wid) * 3 * 64;
            row9_merge(M1[r], M2[r], MI[r], q[0], q[64], q[128]);
        }
    }
#pragma unroll
    for (int r = 0; r < RT; ++r)
        row9_settle<S, kIdx>(a, p, rl, nr, (rb * NT + wid * RT + r) * 32 + (l & 31), h, M1[r], M2[r], MI[r]);
}

// kIdx: pass 1 / pass 2 (the same code; two names for the profiles).  kForm: 0
// rows stationary, 1 / 2 columns stationary with 4 / 8 waves (two 256-thread
// blocks or one 512-thread block per CU: two waves per SIMD either way)
template <int S, int G, int kForm, bool kIdx>
__global__ __launch_bounds__(kForm == 1 ? 256 : 512) __attribute__((amdgpu_waves_per_eu(kForm ? 2 : 4)))
void featnn_row9(RowArgs5 a) {
    if constexpr (kForm == 0) row9_rows<S, G, kIdx>(a);
    else row9_cols<S, G, kIdx, kForm == 1 ? 4 : 8>(a);
}

// featnn_row9's second half (one launch per pass).  A pair's tiles: each
// bucket's rows in 32-row tiles, in bucket order.  Grid (blocks per pair, P):
// a block puts the pair's tiles-per-bucket prefix in LDS once, its waves take
// tiles w, w + 4 gridDim.x, ... (a few each); one MFMA chain over a tile's
// two column tiles (from the packed image) gives every row of the tile its
// winning group's 32 values again (its operand rebuilt from the f32 row, as
// the sweep built it), and the row's (column, B1, B2) record goes to
// featnn_finish9.  (Run inside the sweep, on a workgroup's own 512 rows, the
// regroup cost more: pass 1 2.0 ms against 1.29 + 0.2 -- ~126 chains of ~4
// rows per workgroup and the registers it kept live.)
template <int S, bool kIdx>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4))) void featnn_regroup9(RowArgs5 a) {
    constexpr int NB = S;
    // the pair's per-step tile prefix and row counts, 2 (steps + 1) ints of
    // dynamic LDS (a static 4097-entry pair held 32 KB and four blocks per CU)
    extern __shared__ int rg_lds[];
    __shared__ int wsum[4];
    const int nst = a.ntc >> 1;
    int *ts = rg_lds, *cn = rg_lds + nst + 1;
    // XCD-aware: a pair's blocks on one XCD (its rows and column image in that L2)
    const int nbp = gridDim.x / (8 * ((a.P + 7) >> 3));  // blocks per pair
    const int bid = blockIdx.x, xcd = bid & 7, slot = bid >> 3;
    const int p = (slot / nbp) * 8 + xcd, bx = slot % nbp;
    if (p >= a.P) return;
    const int t = threadIdx.x, wid = t >> 6, l = t & 63, h = l >> 5;
    const int *bc = a.bcnt + (size_t)p * nst;
    // exclusive prefix of the tiles per bucket: each wave scans a quarter
    const int seg = (nst + 3) >> 2, s0 = min(nst, wid * seg), s1 = min(nst, s0 + seg);
    int run = 0;
    for (int c0 = s0; c0 < s1; c0 += 64) {
        const int i = c0 + l;
        const int ci = i < s1 ? min(bc[i], a.bcap) : 0;
        const int ti = (ci + 31) >> 5;
        int x = ti;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int y = __shfl_up(x, o, 64);
            if (l >= o) x += y;
        }
        if (i < s1) {
            ts[i] = run + x - ti;
            cn[i] = ci;
        }
        run += __shfl(x, 63, 64);
    }
    if (l == 0) wsum[wid] = run;
    __syncthreads();
    int add = 0;
    for (int ww = 0; ww < wid; ++ww) add += wsum[ww];
    for (int i = s0 + l; i < s1; i += 64) ts[i] += add;
    if (t == 0) ts[nst] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
    __syncthreads();
    const int ntiles = ts[nst];
    const int nm = a.ich;  // the image's tile stride in chunks
    const f16x8 *bimg = a.Bp + (size_t)p * a.ntc * nm * 64 + l;
    const float *ctp = a.cct + (size_t)p * a.ntc * 32;
    const uint4 *bl = a.blist + (size_t)p * nst * a.bcap;
    // tile q's bucket, its rows' entries (the next tile's loaded while this one runs)
    auto locate = [&](int q, int &b, bool &valid, uint4 &e) {
        int lo = 0, hi = nst;  // ts[lo] <= q < ts[hi]
        while (hi - lo > 1) {
            const int md = (lo + hi) >> 1;
            if (ts[md] <= q) lo = md;
            else hi = md;
        }
        b = lo;
        const int o = (q - ts[b]) * 32 + (l & 31);
        valid = o < cn[b];
        e = valid ? bl[(size_t)b * a.bcap + o] : make_uint4(0u, 0u, 0u, 0u);
    };
    const int qs = nbp * 4;
    int q = bx * 4 + wid, b = 0;
    bool valid = false;
    uint4 e = make_uint4(0u, 0u, 0u, 0u);
    if (q < ntiles) locate(q, b, valid, e);
    for (; q < ntiles; q += qs) {
        int bn = 0;
        bool vn = false;
        uint4 en = make_uint4(0u, 0u, 0u, 0u);
        if (q + qs < ntiles) locate(q + qs, bn, vn, en);
        const int row = (int)e.x;
        f16x8 Bf[2][NB];
        f32x16 acc[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
#pragma unroll
            for (int c = 0; c < NB; ++c) Bf[u][c] = bimg[((size_t)(2 * b + u) * nm + c) * 64];
            acc[u] = colterms(ctp + (size_t)(2 * b + u) * 32, h);
        }
        f16x8 A[NB];
        row_operand<S, 2>(a, p, row, valid, h, A);
#pragma unroll
        for (int c = 0; c < NB; ++c)
#pragma unroll
            for (int u = 0; u < 2; ++u)
                acc[u] = __builtin_amdgcn_mfma_f32_32x32x16_f16(Bf[u][c], A[c], acc[u], 0, 0, 0);
        if (valid && (int)e.w == h) {
            // the winner's column (the first in column order among equal
            // patterns) and the group's second smallest value
            unsigned t2 = 0xffffffffu;
            int pos = -1;
#pragma unroll
            for (int u = 0; u < 2; ++u)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const unsigned v = fbits(acc[u][r]);
                    const bool hit = pos < 0 && v == e.y;
                    t2 = hit ? t2 : umin2(t2, v);
                    pos = hit ? 32 * (2 * b + u) + 8 * (r >> 2) + 4 * h + (r & 3) : pos;
                }
            // a winner not found again (it cannot be: the same chain) is left uncertified
            const unsigned B2 = pos < 0 ? e.y : umin2(e.z, t2);
            a.rec[(size_t)p * a.Rmax + row] = make_uint4((unsigned)(pos < 0 ? 64 * b : pos), e.y, B2, 0u);
        }
        b = bn; valid = vn; e = en;
    }
}

// the rows' certification and outputs (row_tail) in row order, from the
// regroup's (column, B1, B2) records: coalesced, where the regroup visits rows
// in bucket order.  A record marked 1 is a row the sweep gave to the 3-term
// screen.  A row that fails here -- its winning group's own second value
// closed the gap, rare -- goes to a.llist: pass 1 the exact rescan's list (the
// 3-term screen runs beside this kernel), pass 2 none (the resolve sends a
// column whose top-2 gap is too small to the exact column rescan).  1024 rows per block, the listed ones appended with
// one global atomic per block: one counter per pair, the P counters in a few
// cache lines -- per-row atomics from this short kernel serialised there
// (~4 cycles each, 0.15 ms for C4's 73k rows).
template <int S, bool kIdx>
__global__ __launch_bounds__(256) void featnn_finish9(RowArgs5 a) {
    constexpr int R = 4;
    __shared__ int wcnt[4], base;
    const int p = blockIdx.y, t = threadIdx.x, l = t & 63, w = t >> 6;
    const int *rl = a.rlist ? a.rlist + (size_t)p * a.Rmax : nullptr;
    const int nr = rl ? a.rcount[p] : count_of(a.n_rows, p, a.Rmax);
    const int k0 = blockIdx.x * 256 * R;
    if (k0 >= nr) return;  // whole block
    const int m = count_of(a.n_cols, p, a.Cmax);
    int rows[R];
    bool put[R];
    uint4 rc[R];
#pragma unroll
    for (int i = 0; i < R; ++i) {
        const int k = k0 + i * 256 + t;
        rows[i] = k < nr ? (rl ? rl[k] : k) : -1;
        rc[i] = rows[i] >= 0 ? a.rec[(size_t)p * a.Rmax + rows[i]] : make_uint4(0u, 0u, 0u, 1u);
    }
    int mine = 0;
#pragma unroll
    for (int i = 0; i < R; ++i) {
        put[i] = false;
        if (rc[i].w == 0u)
            put[i] = row_tail<kIdx, true, S, true>(a, p, rows[i], m, rc[i].y, rc[i].z, (int)rc[i].x,
                                                   a.rre[(size_t)p * a.ntr * 32 + rows[i]], 0.0,
                                                   a.rct[(size_t)p * a.ntr * 32 + rows[i]]);
        mine += put[i] ? 1 : 0;
        // the threshold route lists them with the sweep's own: marked alike
        if (put[i] && a.thresh && a.llist)
            a.rec[(size_t)p * a.Rmax + rows[i]] = make_uint4(0u, rc[i].y, 0xffffffffu, 1u);
    }
    // block-wide exclusive offsets of the listed rows
    int x = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int y = __shfl_up(x, o, 64);
        if (l >= o) x += y;
    }
    if (l == 63) wcnt[w] = x;
    __syncthreads();
    if (t == 0) {
        const int tot = wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
        base = tot && a.llist ? atomicAdd(a.lcount + p, tot) : 0;
    }
    __syncthreads();
    if (!a.llist) return;
    int off = base + x - mine;
    for (int ww = 0; ww < w; ++ww) off += wcnt[ww];
#pragma unroll
    for (int i = 0; i < R; ++i)
        if (put[i]) a.llist[(size_t)p * a.Rmax + off++] = rows[i];
}

}  // namespace

// featnn_row7 above D = 32: one row tile per wave (two tiles' accumulators and
// fragments spilled at S = 4: 256 VGPRs + 179 spilled), four column tiles per
// LDS group
constexpr int kRow7RT = 1, kRow7G = 4;

// one row screen launch (pass 1: kIdx, F rows; pass 2: the J rows of G)
template <bool kIdx>
int launch_row7(const RowArgs5 &r0, int S, hipStream_t s) {
    RowArgs5 r = r0;
    PCR_REQUIRE(r.ich == 2 * S + 1, PCR_ERR_ARG, "featnn_row7: needs the full operand image (%d chunks)", r.ich);
    r.nrb = cdiv(cdiv(r.Rmax, 32), 8 * kRow7RT);  // 8 waves x 1 row tile per workgroup
    const long long nblk = 8LL * r.nrb * cdiv(r.P, 8);  // XCD-aware 1-D grid
    PCR_REQUIRE(nblk < (1LL << 31), PCR_ERR_ARG, "feature_match: grid too large");
    const dim3 grid((unsigned)nblk);
    if (S == 3) hipLaunchKernelGGL((featnn_row7<3, kRow7G, kIdx, kRow7RT>), grid, dim3(512), 0, s, r);
    else if (S == 4) hipLaunchKernelGGL((featnn_row7<4, kRow7G, kIdx, kRow7RT>), grid, dim3(512), 0, s, r);
    else { set_error("feature dim too large for the f16 split screen"); return PCR_ERR_ARG; }
    PCR_LAUNCH_CHECK();
    return PCR_OK;
}

// one featnn_row8 launch over a grid for all Rmax rows (list mode: the blocks
// past the pair's count exit at once)
template <bool kIdx, bool kOne>
int launch_row8(const RowArgs5 &r0, int S, hipStream_t s) {
    RowArgs5 r = r0;
    PCR_REQUIRE(r.ich == 2 * S + 1, PCR_ERR_ARG, "featnn_row8: needs the full operand image (%d chunks)", r.ich);
    r.nrb = cdiv(cdiv(r.Rmax, 32), 8 * 2);  // 8 waves x 2 row tiles per workgroup
    const int csl = r.rbmajor ? r.csl : 1;
    const long long nblk = 8LL * r.nrb * csl * cdiv(r.P, 8);  // XCD-aware 1-D grid
    PCR_REQUIRE(nblk < (1LL << 31), PCR_ERR_ARG, "feature_corres: grid too large");
    if (S == 1) hipLaunchKernelGGL((featnn_row8<1, kRow8G, kIdx, kOne>), dim3((unsigned)nblk), dim3(512), 0, s, r);
    else hipLaunchKernelGGL((featnn_row8<2, kRow8G, kIdx, kOne>), dim3((unsigned)nblk), dim3(512), 0, s, r);
    PCR_LAUNCH_CHECK();
    if (csl > 1) {
        const dim3 mg(cdiv(r.Rmax, 256), r.P);
        if (S == 1) hipLaunchKernelGGL((featnn_slicemerge<1, kIdx>), mg, dim3(256), 0, s, r);
        else hipLaunchKernelGGL((featnn_slicemerge<2, kIdx>), mg, dim3(256), 0, s, r);
        PCR_LAUNCH_CHECK();
    }
    return PCR_OK;
}

// The sweep's form per pass (kIdx / !kIdx): 0 rows stationary, 1 / 2 columns
// stationary with 4 / 8 waves.  Chosen per pass by measurement (DESIGN.md
// Round 12), as KL is: C4, featnn_bench alone, pass 1 1.06 / 0.93 / 1.13 ms and
// pass 2 0.54 / 0.47 / 0.57 ms for forms 0 / 1 / 2
#ifndef PCR_ROW9_FORM1
#define PCR_ROW9_FORM1 1
#endif
#ifndef PCR_ROW9_FORM2
#define PCR_ROW9_FORM2 1
#endif
constexpr int kRow9Form1 = PCR_ROW9_FORM1, kRow9Form2 = PCR_ROW9_FORM2;

template <bool kIdx>
int launch_row9(const RowArgs5 &r0, int S, hipStream_t s) {
    RowArgs5 r = r0;
    PCR_REQUIRE(r.ich == S || r.ich == 2 * S + 1, PCR_ERR_ARG, "featnn_row9: image of %d chunks per tile", r.ich);
    r.nrb = cdiv(cdiv(r.Rmax, 32), 8 * 2);  // 8 waves x 2 row tiles per workgroup
    const long long nblk = 8LL * r.nrb * cdiv(r.P, 8);  // XCD-aware 1-D grid
    PCR_REQUIRE(nblk < (1LL << 31), PCR_ERR_ARG, "feature_corres: grid too large");
    constexpr int G = kIdx ? kRow9G1 : kRow9G;
    // PCR_ROW9_SWEEP=rows|cols|cols8: the sweep's form (an A/B and parity
    // switch, read on every call); unset: the default of the pass
    int form = kIdx ? kRow9Form1 : kRow9Form2;
    if (const char *e = getenv("PCR_ROW9_SWEEP")) {
        if (!strcmp(e, "rows")) form = 0;
        else if (!strcmp(e, "cols")) form = 1;
        else if (!strcmp(e, "cols8")) form = 2;
    }
    const dim3 grid((unsigned)nblk);
#define PCR_ROW9_LAUNCH(S_)                                                                                     \
    do {                                                                                                        \
        if (form == 0) hipLaunchKernelGGL((featnn_row9<S_, G, 0, kIdx>), grid, dim3(512), 0, s, r);             \
        else if (form == 1) hipLaunchKernelGGL((featnn_row9<S_, G, 1, kIdx>), grid, dim3(256), 0, s, r);        \
        else hipLaunchKernelGGL((featnn_row9<S_, G, 2, kIdx>), grid, dim3(512), 0, s, r);                       \
    } while (0)
    if (S == 1) PCR_ROW9_LAUNCH(1);
    else PCR_ROW9_LAUNCH(2);
#undef PCR_ROW9_LAUNCH
    PCR_LAUNCH_CHECK();
    return PCR_OK;
}

template <bool kIdx>
int launch_regroup9(const RowArgs5 &r, int S, hipStream_t s) {
    // a pair has at most one tile per 32 rows plus one per bucket: ~6 per
    // wave (PCR_REGROUP_TPB: tiles per 4-wave block; 4 / 6 / 12 / 24 measured
    // 0.36 / 0.34 / 0.30 / 0.29 ms per C4 step); 1-D, a pair's blocks on one XCD
    static const int tpb = [] {
        const char *e = getenv("PCR_REGROUP_TPB");
        const int v = e ? atoi(e) : 24;
        return v >= 4 ? v : 24;
    }();
    const int nbp = cdiv(cdiv(r.Rmax, 32) + r.ntc / 2, tpb);
    const dim3 grid((unsigned)(8LL * nbp * cdiv(r.P, 8)));
    const dim3 fgrid(cdiv(r.Rmax, 1024), r.P);
    const size_t sm = sizeof(int) * (2 * (size_t)(r.ntc / 2) + 1);
    if (S == 1) {
        hipLaunchKernelGGL((featnn_regroup9<1, kIdx>), grid, dim3(256), sm, s, r);
        hipLaunchKernelGGL((featnn_finish9<1, kIdx>), fgrid, dim3(256), 0, s, r);
    } else {
        hipLaunchKernelGGL((featnn_regroup9<2, kIdx>), grid, dim3(256), sm, s, r);
        hipLaunchKernelGGL((featnn_finish9<2, kIdx>), fgrid, dim3(256), 0, s, r);
    }
    PCR_LAUNCH_CHECK();
    return PCR_OK;
}

// the device address of g_featnn_fallback_rows (featnn_thresh.hip counts there too)
int fallback_counter(unsigned long long **ctr) {
    PCR_HIP_CHECK(hipGetSymbolAddress((void **)ctr, HIP_SYMBOL(g_featnn_fallback_rows)));
    return PCR_OK;
}

template int launch_row7<true>(const RowArgs5 &, int, hipStream_t);
template int launch_row7<false>(const RowArgs5 &, int, hipStream_t);
template int launch_row8<true, true>(const RowArgs5 &, int, hipStream_t);
template int launch_row8<true, false>(const RowArgs5 &, int, hipStream_t);
template int launch_row8<false, true>(const RowArgs5 &, int, hipStream_t);
template int launch_row8<false, false>(const RowArgs5 &, int, hipStream_t);
template int launch_row9<true>(const RowArgs5 &, int, hipStream_t);
template int launch_row9<false>(const RowArgs5 &, int, hipStream_t);
template int launch_regroup9<true>(const RowArgs5 &, int, hipStream_t);
template int launch_regroup9<false>(const RowArgs5 &, int, hipStream_t);

}  // namespace pcr

extern "C" int pcr_featnn_fallback_rows(int64_t *rows12, int64_t *cols21, int32_t reset) {
    pcr::clear_error();
    unsigned long long v[2] = {0, 0};
    PCR_HIP_CHECK(hipDeviceSynchronize());
    PCR_HIP_CHECK(hipMemcpyFromSymbol(v, HIP_SYMBOL(pcr::g_featnn_fallback_rows), sizeof(v)));
    if (rows12) *rows12 = (int64_t)v[0];
    if (cols21) *cols21 = (int64_t)v[1];
    if (reset) {
        const unsigned long long z[2] = {0, 0};
        PCR_HIP_CHECK(hipMemcpyToSymbol(HIP_SYMBOL(pcr::g_featnn_fallback_rows), z, sizeof(z)));
    }
    return PCR_OK;
}
