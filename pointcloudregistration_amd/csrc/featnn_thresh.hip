// The leftover rows of the 1-term screens settled from threshold candidates
// (DESIGN.md Round 9): featnn_thresh9, then featnn_exact_cand.
//
// A row the 1-term screen (featnn_row9 / featnn_regroup9 / featnn_finish9)
// could not certify has its smallest screened value B1 and its certificate
// bound bnd = 2 e, e the error of one screened value in the row's frame.  The
// exact argmin j* then has a screened value
//     v(j*) <= d(j*) + e <= d(j1) + e <= v(j1) + 2 e = B1 + bnd
// (d the exact value in the row's frame, j1 the column of B1), and so has
// every column that ties with it exactly: the columns with v <= B1 + bnd are a
// complete candidate set, two per failing row on average.  featnn_thresh9 runs
// the screen's MFMA chain once more over the listed rows -- the same operands
// in the same order, so the same value bits, and B1 is found again exactly --
// with one unsigned compare per value against the row's threshold pattern, and
// appends the hits to the row's kThreshK slots.  featnn_exact_cand ranks a
// row's candidates by the rescan's f64 distance.  A row with more than kThreshK
// hits, or without a finite B1, goes to the exact rescan as before.
#include "featnn_v5.h"
#include "featnn_thresh.h"
#include <stdlib.h>
#include <algorithm>
#include <cstdio>
#include <type_traits>

namespace pcr {
namespace {

// per pass (0: pass 1): listed rows, the largest candidate count, rows left to
// the exact rescan -- kept when PCR_THRESH_DEBUG is set
__device__ unsigned g_thresh_stat[2][3];

// A block is one of a pair's column slices (steps of two column tiles, as the
// regroup's chain) and walks it in rounds of W * RT = 16 row tiles of the
// pair's list: wave w holds tiles w and w + 8 of the round, so a list of up
// to 8 tiles has one tile on each of its waves and every SIMD has work (two
// consecutive tiles per wave left 3 of 8 waves idle at C4's 9 tiles).
//
// The column stream goes through LDS as featnn_row9's: kThreshG column tiles
// per group -- the f16 chunks by 16-byte and the column terms by 4-byte LDS
// DMA -- double-buffered, the next group in flight while this one runs; the
// waves read their B fragments and C terms from the group's buffer.  A slice
// is whole steps, not whole groups: the DMA leaves out the tiles past the
// slice's last step (the compute never reads them).
//
// Hits go to LDS: a counter and kThreshK slots per row of the round.  A hit
// is one returning ds_add and a conditional ds_write (lgkmcnt), so the step
// loop has no vector-memory instruction of its own and nothing waits on the
// DMA in flight (one returning global atomic per hit drained it: vmcnt counts
// in order -- DESIGN.md Round 10).  After the slice the block adds each row's
// local count to rec.x once and copies the local slots that land below
// kThreshK (thresh_flush_count); rec.x ends as the sum of all counted hits, as
// before, so "more than kThreshK" still means overflow.  The hits of different
// slices append independently: no merge.  A pair's blocks sit on one XCD (its
// column image in that L2).
#ifndef PCR_THRESH_G
#define PCR_THRESH_G 16
#endif
#ifndef PCR_THRESH_PF
#define PCR_THRESH_PF 1  // the next step's fragments read from LDS behind this step's MFMAs
#endif
constexpr int kThreshG = PCR_THRESH_G;  // column tiles per LDS group

// A hit's returning LDS add and LDS store, by their LDS byte addresses.  As
// inline asm because the compiler puts s_waitcnt vmcnt(0) in front of every
// LDS access of its own that it cannot tie to one of the LDS DMAs in flight --
// the hit lists are no DMA's target, so each hit would wait for the next
// group's DMA, which is what this kernel is rid of.  Their operands are
// addresses and column numbers, never an MFMA's accumulators (whose hazard
// wait states the compiler does not place around inline asm).
__device__ __forceinline__ unsigned lds_add_rtn(unsigned addr, unsigned v) {
    unsigned r;
    asm volatile("ds_add_rtn_u32 %0, %1, %2\n\ts_waitcnt lgkmcnt(0)" : "=v"(r) : "v"(addr), "v"(v) : "memory");
    return r;
}
__device__ __forceinline__ void lds_store(unsigned addr, int v) {
    asm volatile("ds_write_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)" : : "v"(addr), "v"(v) : "memory");
}

template <int S, bool kIdx>
__global__ __launch_bounds__(512) void featnn_thresh9(RowArgs5 a) {
    constexpr int NB = S, W = 8, RT = 2, G = kThreshG, GS = G / 2;
    constexpr int kT = G * NB * 64;     // f16x8 of a buffer's fragments
    constexpr int kRows = W * RT * 32;  // rows of a block round: one per thread
    static_assert(G % 2 == 0 && kRows == 512, "whole steps; the flush is one row per thread");
    // the two buffers' fragments and column terms (G x 32 floats) as arrays of
    // their own, each named at compile time where it is read or filled: the
    // compiler then knows that a read of one does not touch the DMA in flight
    // into another (behind a run-time choice of one array's parts it waits
    // for every DMA before the reads)
    __shared__ __attribute__((aligned(16))) f16x8 Bs0[kT];
    __shared__ __attribute__((aligned(16))) f16x8 Bs1[kT];
    __shared__ __attribute__((aligned(16))) float Cs0[G * 32];
    __shared__ __attribute__((aligned(16))) float Cs1[G * 32];
    __shared__ unsigned hcnt[kRows];
    __shared__ int hslot[kRows * kThreshK];
    const int nbp = gridDim.x / (8 * ((a.P + 7) >> 3));  // blocks per pair
    const int bid = blockIdx.x, xcd = bid & 7, slot = bid >> 3;
    const int p = (slot / nbp) * 8 + xcd, sl = slot % nbp;
    if (p >= a.P) return;
    const int nr = min(a.rcount[p], a.Rmax);
    const int m = count_of(a.n_cols, p, a.Cmax);
    const int nst = (((m + 31) >> 5) + 1) >> 1;  // column steps (2 nst <= ntc: ntc is even)
    const int nsl = min(nbp, nst);
    if (nr <= 0 || sl >= nsl) return;  // whole block
    const int s0 = (int)((long long)nst * sl / nsl), s1 = (int)((long long)nst * (sl + 1) / nsl);
    const int ngr = (s1 - s0 + GS - 1) / GS;  // the slice's groups, the last one short
    const int wid = threadIdx.x >> 6, l = threadIdx.x & 63, h = l >> 5;
    const int ntl = (nr + 31) >> 5;
    const int *rl = a.rlist + (size_t)p * a.Rmax;
    const int nm = a.ich;  // the image's tile stride in chunks
    const f16x8 *bimg = a.Bp + (size_t)p * a.ntc * nm * 64 + l;
    const float *ctp = a.cct + (size_t)p * a.ntc * 32 + l;
    // group grp of the slice into buffer bufi: tiles [2 sg, 2 min(sg + GS, s1))
    // (all below 2 nst <= ntc: inside the pair's image and terms)
    auto issue = [&](auto bufc_, int grp) {
        f16x8 *Bs = decltype(bufc_)::value ? Bs1 : Bs0;
        float *Cs = decltype(bufc_)::value ? Cs1 : Cs0;
        const int sg = s0 + grp * GS;
        for (int c = wid; c < G * NB + GS; c += W) {
            if (c >= G * NB) {  // a step's column terms: two tiles, 4 B per lane
                const int j = c - G * NB;
                if (sg + j < s1)
                    __builtin_amdgcn_global_load_lds(
                        (const __attribute__((address_space(1))) void *)(ctp + (size_t)(sg + j) * 64),
                        (__attribute__((address_space(3))) void *)(Cs + j * 64),
                        4, 0, 0);
                continue;
            }
            const int g = c / NB, cc = c - g * NB;
            if (sg + (g >> 1) < s1)
                __builtin_amdgcn_global_load_lds(
                    (const __attribute__((address_space(1))) void *)(bimg + ((size_t)(2 * sg + g) * nm + cc) * 64),
                    (__attribute__((address_space(3))) void *)(Bs + c * 64), 16, 0, 0);
        }
    };
    // min of a lane's values x[8 q .. 8 q + 7] of one column tile (featnn_row9's chains)
    auto min8 = [](const f32x16 &x, int q) {
        unsigned c = umin2(umin2(fbits(x[8 * q]), fbits(x[8 * q + 1])), fbits(x[8 * q + 2]));
        c = umin2(umin2(c, fbits(x[8 * q + 3])), fbits(x[8 * q + 4]));
        c = umin2(umin2(c, fbits(x[8 * q + 5])), fbits(x[8 * q + 6]));
        return umin2(c, fbits(x[8 * q + 7]));
    };
    for (int tb = 0; tb < ntl; tb += W * RT) {
        // (the previous round's flush is behind a barrier; the hits of this one
        // come after the first group's)
        hcnt[threadIdx.x] = 0u;
        issue(std::integral_constant<int, 0>{}, 0);
        // the wave's row tiles tb + wid and tb + wid + 8
        const int nt = tb + wid + W < ntl ? 2 : (tb + wid < ntl ? 1 : 0);
        size_t o[RT];
        unsigned B1[RT], thr[RT], am[RT];
        bool live[RT];
        int nh[RT], lr[RT];
        unsigned ca[RT], sa[RT];  // the LDS addresses of the row's counter and slots
        f16x8 A[RT][NB];
#pragma unroll
        for (int t = 0; t < RT; ++t) {
            lr[t] = (t * W + wid) * 32 + (l & 31);  // the row's slot of the round
            ca[t] = (unsigned)(uintptr_t)(hcnt + lr[t]);
            sa[t] = (unsigned)(uintptr_t)(hslot + lr[t] * kThreshK);
            const int k = tb * 32 + lr[t];
            const bool valid = k < nr;
            const int row = valid ? rl[k] : 0;
            o[t] = (size_t)p * a.Rmax + row;
            B1[t] = valid ? a.rec[o[t]].y : 0x7f800000u;
            // the row's threshold pattern; a row without a finite one has no
            // hits (it stays at zero candidates: the exact rescan's)
            thr[t] = 0u;
            live[t] = false;
            if (valid && B1[t] < 0x7f800000u) {
                const double bnd = row_bound_ct(a, p, row, a.rre[(size_t)p * a.ntr * 32 + row], 16 * S);
                thr[t] = thresh_bits_up((double)__uint_as_float(B1[t]) + bnd * (1.0 + 0x1p-20));
                live[t] = thr[t] < 0x7f800000u;
            }
            row_operand<S, 3>(a, p, row, valid, h, A[t]);
            am[t] = 0xffffffffu;  // pass 1: the first column whose value is B1
            nh[t] = 0;            // this lane's hits in this slice
        }
        // one group of the slice for the wave's NT row tiles
        auto sweep = [&](auto ntc_, auto bufc_, int grp) {
            constexpr int NT = decltype(ntc_)::value;
            const f16x8 *Bs = decltype(bufc_)::value ? Bs1 : Bs0;
            const float *Cb = decltype(bufc_)::value ? Cs1 : Cs0;
            const int sg = s0 + grp * GS, ns = min(GS, s1 - sg);
            const f16x8 *Bb = Bs + l;
            auto load = [&](int j, f16x8 (&Bf)[2][NB], f32x16 (&Cf)[2]) {
#pragma unroll
                for (int u = 0; u < 2; ++u) {
#pragma unroll
                    for (int c = 0; c < NB; ++c) Bf[u][c] = Bb[((2 * j + u) * NB + c) * 64];
                    Cf[u] = colterms(Cb + (2 * j + u) * 32, h);
                }
            };
            f16x8 Bf[2][NB];
            f32x16 Cf[2];
            if (PCR_THRESH_PF) load(0, Bf, Cf);
            for (int j = 0; j < ns; ++j) {
                const int st = sg + j;
                f16x8 Bn[2][NB];
                f32x16 Cn[2];
                if (PCR_THRESH_PF) load(j + 1 < ns ? j + 1 : j, Bn, Cn);
                else load(j, Bf, Cf);
                f32x16 acc[NT][2];
#pragma unroll
                for (int c = 0; c < NB; ++c)
#pragma unroll
                    for (int u = 0; u < 2; ++u)
#pragma unroll
                        for (int t = 0; t < NT; ++t)
                            acc[t][u] = __builtin_amdgcn_mfma_f32_32x32x16_f16(Bf[u][c], A[t][c],
                                                                               c == 0 ? Cf[u] : acc[t][u], 0, 0, 0);
#pragma unroll
                for (int t = 0; t < NT; ++t)
#pragma unroll
                    for (int u = 0; u < 2; ++u) {
                        // one compare of the lane's smallest value against the
                        // row's threshold; a dead lane's pattern is 0, below
                        // every value.  A wave's 32 rows have ~64 hits in 256
                        // column tiles: three tiles of four skip the scan, and
                        // the others scan the half of the registers with the hit
                        const unsigned m0 = min8(acc[t][u], 0), m1 = min8(acc[t][u], 1);
                        if (__ballot(umin2(m0, m1) <= thr[t]) == 0ull) continue;
                        const bool half[2] = {__ballot(m0 <= thr[t]) != 0ull, __ballot(m1 <= thr[t]) != 0ull};
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            if (!half[r >> 3]) continue;
                            const unsigned v = fbits(acc[t][u][r]);
                            const int col = 32 * (2 * st + u) + 8 * (r >> 2) + 4 * h + (r & 3);
                            if (v <= thr[t] && live[t] && col < m) {
                                if (kIdx && v == B1[t]) am[t] = umin2(am[t], (unsigned)col);
                                // past kThreshK + 1 hits of its own the lane stops counting: the row overflows
                                if (nh[t] <= kThreshK) {
                                    const unsigned pos = lds_add_rtn(ca[t], 1u);
                                    if (pos < (unsigned)kThreshK) lds_store(sa[t] + 4u * pos, col);
                                }
                                ++nh[t];
                            }
                        }
                    }
                if (PCR_THRESH_PF) {
#pragma unroll
                    for (int u = 0; u < 2; ++u) {
#pragma unroll
                        for (int c = 0; c < NB; ++c) Bf[u][c] = Bn[u][c];
                        Cf[u] = Cn[u];
                    }
                }
            }
        };
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        auto group = [&](auto bufc_, int grp) {
            constexpr int buf = decltype(bufc_)::value;
            if (grp + 1 < ngr) issue(std::integral_constant<int, buf ^ 1>{}, grp + 1);
            if (nt == 2) sweep(std::integral_constant<int, 2>{}, bufc_, grp);
            else if (nt == 1) sweep(std::integral_constant<int, 1>{}, bufc_, grp);
            // the next group's DMA has landed for every wave, and every wave is done
            // reading this buffer before the group after next overwrites it
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
        };
        for (int grp = 0; grp < ngr; grp += 2) {
            group(std::integral_constant<int, 0>{}, grp);
            if (grp + 1 < ngr) group(std::integral_constant<int, 1>{}, grp + 1);
        }
#pragma unroll
        for (int t = 0; t < RT; ++t)
            if (kIdx && am[t] != 0xffffffffu) atomicMin(reinterpret_cast<unsigned *>(a.rec + o[t]) + 2, am[t]);
        // the flush (every wave's hits are behind the last group's barrier):
        // thread r takes row slot r of the round
        {
            const int r = threadIdx.x, k = tb * 32 + r;
            const unsigned lc = hcnt[r];
            if (k < nr && lc != 0u) {
                const size_t oo = (size_t)p * a.Rmax + rl[k];
                const unsigned base = atomicAdd(reinterpret_cast<unsigned *>(a.rec + oo), lc);
                const int n = thresh_flush_count(base, lc, kThreshK);
                for (int i = 0; i < n; ++i) a.cand[oo * kThreshK + base + i] = hslot[r * kThreshK + i];
            }
        }
        __syncthreads();  // the next round clears the counters
    }
}

// The exact decision of each listed row from its candidates: the rescan's f64
// distance (df = (double)q[k] - (double)c[k], acc = acc + df * df, k ascending,
// from the f32 inputs), the lexicographic (distance, column) minimum.
//   pass 1: nn, v = best * sc^2 and e = 0 as the rescan's outputs, and nns, the
//           row's screened argmin (the first column whose value is B1: J is
//           built from it); a row that overflowed is appended to llist;
//   pass 2: the column's exact argmin to nn (nn21x) and used 1 -> 2, with a
//           non-finite bound in wq: featmut_resolve leaves the candidates of
//           such a column undecided without listing it again, and
//           featmut_corres reads nn21x.  A column that overflowed keeps used = 1
//           under the same wq: the resolve lists it for the exact column rescan.
// Eight lanes per listed row, one per candidate slot (a thread per row walking
// its candidates one after the other was a chain of dependent loads: 0.34 ms
// for pass 1 of C4); their results meet by three exchanges.
template <int DV, bool kIdx>
__global__ __launch_bounds__(256) void featnn_exact_cand(RowArgs5 a) {
    const int p = blockIdx.y;
    const int nr = min(a.rcount[p], a.Rmax);
    if (nr <= 0) return;
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(a.fbctr + (kIdx ? 0 : 1), (unsigned long long)nr);
    const int m = count_of(a.n_cols, p, a.Cmax);
    const int *rl = a.rlist + (size_t)p * a.Rmax;
    const int c = threadIdx.x & 7, rr = threadIdx.x >> 3, D = a.D;
    const float4 open = make_float4(__builtin_inff(), __builtin_inff(), __builtin_inff(), 0.0f);
    // (the bounds are the block's: every lane takes part in the exchanges)
    for (int k0 = blockIdx.x * 32; k0 < nr; k0 += gridDim.x * 32) {
        const bool act = k0 + rr < nr;
        const int row = act ? rl[k0 + rr] : 0;
        const size_t o = (size_t)p * a.Rmax + row;
        const uint4 rc = act ? a.rec[o] : make_uint4(0u, 0x7f800000u, 0u, 1u);
        const int cnt = (int)min(rc.x, (unsigned)kThreshK + 1u);
        double best = __builtin_inf();
        int bj = 0x7fffffff;
        if (act && m > 0 && c < cnt && cnt <= kThreshK && rc.y < 0x7f800000u) {
            const int j = a.cand[o * kThreshK + c];
            const float *q = a.Xr + o * D, *y = a.Xc + ((size_t)p * a.Cmax + j) * D;
            float qf[DV], yf[DV];  // zero past D: exact zero terms, as the rescan's
            if (D == DV && (((uintptr_t)q | (uintptr_t)y) & 15) == 0) {
#pragma unroll
                for (int k = 0; k < DV; k += 4) {
                    const float4 u = *reinterpret_cast<const float4 *>(q + k), w = *reinterpret_cast<const float4 *>(y + k);
                    qf[k] = u.x; qf[k + 1] = u.y; qf[k + 2] = u.z; qf[k + 3] = u.w;
                    yf[k] = w.x; yf[k + 1] = w.y; yf[k + 2] = w.z; yf[k + 3] = w.w;
                }
            } else {
#pragma unroll
                for (int k = 0; k < DV; ++k) {
                    qf[k] = k < D ? q[k] : 0.0f;
                    yf[k] = k < D ? y[k] : 0.0f;
                }
            }
            double acc = 0.0;
#pragma unroll
            for (int k = 0; k < DV; ++k) {
                const double df = (double)qf[k] - (double)yf[k];
                acc = acc + df * df;
            }
            if (acc < best) { best = acc; bj = j; }  // (a NaN or infinite distance is no candidate)
        }
#pragma unroll
        for (int x = 1; x < 8; x <<= 1) {
            const double ob = __shfl_xor(best, x, 64);
            const int oj = __shfl_xor(bj, x, 64);
            if (ob < best || (ob == best && oj < bj)) { best = ob; bj = oj; }
        }
        if (c != 0 || !act) continue;
        if (m == 0) {  // no column: row_tail's outputs
            if constexpr (kIdx) {
                a.nn[o] = 0;
                a.nns[o] = 0;
                a.v[o] = __builtin_inf();
                a.e[o] = 0.0f;
            } else {
                a.wq[o] = open;
            }
            continue;
        }
        if constexpr (kIdx) a.nns[o] = rc.z < (unsigned)m ? (int)rc.z : 0;
        const bool over = bj == 0x7fffffff;  // too many candidates, none, or no finite distance
        if (a.dbg) {
            atomicAdd(&g_thresh_stat[kIdx ? 0 : 1][0], 1u);
            atomicMax(&g_thresh_stat[kIdx ? 0 : 1][1], rc.x);
            if (over) atomicAdd(&g_thresh_stat[kIdx ? 0 : 1][2], 1u);
        }
        if constexpr (kIdx) {
            if (over) {
                a.llist[(size_t)p * a.Rmax + atomicAdd(a.lcount + p, 1)] = row;
            } else {
                const double sc = (double)__uint_as_float(a.sc[p]);  // the scale the packs used
                a.nn[o] = bj;
                a.v[o] = best * sc * sc;
                a.e[o] = 0.0f;
            }
        } else {
            a.wq[o] = open;
            if (!over) {
                a.nn[o] = bj;
                a.used[(size_t)p * (a.Rmax + 1) + row] = 2;
            }
        }
    }
}

}  // namespace

// blocks (column slices) per pair of featnn_thresh9: ~256 blocks whatever the
// batch, one per CU -- 1 slice at 256 pairs, 8 at 32 pairs, 32 at 8 pairs and
// below (PCR_THRESH_SLICES: A/B, DESIGN.md Round 10 has the measurements)
static int thresh_blocks_per_pair(int P) {
    static const int forced = [] {
        const char *e = getenv("PCR_THRESH_SLICES");
        return e ? atoi(e) : 0;
    }();
    if (forced >= 1 && forced <= 128) return forced;
    return std::max(1, std::min(32, 256 / std::max(P, 1)));
}

template <bool kIdx>
int launch_thresh9(const RowArgs5 &r0, int S, hipStream_t s) {
    RowArgs5 r = r0;
    static const bool dbg = getenv("PCR_THRESH_DEBUG") != nullptr;
    r.dbg = dbg ? 1 : 0;
    int rc = fallback_counter(&r.fbctr);
    if (rc != PCR_OK) return rc;
    const int nbp = thresh_blocks_per_pair(r.P);
    const dim3 grid((unsigned)(8LL * nbp * cdiv(r.P, 8)));
    if (S == 1) hipLaunchKernelGGL((featnn_thresh9<1, kIdx>), grid, dim3(512), 0, s, r);
    else hipLaunchKernelGGL((featnn_thresh9<2, kIdx>), grid, dim3(512), 0, s, r);
    PCR_LAUNCH_CHECK();
    const dim3 eg(std::min(8, cdiv(r.Rmax, 32)), r.P);  // 32 rows per block and turn
    if (S == 1) hipLaunchKernelGGL((featnn_exact_cand<16, kIdx>), eg, dim3(256), 0, s, r);
    else hipLaunchKernelGGL((featnn_exact_cand<32, kIdx>), eg, dim3(256), 0, s, r);
    PCR_LAUNCH_CHECK();
    if (dbg) {  // diagnostic (host sync): the pass's statistics since the last print
        unsigned st[2][3];
        PCR_HIP_CHECK(hipStreamSynchronize(s));
        PCR_HIP_CHECK(hipMemcpyFromSymbol(st, HIP_SYMBOL(g_thresh_stat), sizeof(st)));
        const int d = kIdx ? 0 : 1;
        fprintf(stderr, "thresh pass %d: listed %u, max candidates %u, to the exact rescan %u\n", d + 1, st[d][0],
                st[d][1], st[d][2]);
        const unsigned z[3] = {0, 0, 0};
        PCR_HIP_CHECK(hipMemcpyToSymbol(HIP_SYMBOL(g_thresh_stat), z, sizeof(z), sizeof(z) * d));
    }
    return PCR_OK;
}

template int launch_thresh9<true>(const RowArgs5 &, int, hipStream_t);
template int launch_thresh9<false>(const RowArgs5 &, int, hipStream_t);

}  // namespace pcr
