// The dual screen (pcr_feature_match, D <= 64): both directions' top-2 out of
// one launch over the packed images (featnn_v5.h, featnn_pack.hip), the column
// partials' merge, then the exact rescan of what neither certified.
#include "featnn_v5.h"

namespace pcr {
namespace {

// raw v_min / v_med3 on bit-packed values: as builtins the compiler inserts a
// NaN canonicalisation (v_max x,x) per packed operand.  Inputs are never
// signalling NaNs; a quiet NaN (NaN feature) is ignored by IEEE min, as the
// oracle's strict < ignores it, or forces a rescan.
// NEVER feed an MFMA accumulator straight into these: the compiler does not
// place the MFMA read-after-write wait states in front of inline asm, and the
// first registers read come back without the chain's last MFMA (measured:
// featnn_row7 with asm reads of acc).  Here every operand comes from a
// compiler-visible instruction (the index pack).
__device__ __forceinline__ float vmin(float a, float b) {
    float d;
    asm("v_min_f32 %0, %1, %2" : "=v"(d) : "v"(a), "v"(b));
    return d;
}
// a NaN operand yields the other value: the pair's second value then equals its
// first (a tie), which only fails certification (exact rescan)
__device__ __forceinline__ float vmax(float a, float b) {
    float d;
    asm("v_max_f32 %0, %1, %2" : "=v"(d) : "v"(a), "v"(b));
    return d;
}
__device__ __forceinline__ float vmed3(float a, float b, float c) {
    float d;
    asm("v_med3_f32 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "v"(c));
    return d;
}

// ---------------------------------------------------------------------------
// v7 = v5 with an in-wave software pipeline.  Ablations of v5 showed its
// phases add: MFMA chain (after its B-fragment LDS reads have landed) and
// the VALU epilogue never overlap.  Here iteration g of a group issues, in one
// scheduling region, the 7 MFMAs of tile g, the ds_read_b128 B fragments of
// tile g+1 (register double buffer) and the epilogue of tile g-1, interleaved
// 1 MFMA : 1 LDS read : V VALU by sched_group_barrier.  G = 8 tiles per LDS
// group halves the barriers (B double buffer 2 x 57 KB + partials 32 KB).
// ---------------------------------------------------------------------------
template <int S, int G>
__global__ __launch_bounds__(512) void featnn_dual7(DualArgs5 a) {
    constexpr int W = 8;  // waves per workgroup, one 32-row tile each
    constexpr int NX = 3 * S + 1, NM = 2 * S + 1;  // executed / stored k-chunks
    constexpr int kB = G * NM * 64;  // f16x8 per B buffer
    constexpr int kP = G * W * 32;
    __shared__ __attribute__((aligned(16))) char smem[2 * kB * 16 + 2 * 2 * kP * 4];
    // column partials first: their per-tile stores then fit the ds_write
    // immediate offset (below 64 KiB), the B buffers follow
    float *Pc1 = reinterpret_cast<float *>(smem);  // [2][G][W waves][32 cols]
    float *Pc2 = Pc1 + 2 * kP;
    f16x8 *Bs = reinterpret_cast<f16x8 *>(smem + 2 * 2 * kP * 4);
    const int b = blockIdx.x, xcd = b & 7, slot = b >> 3;
    const int p = (slot / a.nrb) * 8 + xcd, rb = slot - (slot / a.nrb) * a.nrb;
    if (p >= a.P) return;  // whole block
    const int wid = threadIdx.x >> 6, l = threadIdx.x & 63, h = l >> 5;
    const int n = count_of(a.n_src, p, a.Nmax), m = count_of(a.n_tgt, p, a.Mmax);
    const int qt = rb * W + wid;
    const int ntc = (m + 31) >> 5;
    const int ngroups = (ntc + G - 1) / G;
    const unsigned ctmask = (1u << a.ctbits) - 1u;
    unsigned keep_r = ~ctmask;
    asm("" : "+v"(keep_r));
    unsigned ccode[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        ccode[r] = (unsigned)((wid << 5) | (h << 4) | r);
        asm("" : "+v"(ccode[r]));
    }
    f16x8 A[NM];
    const f16x8 *qp = a.Ap + ((size_t)p * a.ntn + qt) * NM * 64 + l;
#pragma unroll
    for (int c = 0; c < NM; ++c) A[c] = qp[(size_t)c * 64];
    float b1[16], b2[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) { b1[r] = __builtin_inff(); b2[r] = __builtin_inff(); }

    const f16x8 *bsrc = a.Bp + (size_t)p * a.ntm * NM * 64 + l;
    auto issue = [&](int grp, int bufi) {
        for (int c = wid; c < G * NM; c += W) {
            const f16x8 *src = bsrc + ((size_t)grp * G * NM + c) * 64;
            __builtin_amdgcn_global_load_lds(
                (const __attribute__((address_space(1))) void *)src,
                (__attribute__((address_space(3))) void *)(Bs + bufi * kB + c * 64), 16, 0, 0);
        }
    };
    auto epilogue = [&](const f32x16 &acc, unsigned ct, int pbase, int pe) {
        asm("" : "+s"(ct));
        float c1[2], c2[2];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const unsigned ub = __float_as_uint(acc[r]);
            const float vr = __uint_as_float((ub & keep_r) | ct);
            const float vc = __uint_as_float((ub & 0xFFFFFF00u) | ccode[r]);
            b2[r] = vmed3(b1[r], b2[r], vr);
            b1[r] = vmin(b1[r], vr);
            // column top-2 of the lane's 16 values in two interleaved chains
            // (one merge; no +inf staged: the first two values give min / max)
            const int q = r & 1;
            if (r < 2) {
                c1[q] = vc;
            } else if (r < 4) {
                c2[q] = vmax(c1[q], vc);
                c1[q] = vmin(c1[q], vc);
            } else {
                c2[q] = vmed3(c1[q], c2[q], vc);
                c1[q] = vmin(c1[q], vc);
            }
        }
        {
            const float m2 = vmin(c2[0], c2[1]);
            c2[0] = vmed3(c1[0], c1[1], m2);
            c1[0] = vmin(c1[0], c1[1]);
        }
        // merge with the other half-wave without LDS (a ds_bpermute here would share
        // lgkmcnt with the B-fragment reads in flight).  One swap of (c1, c2)
        // leaves lanes 0-31 with (own c1, other c1) and lanes 32-63 with
        // (own c2, other c2): their min is the new c1 below and min(c2, c2')
        // above, which a second swap brings down for the med3 -- 5 VALU, where
        // swapping c1 and c2 separately needed 4 copies more.
        const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(c1[0]),
                                                         __float_as_uint(c2[0]), false, false);
        const float lo = __uint_as_float(sw[0]), up = __uint_as_float(sw[1]);
        const float mm = vmin(lo, up);
        const auto sw2 = __builtin_amdgcn_permlane32_swap(__float_as_uint(mm), __float_as_uint(mm),
                                                          false, false);
        c2[0] = vmed3(lo, up, __uint_as_float(sw2[1]));
        c1[0] = __uint_as_float(sw2[0]);  // lanes 0-31 of the swapped mm: mm itself
        if (h == 0) {
            const int e = pbase + pe * (W * 32);  // pe: compile-time tile of the group
            Pc1[e] = c1[0];
            Pc2[e] = c2[0];
        }
    };
    const size_t cpoff = ((size_t)p * a.nrb + rb) * (size_t)a.ntm * 32;
    issue(0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    for (int grp = 0; grp < ngroups; ++grp) {
        const int buf = grp & 1;
        if (grp + 1 < ngroups) issue(grp + 1, buf ^ 1);
        const f16x8 *Bb = Bs + buf * kB + l;
        const int pbase = buf * (G * W * 32) + wid * 32 + l;  // this group's column partials
        f16x8 Bf[2][NM];
        f32x16 acc[2];
#pragma unroll
        for (int c = 0; c < NM; ++c) Bf[0][c] = Bb[c * 64];
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const int cur = g & 1;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[cur][r] = 0.0f;
#pragma unroll
            for (int c = 0; c < NX; ++c)
                acc[cur] = __builtin_amdgcn_mfma_f32_32x32x16_f16(A[amap(c, S)], Bf[cur][bmap(c, S)], acc[cur],
                                                                  0, 0, 0);
            if (g + 1 < G) {
#pragma unroll
                for (int c = 0; c < NM; ++c) Bf[cur ^ 1][c] = Bb[((g + 1) * NM + c) * 64];
            }
            if (g > 0) epilogue(acc[cur ^ 1], (unsigned)(grp * G + g - 1), pbase, g - 1);
            // one region per iteration: MFMA : LDS read : VALU = 1 : 1 : 18
#pragma unroll
            for (int c = 0; c < NX; ++c) {
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                if (g + 1 < G && c < NM) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
                if (g > 0) __builtin_amdgcn_sched_group_barrier(0x002, 18, 0);
            }
        }
        epilogue(acc[(G - 1) & 1], (unsigned)(grp * G + G - 1), pbase, G - 1);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        const int t = threadIdx.x;
        if (t < G * 32) {
            const int g = t >> 5, col = t & 31, ct = grp * G + g;
            if (ct < ntc) {
                const int e0 = (buf * G + g) * (W * 32) + col;
                float m1 = Pc1[e0], mm2 = Pc2[e0];
#pragma unroll
                for (int w = 1; w < W; ++w) {
                    const float o1 = Pc1[e0 + 32 * w], o2 = Pc2[e0 + 32 * w];
                    const float t2 = vmin(mm2, o2);
                    mm2 = vmed3(m1, o1, t2);
                    m1 = vmin(m1, o1);
                }
                // no row index stored: featnn_colmerge5 decodes it from m1's
                // code bits (a third fewer column-partial bytes written and read)
                const size_t o = cpoff + (size_t)ct * 32 + col;
                a.cp1[o] = m1;
                a.cp2[o] = mm2;
            }
        }
    }
    if (qt * 32 >= n) return;
    int i1[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) i1[r] = (int)(__float_as_uint(b1[r]) & ctmask) * 32 + (l & 31);
#pragma unroll
    for (int o = 1; o < 32; o <<= 1) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float ob1 = __shfl_xor(b1[r], o, 64);
            const float ob2 = __shfl_xor(b2[r], o, 64);
            const int oi1 = __shfl_xor(i1[r], o, 64);
            top2_merge(b1[r], i1[r], b2[r], ob1, oi1, ob2);
        }
    }
    const int lr = l & 31;
    if (lr >= 16) return;
    float mb1 = 0.f, mb2 = 0.f;
    int mi1 = 0;
#pragma unroll
    for (int r = 0; r < 16; ++r)
        if (lr == r) { mb1 = b1[r]; mb2 = b2[r]; mi1 = i1[r]; }
    const int row = qt * 32 + (lr & 3) + 8 * (lr >> 2) + 4 * h;
    if (row >= n) return;
    if (m == 0) { a.nn12[(size_t)p * a.Nmax + row] = 0; return; }
    a.nn12[(size_t)p * a.Nmax + row] = mi1;
    const double Gm = (double)__uint_as_float(a.gmax[p]);
    const double qn = (double)a.fnr[(size_t)p * a.ntn * 32 + row];
    const double pert = __builtin_ldexp(1.0, a.ctbits - 23) *
                        (__builtin_fabs((double)mb1) + __builtin_fabs((double)mb2));
    if (!((double)mb2 - (double)mb1 > bound5(qn, Gm, 16 * NX, a.D) + pert))
        a.list12[(size_t)p * a.Nmax + atomicAdd(a.count12 + p, 1)] = row;
}

__global__ void featnn_colmerge5(DualArgs5 a, int32_t *nn21, int *list21, int *count21, int Kt,
                                 int W) {
    const int p = blockIdx.y;
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    const int m = count_of(a.n_tgt, p, a.Mmax);
    if (j >= m) return;
    const int n = count_of(a.n_src, p, a.Nmax);
    if (n == 0) { nn21[(size_t)p * a.Mmax + j] = 0; return; }
    const int nrb_used = (((n + 31) >> 5) + 7) >> 3;
    float b1 = __builtin_inff(), b2 = __builtin_inff();
    int i1 = 0;
    for (int rb = 0; rb < nrb_used; ++rb) {
        const size_t o = ((size_t)p * a.nrb + rb) * (size_t)a.ntm * 32 + j;
        // row index of the partial's winner from its code bits (wave, half,
        // register), as the screen kernels packed them
        const float v1 = a.cp1[o];
        const unsigned code = __float_as_uint(v1) & (unsigned)(W * 32 - 1);
        const int r = code & 15;
        const int vi = rb * (W * 32) + (int)(code >> 5) * 32 + (int)((code >> 4) & 1) * 4 + (r & 3) + 8 * (r >> 2);
        top2_merge(b1, i1, b2, v1, vi, a.cp2[o]);
    }
    nn21[(size_t)p * a.Mmax + j] = i1;
    const double F = (double)__uint_as_float(a.fmax[p]);
    const double gn = (double)a.gnr[(size_t)p * a.ntm * 32 + j];
    const double pert = 3.0517578125e-05 /* 2^-15: 8-bit row code */ *
                        (__builtin_fabs((double)b1) + __builtin_fabs((double)b2));
    if (!((double)b2 - (double)b1 > bound5(gn, F, Kt, a.D) + pert))
        list21[(size_t)p * a.Mmax + atomicAdd(count21 + p, 1)] = j;
}

}  // namespace

int feature_match_v5(const float *F, const float *G, int P, int Nmax, int Mmax, int D,
                            const int32_t *n_src, const int32_t *n_tgt, int32_t *nn12,
                            int32_t *nn21, hipStream_t s) {
    V5Buf v;
    int rc = v5_prepare(F, G, P, Nmax, Mmax, D, n_src, n_tgt, s, v);
    if (rc != PCR_OK) return rc;
    PCR_REQUIRE(v.ich == v.NM, PCR_ERR_ARG, "feature_match: the dual screen needs the full operand image");
    const V5Side &f = v.side[0], &g = v.side[1];
    const int W = v.W, nrb = v.nrb, ntm = g.nt;
    DualArgs5 d;
    d.Ap = f.Xp; d.Bp = g.Xp; d.fnr = f.nr; d.gnr = g.nr; d.fmax = f.nmax; d.gmax = g.nmax;
    d.n_src = n_src; d.n_tgt = n_tgt; d.P = P; d.Nmax = Nmax; d.Mmax = Mmax; d.ntn = f.nt;
    d.ntm = ntm; d.nrb = nrb; d.D = D; d.nn12 = nn12; d.list12 = v.list12;
    d.count12 = v.cnt12;
    // the dual screen's row code: column tiles only
    d.ctbits = 1;
    while ((1 << d.ctbits) < ntm) ++d.ctbits;
    const size_t cpn = (size_t)P * nrb * ntm * 32;
    WsLayout l;
    l.take(d.cp1, cpn);
    l.take(d.cp2, cpn);
    PCR_REQUIRE(workspace_bind(kWsFeatDualCols, l, kWsSlack), PCR_ERR_NOMEM, "feature_match: %s", pcr_last_error());
    d.cpi = nullptr;
    const long long nblk = 8LL * nrb * cdiv(P, 8);  // XCD-aware 1-D grid
    PCR_REQUIRE(nblk < (1LL << 31), PCR_ERR_ARG, "feature_match: grid too large");
    prof_begin(s, kProfFeatScreen);
    {
        switch (v.S) {
#define PCR_D7CASE(K)                                                                        \
    case K:                                                                                  \
        hipLaunchKernelGGL((featnn_dual7<K, (K <= 2 ? 8 : 4)>), dim3((unsigned)nblk),          \
                           dim3(512), 0, s, d);                                              \
        break;
            PCR_D7CASE(1) PCR_D7CASE(2) PCR_D7CASE(3) PCR_D7CASE(4)
#undef PCR_D7CASE
            default: set_error("feature dim too large for the f16 split screen"); return PCR_ERR_ARG;
        }
    }
    PCR_LAUNCH_CHECK();
    prof_end(s, kProfFeatScreen);
    hipLaunchKernelGGL(featnn_colmerge5, dim3(cdiv(Mmax, 256), P), dim3(256), 0, s, d, nn21, v.list21,
                       v.cnt21, 16 * v.NX, W);
    PCR_LAUNCH_CHECK();
    RescanArgs5 ra = rescan_args(F, G, n_src, n_tgt, Nmax, Mmax, D);
    ra.list12 = v.list12; ra.list21 = v.list21; ra.cnt12 = v.cnt12; ra.cnt21 = v.cnt21;
    ra.nn12 = nn12; ra.nn21 = nn21;
    return run_rescan(ra, P, D, s);
}

}  // namespace pcr
