// The exact f64 rescan of the rows / columns the screens could not certify
// (both feature_match_v5 and feature_corres_v5 end in it).
#include "featnn_v5.h"
#include <stdlib.h>
#include <algorithm>
#include <cstdio>
#include <vector>

namespace pcr {
namespace {

// exact f64 rescan of v5's per-pair ambiguous lists: one 256-thread block per
// batch of R listed rows of one pair and direction; the rows sit in LDS as
// f64, every thread streams candidates j = tid + 256 i once (float4 rows) and
// keeps R running minima, so a pair's candidate cloud is read once per batch
// instead of once per row.  blockIdx.z = direction (0: F->G, 1: G->F).
// rows sent to the exact rescan since the last reset (diagnostic, pcr_featnn_rescan_rows)
__device__ unsigned long long g_featnn_rescan_rows[2];

__device__ __forceinline__ void rescan_out(const RescanArgs5 &a, int dir, int p, int row, double best,
                                           int bj, int32_t *nn) {
    nn[row] = (bj == 0x7fffffff) ? 0 : bj;
    if (dir == 0 && a.v12) {
        const double sc = (double)__uint_as_float(a.mx[p]);  // the scale the packs used
        a.v12[(size_t)p * a.Nmax + row] = best * sc * sc;
        a.e12[(size_t)p * a.Nmax + row] = 0.0f;
    }
}

typedef float f2v __attribute__((ext_vector_type(2)));

template <int DV, bool V4>
__global__ __launch_bounds__(256) void featnn_rescan3(RescanArgs5 a) {
    // thread (row r = tid>>3, slice sl = tid&7): row r of the current batch of
    // 32 listed rows (held as f64 in registers) against candidates sl, sl+8,
    // ... of each 128-candidate chunk staged in LDS.  Row stride DV+4 floats:
    // the 8 slices' ds_read_b128 hit disjoint banks, the rows of a slice
    // broadcast.  Dims in [D, DV) are zero on both sides (exact zero terms).
    constexpr int kChunk = 128, kSt = DV + 4;
    __shared__ __attribute__((aligned(16))) float csb[2][kChunk * kSt];  // double buffer (V4 path)
    const int dir = blockIdx.y, p = blockIdx.x, S = gridDim.z, sid = blockIdx.z;
    const int tid = threadIdx.x, r = tid >> 3, sl = tid & 7;
    const float *Q = dir ? a.G : a.F;
    const float *C = dir ? a.F : a.G;
    const int Nq = dir ? a.Mmax : a.Nmax, Nc = dir ? a.Nmax : a.Mmax;
    const int ncand = count_of(dir ? a.n_src : a.n_tgt, p, Nc);
    const int *list = (dir ? a.list21 : a.list12) + (size_t)p * Nq;
    const int cnt = (dir ? a.cnt21 : a.cnt12)[p];
    if (tid == 0 && sid == 0 && cnt > 0) atomicAdd(&g_featnn_rescan_rows[dir], (unsigned long long)cnt);
    int32_t *nn = (dir ? a.nn21 : a.nn12) + (size_t)p * Nq;
    const int D = a.D;
    const float *cb = C + (size_t)p * Nc * D;
    // this slice's candidates: whole 128-candidate chunks [clo, chi)
    const int nchunk = (ncand + kChunk - 1) / kChunk;
    const int clo = S > 1 ? min(ncand, (int)((long long)nchunk * sid / S) * kChunk) : 0;
    const int chi = S > 1 ? min(ncand, (int)((long long)nchunk * (sid + 1) / S) * kChunk) : ncand;
    const int ecap = S > 1 ? min(cnt, a.cap) : 0;  // rows handled by the slices
    // slices take rows [0, ecap); slice 0 also the rows past the cap, whole
    for (int b0 = 0; b0 < (sid > 0 ? ecap : cnt); b0 += 32) {
        const bool sliced = b0 < ecap;
        const int c_lo = sliced ? clo : 0, c_hi = sliced ? chi : ncand;
        const int bend = sliced ? ecap : cnt;
        const bool act = b0 + r < bend;
        const int row = act ? list[b0 + r] : 0;
        const float *q = Q + ((size_t)p * Nq + row) * D;
        double qd[DV];
        float qf[DV];
#pragma unroll
        for (int k = 0; k < DV; ++k) {
            qf[k] = k < D ? q[k] : 0.0f;
            qd[k] = (double)qf[k];
        }
        double best = __builtin_inf();
        int bj = 0x7fffffff;
        float m32 = __builtin_inff();
        const float kRel = 1.0f + 3.0f * (float)(D + 5) * 5.9604644775390625e-08f;
        // candidate chunk -> registers -> LDS; with V4 the next chunk's global
        // loads are in flight while the current chunk is scanned
        constexpr int kPer = kChunk * (DV / 4) / 256;  // float4 per thread per chunk
        float4 stage[kPer];
        auto gload = [&](int c0, int cend) {
#pragma unroll
            for (int u = 0; u < kPer; ++u) {
                const int e = tid + 256 * u, i = e / (DV / 4), k = (e - i * (DV / 4)) * 4;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (c0 + i < cend && k < D)
                    v = *reinterpret_cast<const float4 *>(cb + (size_t)(c0 + i) * D + k);
                stage[u] = v;
            }
        };
        auto lstore = [&](float *cs) {
#pragma unroll
            for (int u = 0; u < kPer; ++u) {
                const int e = tid + 256 * u, i = e / (DV / 4), k = (e - i * (DV / 4)) * 4;
                *reinterpret_cast<float4 *>(cs + i * kSt + k) = stage[u];
            }
        };
        auto scan = [&](const float *cs, int c0, int ncand) {
            // f32 screen of the thread's kChunk / 8 candidates (packed: two
            // dims per v_pk_fma): all terms are >= 0, so |d32 - d| <= (D+3) u d
            // whatever the order; only candidates within kRel of the thread's
            // running f32 minimum after the chunk (>= the global one) can be
            // the exact winner.  Those are re-ranked in f64 AFTER the chunk's
            // screen, in candidate order (first index on ties): a wave runs
            // one or two f64 ranks per chunk instead of one wherever any lane
            // had a running-minimum candidate (~a quarter of the steps).
            constexpr int kPer8 = kChunk / 8;
            float a32v[kPer8];
#pragma unroll
            for (int t = 0; t < kPer8; ++t) {
                const int i = sl + 8 * t;
                float a32 = __builtin_inff();
                if (i < ncand) {
                    const float *cp = cs + i * kSt;
                    f2v acc = {0.0f, 0.0f};
#pragma unroll
                    for (int k = 0; k < DV; k += 4) {
                        const float4 v = *reinterpret_cast<const float4 *>(cp + k);
                        const f2v d0 = f2v{v.x, v.y} - f2v{qf[k], qf[k + 1]};
                        const f2v d1 = f2v{v.z, v.w} - f2v{qf[k + 2], qf[k + 3]};
                        acc = __builtin_elementwise_fma(d0, d0, acc);
                        acc = __builtin_elementwise_fma(d1, d1, acc);
                    }
                    a32 = acc.x + acc.y;
                }
                a32v[t] = a32;
                m32 = fminf(m32, a32);
            }
            const float lim = m32 * kRel + 1e-30f;
            unsigned pend = 0;
#pragma unroll
            for (int t = 0; t < kPer8; ++t) pend |= (sl + 8 * t < ncand && a32v[t] <= lim ? 1u : 0u) << t;
            while (pend) {
                const int t = __builtin_ctz(pend);
                pend &= pend - 1;
                const int i = sl + 8 * t;
                const float *cp = cs + i * kSt;
                double acc = 0.0;
#pragma unroll
                for (int k = 0; k < DV; k += 4) {
                    const float4 v = *reinterpret_cast<const float4 *>(cp + k);
                    double df = qd[k] - (double)v.x;
                    acc = acc + df * df;
                    df = qd[k + 1] - (double)v.y;
                    acc = acc + df * df;
                    df = qd[k + 2] - (double)v.z;
                    acc = acc + df * df;
                    df = qd[k + 3] - (double)v.w;
                    acc = acc + df * df;
                }
                if (acc < best) { best = acc; bj = c0 + i; }
            }
        };
        if (V4) {
            __syncthreads();  // previous batch done with both buffers
            if (c_lo < c_hi) {
                gload(c_lo, c_hi);
                lstore(csb[0]);
            }
            __syncthreads();
            int buf = 0;
            for (int c0 = c_lo; c0 < c_hi; c0 += kChunk, buf ^= 1) {
                const bool more = c0 + kChunk < c_hi;
                if (more) gload(c0 + kChunk, c_hi);
                scan(csb[buf], c0, min(kChunk, c_hi - c0));
                if (more) lstore(csb[buf ^ 1]);  // read last in the previous iteration
                __syncthreads();
            }
        } else {
            for (int c0 = c_lo; c0 < c_hi; c0 += kChunk) {
                const int nin = min(kChunk, c_hi - c0);
                __syncthreads();  // previous chunk fully consumed
                for (int e = tid; e < kChunk * DV; e += 256) {
                    const int i = e / DV, k = e - i * DV;
                    csb[0][i * kSt + k] = (i < nin && k < D) ? cb[(size_t)(c0 + i) * D + k] : 0.0f;
                }
                __syncthreads();
                scan(csb[0], c0, nin);
            }
        }
#pragma unroll
        for (int o = 1; o < 8; o <<= 1) {
            const double ob = __shfl_xor(best, o, 64);
            const int oj = __shfl_xor(bj, o, 64);
            if (ob < best || (ob == best && oj < bj)) { best = ob; bj = oj; }
        }
        if (sl == 0 && act) {
            if (sliced) {
                const size_t slot = (((size_t)p * 2 + dir) * a.cap + b0 + r) * S + sid;
                a.sd[slot] = best;
                a.sj[slot] = bj;
            } else {
                rescan_out(a, dir, p, row, best, bj, nn);
            }
        }
    }
}

// lexicographic (d, j) minimum of the S slice results of each sliced row
__global__ __launch_bounds__(256) void featnn_rescan_merge(RescanArgs5 a, int S) {
    const int dir = blockIdx.y, p = blockIdx.x;
    const int Nq = dir ? a.Mmax : a.Nmax;
    const int cnt = min((dir ? a.cnt21 : a.cnt12)[p], a.cap);
    const int *list = (dir ? a.list21 : a.list12) + (size_t)p * Nq;
    int32_t *nn = (dir ? a.nn21 : a.nn12) + (size_t)p * Nq;
    for (int e = threadIdx.x; e < cnt; e += 256) {
        const size_t slot = (((size_t)p * 2 + dir) * a.cap + e) * S;
        double best = a.sd[slot];
        int bj = a.sj[slot];
        for (int s = 1; s < S; ++s) {
            const double d = a.sd[slot + s];
            const int j = a.sj[slot + s];
            if (d < best || (d == best && j < bj)) { best = d; bj = j; }
        }
        rescan_out(a, dir, p, list[e], best, bj, nn);
    }
}

}  // namespace

RescanArgs5 rescan_args(const float *F, const float *G, const int32_t *n_src,
                               const int32_t *n_tgt, int Nmax, int Mmax, int D) {
    RescanArgs5 ra;
    ra.F = F; ra.G = G; ra.n_src = n_src; ra.n_tgt = n_tgt; ra.Nmax = Nmax; ra.Mmax = Mmax;
    ra.D = D;
    ra.list12 = ra.list21 = nullptr;
    ra.cnt12 = ra.cnt21 = nullptr;
    ra.nn12 = ra.nn21 = nullptr;
    ra.cap = 256;
    ra.sd = nullptr;
    ra.sj = nullptr;
    ra.v12 = nullptr; ra.e12 = nullptr; ra.mx = nullptr; ra.T = 0;
    return ra;
}

// exact f64 rescan of the listed rows of both directions (a direction with a
// zero count costs its empty blocks only)
int run_rescan(RescanArgs5 &ra, int P, int D, hipStream_t s) {
    const bool v4 = (D % 4) == 0 && ((uintptr_t)ra.F & 15) == 0 && ((uintptr_t)ra.G & 15) == 0;
    // candidate slices per (pair, direction): ~8192 blocks whatever the batch --
    // a pair's list is short (C4: 27 rows on average, 45 at most, one or two
    // 32-row batches), so a block is a short chain of dependent candidate
    // loads and more, shorter slices finish sooner (256 pairs: 4 / 8 / 16
    // slices 0.575 / 0.489 / 0.471 ms per step)
    const int S = std::max(1, std::min(16, 4096 / std::max(P, 1)));
    if (S > 1) {
        WsLayout l;
        l.take(ra.sd, (size_t)P * 2 * ra.cap * S);
        l.take(ra.sj, (size_t)P * 2 * ra.cap * S);
        PCR_REQUIRE(workspace_bind(kWsFeatRescan, l, kWsSlack), PCR_ERR_NOMEM, "feature_match: %s", pcr_last_error());
    }
    const dim3 rg(P, 2, S);
    if (getenv("PCR_RESCAN_DEBUG")) {  // diagnostic: the per-pair list lengths (host sync)
        for (int d = 0; d < 2; ++d) {
            const int *c = d ? ra.cnt21 : ra.cnt12;
            if (!c) continue;
            std::vector<int> h((size_t)P);
            PCR_HIP_CHECK(hipMemcpyAsync(h.data(), c, sizeof(int) * (size_t)P, hipMemcpyDeviceToHost, s));
            PCR_HIP_CHECK(hipStreamSynchronize(s));
            long long tot = 0;
            int mx = 0, over = 0;
            for (int v : h) { tot += v; mx = std::max(mx, v); over += v > ra.cap ? 1 : 0; }
            std::sort(h.begin(), h.end());
            fprintf(stderr, "rescan dir %d: rows %lld, max %d, p50 %d, p90 %d, p99 %d, pairs over cap %d\n", d, tot,
                    mx, h[P / 2], h[(P * 9) / 10], h[(P * 99) / 100], over);
        }
    }
    prof_begin(s, kProfFeatRescan);
    const int dv = cdiv(D, 16) * 16;
#define PCR_R3(DVV)                                                                    \
    if (dv == DVV) {                                                                    \
        if (v4) hipLaunchKernelGGL((featnn_rescan3<DVV, true>), rg, dim3(256), 0, s, ra); \
        else hipLaunchKernelGGL((featnn_rescan3<DVV, false>), rg, dim3(256), 0, s, ra);  \
    }
    PCR_R3(16) PCR_R3(32) PCR_R3(48) PCR_R3(64)
#undef PCR_R3
    PCR_LAUNCH_CHECK();
    if (S > 1) {
        hipLaunchKernelGGL(featnn_rescan_merge, dim3(P, 2), dim3(256), 0, s, ra, S);
        PCR_LAUNCH_CHECK();
    }
    prof_end(s, kProfFeatRescan);
    return PCR_OK;
}

}  // namespace pcr

extern "C" int pcr_featnn_rescan_rows(int64_t *rows12, int64_t *rows21, int32_t reset) {
    pcr::clear_error();
    unsigned long long v[2] = {0, 0};
    PCR_HIP_CHECK(hipDeviceSynchronize());
    PCR_HIP_CHECK(hipMemcpyFromSymbol(v, HIP_SYMBOL(pcr::g_featnn_rescan_rows), sizeof(v)));
    if (rows12) *rows12 = (int64_t)v[0];
    if (rows21) *rows21 = (int64_t)v[1];
    if (reset) {
        const unsigned long long z[2] = {0, 0};
        PCR_HIP_CHECK(hipMemcpyToSymbol(HIP_SYMBOL(pcr::g_featnn_rescan_rows), z, sizeof(z)));
    }
    return PCR_OK;
}
