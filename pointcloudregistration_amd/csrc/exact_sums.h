// The exact-sum reduction that the ICP kernels share (icp.hip: 15 Umeyama sums,
// icp_plane.hip: 27 normal-equation sums), templated on the number of sums NQ.
// Every summand is an integer multiple of a per-pair quantum and every partial
// sum stays below 2^52 quanta, so the f64 additions are exact and the tree shape
// -- lanes, waves, workgroups -- is free: any split gives the same bits.
//
// A kernel's LDS header SH provides
//   double ws[waves][NQ]; u64 wacc[waves]; int wcnt[waves];
//   double tot[NQ]; u64 acc; int cnt; int nred;
// with waves = blockDim.x / 64 (read off wcnt's extent).
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>
#include "coop.h"

namespace pcr {

// one workgroup's partial of a reduction (G > 1): HBM slot per (pair, parity, g)
template <int NQ>
struct XPart {
    double s[NQ];
    unsigned long long acc;
    int cnt, pad;
};

// The working copy when a pair has G > 1 workgroups: each pair barrier's
// release fence writes back the XCD L2's dirty lines, and a sweep dirtied ~48 KB
// of working copy per workgroup (2,048 points x 24 B at 32 pairs, G = 4).
// Stored write-through (sc1: the line leaves L2 clean) there is nothing of it to
// write back; visibility is still the barrier's release / acquire.
__device__ __forceinline__ void put3(double *q, double x, double y, double z, bool wt) {
    if (wt) {
        __hip_atomic_store(q, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(q + 1, y, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(q + 2, z, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else {
        q[0] = x; q[1] = y; q[2] = z;
    }
}

// wave-level sums of the NQ exact f64 values (integer multiples of the quantum:
// the additions are exact, so the tree shape is free), parked in
// sh.ws[wave][0..NQ).  A reduce-scatter butterfly over NP = 16 or 32 padded
// values: at each of the offsets 32, 16, ... a lane keeps half of its values and
// adds its partner's copy of that half (NP - 1 shuffles instead of 6 per value),
// then the offsets left below 64 / NP finish the one value left -- lane l ends
// with value l / (64 / NP) summed over the wave, which wave_scatter_sum returns.
template <int NQ>
__device__ __forceinline__ double wave_scatter_sum(const double *v) {
    static_assert(NQ >= 1 && NQ <= 32, "wave_scatter_sum: at most 32 sums");
    constexpr int NP = NQ <= 16 ? 16 : 32, kStep = 64 / NP;  // lanes per value at the end
    const int lane = threadIdx.x & 63;
    double w[NP];
#pragma unroll
    for (int q = 0; q < NP; ++q) w[q] = q < NQ ? v[q] : 0.0;
    auto step = [&](auto hc) {
        constexpr int h = decltype(hc)::value, o = kStep * h;
        const bool up = (lane & o) != 0;  // keeps the upper half
#pragma unroll
        for (int i = 0; i < h; ++i) {
            const double keep = up ? w[i + h] : w[i], send = up ? w[i] : w[i + h];
            w[i] = keep + __shfl_xor(send, o, 64);
        }
    };
    if constexpr (NP == 32) step(std::integral_constant<int, 16>{});
    step(std::integral_constant<int, 8>{});
    step(std::integral_constant<int, 4>{});
    step(std::integral_constant<int, 2>{});
    step(std::integral_constant<int, 1>{});
    double t = w[0];
#pragma unroll
    for (int o = kStep / 2; o >= 1; o >>= 1) t += __shfl_xor(t, o, 64);
    return t;
}
// park a lane's value of wave_scatter_sum (or a sum of several, one per chunk of
// a sweep: the additions are exact): the lane bits above log2(kStep) picked the
// half at each offset, the highest bit first, so lane l holds value l / kStep
template <int NQ, typename SH>
__device__ __forceinline__ void wave_park_lane(SH &sh, double t) {
    constexpr int kStep = 64 / (NQ <= 16 ? 16 : 32);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int q = lane / kStep;
    if ((lane & (kStep - 1)) == 0 && q < NQ) sh.ws[wid][q] = t;
}
template <int NQ, typename SH>
__device__ __forceinline__ void wave_park(SH &sh, const double *v) {
    wave_park_lane<NQ>(sh, wave_scatter_sum<NQ>(v));
}

// sum the NV parked values + (cnt, acc) over the pair's G workgroups (partials
// in part, barrier words at bar: both only read when G > 1); result in
// sh.tot / sh.cnt / sh.acc (all threads call; ends with a barrier)
// mk(ph): debug phase clocks: 5 = the workgroup's waves joined, 6 = the pair
// barrier passed
template <int NV, typename SH, typename Mark>
__device__ void pair_reduce(XPart<NV> *part, unsigned *bar, SH &sh, int p, int g, int G, int cnt,
                            unsigned long long acc, Mark mk) {
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    constexpr int waves = (int)(sizeof(sh.wcnt) / sizeof(sh.wcnt[0]));
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        cnt += __shfl_xor(cnt, o, 64);
        acc += __shfl_xor(acc, o, 64);
    }
    if (lane == 0) {
        sh.wcnt[wid] = cnt;
        sh.wacc[wid] = acc;
    }
    __syncthreads();
    mk(5);
    if (tid < NV + 2) {  // thread q sums quantity q (NV: count, NV+1: error sum)
        double s = 0.0;
        unsigned long long A = 0;
        int C = 0;
        for (int w = 0; w < waves; ++w) {
            if (tid < NV) s += sh.ws[w][tid];
            else if (tid == NV) C += sh.wcnt[w];
            else A += sh.wacc[w];
        }
        if (G > 1) {
            XPart<NV> &me = part[((size_t)p * 2 + (sh.nred & 1)) * G + g];
            if (tid < NV) me.s[tid] = s;
            else if (tid == NV) me.cnt = C;
            else me.acc = A;
        } else {
            if (tid < NV) sh.tot[tid] = s;
            else if (tid == NV) sh.cnt = C;
            else sh.acc = A;
        }
    }
    if (G > 1) {
        pair_barrier(bar + 4 * (size_t)p, G);
        mk(6);
        if (tid < NV + 2) {
            const XPart<NV> *all = part + ((size_t)p * 2 + (sh.nred & 1)) * G;
            double s = 0.0;
            unsigned long long A = 0;
            int C = 0;
            for (int h = 0; h < G; ++h) {
                if (tid < NV) s += all[h].s[tid];
                else if (tid == NV) C += all[h].cnt;
                else A += all[h].acc;
            }
            if (tid < NV) sh.tot[tid] = s;
            else if (tid == NV) sh.cnt = C;
            else sh.acc = A;
        }
    }
    __syncthreads();
    if (tid == 0) sh.nred += 1;  // read only by threads < NV + 2 after the next barrier
}

}  // namespace pcr
