// The finalize rule of the whole-cloud norms (groupmlp.hip, unary.hip, pointwise.hip): the
// tiles' f64 partials of sum y and sum y^2 into the f32 coefficients a, b of
// h = fmaf(y, a, b).  One definition, so every unit adds in the same order.
// Header only; HIP units only.  The kernel has internal linkage: each unit that
// includes it carries its own copy of the same code.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>

namespace pcr {

constexpr int kFinThreads = 64;
constexpr int kFinDepth = 32;   // partials a norm_finalize lane has in flight
constexpr int kFinRuns = 16;    // waves of a norm_finalize workgroup: runs of consecutive tiles

struct FinArgs {
    const double *part;  // (b, tiles, C, 2)
    const float *gamma, *beta;  // (C) or null
    float *coef;         // (b, C, 2)
    double *stats;       // (b, C / g, 2): mean, var; or null
    double count, eps;   // values per channel and cloud
    int tiles, C, g;
};

// A channel's sums over the tiles of cloud b, for the kFinThreads * kFinRuns threads of a workgroup whose
// lane `lane` of every wave owns channel c (in: c exists).  Ends with the sums in wave 0's lanes; the other
// waves get their own run's.  One __syncthreads().
static __device__ __forceinline__ void fin_channel_sums(const FinArgs &a, int b, int c, bool in, int lane, int run,
                                                        double2 (*runs)[kFinThreads], double &s, double &ss) {
    s = 0.0; ss = 0.0;
    if (in) {
        // wave `run` adds its run of ceil(tiles / 16) consecutive tiles in ascending order, 32 independent
        // loads in flight per lane (one dependent load per tile made this walk a third of the call)
        const int len = (a.tiles + kFinRuns - 1) / kFinRuns, t1 = min(a.tiles, (run + 1) * len);
        const double2 *p = reinterpret_cast<const double2 *>(a.part) + (size_t)b * a.tiles * a.C + c;
        for (int t0 = run * len; t0 < t1; t0 += kFinDepth) {
            double2 v[kFinDepth];
#pragma unroll
            for (int i = 0; i < kFinDepth; ++i) v[i] = p[(size_t)min(t0 + i, t1 - 1) * a.C];
#pragma unroll
            for (int i = 0; i < kFinDepth; ++i)
                if (t0 + i < t1) {
                    s += v[i].x;
                    ss += v[i].y;
                }
        }
    }
    runs[run][lane] = make_double2(s, ss);
    __syncthreads();
    if (run != 0) return;
    s = 0.0; ss = 0.0;
    for (int r = 0; r < kFinRuns; ++r) {  // the runs' sums in run order
        s += runs[r][lane].x;
        ss += runs[r][lane].y;
    }
}

// mean and variance of cnt values into the f32 coefficients of channel c of cloud b
static __device__ __forceinline__ void fin_coef(const FinArgs &a, int b, int c, double mean, double var) {
    const double a64 = (a.gamma ? (double)a.gamma[c] : 1.0) * (1.0 / sqrt(var + a.eps));
    const double b64 = (a.beta ? (double)a.beta[c] : 0.0) - mean * a64;
    float *cf = a.coef + ((size_t)b * a.C + c) * 2;
    cf[0] = (float)a64;
    cf[1] = (float)b64;
}

// grid (ceil(C / 64), b), kFinThreads * kFinRuns threads.  g = 32 needs C a multiple of 32.
static __global__ __launch_bounds__(kFinThreads * kFinRuns) void norm_finalize(FinArgs a) {
    __shared__ double2 runs[kFinRuns][kFinThreads];
    const int lane = threadIdx.x & 63, c = blockIdx.x * kFinThreads + lane, b = blockIdx.y;
    const int run = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const bool in = c < a.C;
    double s, ss;
    fin_channel_sums(a, b, c, in, lane, run, runs, s, ss);
    if (run != 0) return;
    double cnt = a.count;
    if (a.g == 32) {  // the group's 32 channels sit in one lane half: summed over channels ascending
        const int base = lane & 32;
        double gs = 0.0, gss = 0.0;
        for (int j = 0; j < 32; ++j) {
            gs += __shfl(s, base + j, 64);
            gss += __shfl(ss, base + j, 64);
        }
        s = gs; ss = gss; cnt *= 32.0;
    }
    if (!in) return;
    const double mean = s / cnt;
    double var = ss / cnt - mean * mean;
    if (!(var > 0.0)) var = 0.0;
    fin_coef(a, b, c, mean, var);
    if (a.stats && (a.g == 1 || (lane & 31) == 0)) {
        double *st = a.stats + ((size_t)b * (a.C / a.g) + c / a.g) * 2;
        st[0] = mean;
        st[1] = var;
    }
}

// The sibling for a norm over groups of any width g (C a multiple of g): grid (C / g, b), one workgroup a
// (cloud, group).  Each channel's sums as above; the group's are those added over its channels ascending,
// 64 at a time through wave 0's lanes (as the g = 32 branch above adds its 32).  count: values per channel.
static __global__ __launch_bounds__(kFinThreads * kFinRuns) void norm_finalize_groups(FinArgs a) {
    __shared__ double2 runs[kFinRuns][kFinThreads];
    const int lane = threadIdx.x & 63, grp = blockIdx.x, b = blockIdx.y;
    const int run = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    double gs = 0.0, gss = 0.0;
    for (int c0 = 0; c0 < a.g; c0 += kFinThreads) {
        const bool in = c0 + lane < a.g;
        double s, ss;
        fin_channel_sums(a, b, grp * a.g + c0 + lane, in, lane, run, runs, s, ss);
        if (run == 0) {
            const int live = min(kFinThreads, a.g - c0);
            for (int j = 0; j < live; ++j) {
                gs += __shfl(s, j, 64);
                gss += __shfl(ss, j, 64);
            }
        }
        __syncthreads();  // runs[] is free for the next 64 channels
    }
    if (run != 0) return;
    const double cnt = a.count * a.g, mean = gs / cnt;
    double var = gss / cnt - mean * mean;
    if (!(var > 0.0)) var = 0.0;
    for (int c = lane; c < a.g; c += kFinThreads) fin_coef(a, b, grp * a.g + c, mean, var);
    if (a.stats && lane == 0) {
        double *st = a.stats + ((size_t)b * gridDim.x + grp) * 2;
        st[0] = mean;
        st[1] = var;
    }
}

}  // namespace pcr
