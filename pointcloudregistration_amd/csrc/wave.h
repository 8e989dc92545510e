// Device / launch helpers that units used to carry copies of: wave64 butterfly
// reductions, the block-wide bounding-box reduction, the 32x32 MFMA accumulator's
// row map, a few one-line functions.
// Header only; HIP units only (it calls __shfl_xor).  A kernel whose device
// code is pinned keeps its written-out butterfly: the same loop behind an
// inlined call schedules differently.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pcr {

typedef unsigned long long u64;

// The 32x32 f32 MFMA accumulator: 16 registers per lane.  Lane l holds column
// l & 31; register r of lane half hh = l >> 5 holds the row tile_row(r, hh).
typedef float f32x16 __attribute__((ext_vector_type(16)));
__device__ __forceinline__ int tile_row(int r, int hh) { return (r & 3) + 8 * (r >> 2) + 4 * hh; }

// Wave reduce: the xor butterfly, offsets 32 down to 1, result in every lane.
// One fixed order, so a floating-point sum has the same bits wherever it is
// taken.  All 64 lanes must call it.
template <typename T, typename Op>
__device__ __forceinline__ T wave_reduce(T v, Op op) {
#pragma unroll
    for (int o = 32; o; o >>= 1) v = op(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ float vmin(float a, float b) { return fminf(a, b); }
__device__ __forceinline__ float vmax(float a, float b) { return fmaxf(a, b); }
__device__ __forceinline__ double vmin(double a, double b) { return fmin(a, b); }
__device__ __forceinline__ double vmax(double a, double b) { return fmax(a, b); }
template <typename T>
__device__ __forceinline__ T wave_sum(T v) { return wave_reduce(v, [](T a, T b) { return a + b; }); }
template <typename T>
__device__ __forceinline__ T wave_min(T v) { return wave_reduce(v, [](T a, T b) { return vmin(a, b); }); }
template <typename T>
__device__ __forceinline__ T wave_max(T v) { return wave_reduce(v, [](T a, T b) { return vmax(a, b); }); }
__device__ __forceinline__ int wave_or(int v) { return wave_reduce(v, [](int a, int b) { return a | b; }); }

// Block-wide bounding box over a block of WAVES waves.  Every thread passes its
// lo[3] / hi[3] / bad; thread 0 comes back with the block's box in lo / hi and
// the or of every bad as the result (other threads: wave partials).  Ends
// after one __syncthreads(); what a caller makes of the box -- a cell rule, an
// origin corner, the raw bounds -- is its own epilogue.
template <typename T, int WAVES>
__device__ __forceinline__ int block_bbox(T (&lo)[3], T (&hi)[3], int bad) {
    __shared__ T sl[3][WAVES], sh[3][WAVES];
    __shared__ int sb[WAVES];
    const int t = threadIdx.x;
    for (int c = 0; c < 3; ++c) { lo[c] = wave_min(lo[c]); hi[c] = wave_max(hi[c]); }
    bad = wave_or(bad);
    if ((t & 63) == 0) {
        for (int c = 0; c < 3; ++c) { sl[c][t >> 6] = lo[c]; sh[c][t >> 6] = hi[c]; }
        sb[t >> 6] = bad;
    }
    __syncthreads();
    if (t != 0) return bad;
    for (int w = 1; w < WAVES; ++w) {
        for (int c = 0; c < 3; ++c) { lo[c] = vmin(lo[c], sl[c][w]); hi[c] = vmax(hi[c], sh[c][w]); }
        bad |= sb[w];
    }
    return bad;
}

// points of pair p: the per-pair count clamped to [0, Nmax]; Nmax without counts
__device__ __forceinline__ int count_of(const int32_t *n, int p, int Nmax) {
    return n ? min(max(n[p], 0), Nmax) : Nmax;
}
// the segment (cloud, batch element) of flat index i: largest b with off[b] <= i
__device__ __forceinline__ int segment_of(const int *off, int nb, int i) {
    int lo = 0, hi = nb - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (off[mid] <= i) lo = mid; else hi = mid - 1;
    }
    return lo;
}
// f32 squared distance, associated (dx^2 + dy^2) + dz^2
__device__ __forceinline__ float d2_direct(float ax, float ay, float az, float bx, float by, float bz) {
    const float dx = ax - bx, dy = ay - by, dz = az - bz;
    return (dx * dx + dy * dy) + dz * dz;
}
inline int cdiv(long long a, long long b) { return (int)((a + b - 1) / b); }
inline long long cdiv64(long long a, long long b) { return (a + b - 1) / b; }
inline unsigned nbits(u64 x) { return x ? 64u - (unsigned)__builtin_clzll(x) : 0u; }

}  // namespace pcr
