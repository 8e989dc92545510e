// The f16 split screen's operands (featnn_v5.h has the layout): the pair's
// scale from a sample, the packed images of both clouds with their norms, split
// errors and per-pair maxima, the repair of the pairs the sample misjudged, and
// featnn_row9's column terms.  One host entry point: v5_prepare.
#include "featnn_v5.h"
#include <algorithm>

namespace pcr {
namespace {

// Round 5: the pair's scale without a separate pass over the descriptors.
// The split needs every |x s| below 2^T (f16 range of hi / lo and of the norm
// parts); round 4 read both clouds once for their max (feat_maxabs, 537 MB per
// 256-pair step) before the packs read them again.  Now:
//   feat_sample  -- per pair, the max |x| of the first kSampleRows rows of each cloud;
//   the packs    -- scale s = 2^(T - kSpecMargin - 1 - e) for the sample max in
//                   [2^e, 2^(e+1)), i.e. kSpecMargin binades of headroom; a row
//                   with an element at or above 2^T after scaling (or not
//                   finite) flags its pair;
//   repair       -- feat_maxabs and the packs again, for the flagged pairs only
//                   (the round-4 path: s from the full max), launched every
//                   call on a small grid that walks the flags (empty in the
//                   common case).
// The screens' bounds are in the units of the scale actually used (the packs
// store it per pair), so a smaller-than-optimal scale only loosens the
// certification by its absolute (f16 subnormal, norm-split) terms: one binade
// of headroom (any element up to 2-4x the sample's max stays in range) cost
// ~2 % of the bound at the bench's magnitudes; three binades cost 25 % (27 %
// more rows rescanned, measured).
constexpr int kSpecMargin = 1;
constexpr int kSampleRows = 64;  // rows of each cloud in the sample
constexpr int kRepairR = 8;  // repair launches' grid.y (flagged pairs by rank mod R)

// the flagged pairs of rank y, y + R, ... (every wave walks the same flags, so
// control flow stays uniform across the block)
template <class Fn>
__device__ __forceinline__ void for_flagged(const int *bad, int P, int y, int R, Fn fn) {
    const int l = threadIdx.x & 63;
    int rank = 0;
    for (int b = 0; b < P; b += 64) {
        unsigned long long f = __ballot(b + l < P && bad[b + l] != 0);
        while (f) {
            const int q = b + __builtin_ctzll(f);
            f &= f - 1;
            if (rank % R == y) fn(q);
            ++rank;
        }
    }
}

// sample max bits per pair; clears the pair's counters that the stage's later
// launches accumulate into (norm maxima, rescan list counts) and its flag
__global__ __launch_bounds__(256) void feat_sample(const float *F, const int32_t *nf, int Nmax,
                                                   const float *G, const int32_t *ng, int Mmax, int D,
                                                   unsigned *smax, unsigned *clr, int *bad, int P) {
    const int p = blockIdx.x, t = threadIdx.x;
    float m = 0.0f;
    for (int which = 0; which < 2; ++which) {
        const float *x = (which ? G + (size_t)p * Mmax * D : F + (size_t)p * Nmax * D);
        const int rows = min(which ? count_of(ng, p, Mmax) : count_of(nf, p, Nmax), kSampleRows);
        for (int i = t; i < rows * D; i += 256) m = fmaxf(m, fabsf(x[i]));
    }
#pragma unroll
    for (int o = 32; o; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    __shared__ float wm[4];
    if ((t & 63) == 0) wm[t >> 6] = m;
    __syncthreads();
    if (t == 0) {
        smax[p] = __float_as_uint(fmaxf(fmaxf(wm[0], wm[1]), fmaxf(wm[2], wm[3])));  // >= 0, never NaN
        clr[p] = 0u;          // gmax
        clr[P + p] = 0u;      // fmax
        clr[3 * P + p] = 0u;  // cnt12
        clr[4 * P + p] = 0u;  // cnt21
        clr[5 * P + p] = 0u;  // gemax
        clr[6 * P + p] = 0u;  // femax
        clr[7 * P + p] = 0u;  // fbc12
        clr[8 * P + p] = 0u;  // fbc21
        bad[p] = 0;
    }
}

// repair: max |element| of each FLAGGED pair's clouds, gridDim.z 1024-thread
// blocks per (pair, cloud), each a contiguous slice of float4 loads; partial
// maxima, one plain store per block (mxp[(p * 2 + which) * Z + z]); block
// (., 0, 0) also clears the pair's norm maxima for the repair packs
__global__ __launch_bounds__(1024) void feat_maxabs(const float *F, const int32_t *nf, int Nmax,
                                                    const float *G, const int32_t *ng, int Mmax,
                                                    int D, unsigned *mxp, unsigned *clr, const int *bad, int P) {
    const int which = blockIdx.y, t = threadIdx.x, z = blockIdx.z, Z = gridDim.z;
    for_flagged(bad, P, blockIdx.x, gridDim.x, [&](int p) {
        const float *X = which ? G : F;
        const int cnt = which ? count_of(ng, p, Mmax) : count_of(nf, p, Nmax);
        const size_t tot = (size_t)cnt * D;
        const float *x = X + (size_t)p * (which ? Mmax : Nmax) * D;
        float m = 0.0f;
        if (((uintptr_t)x & 15) == 0) {
            const float4 *x4 = reinterpret_cast<const float4 *>(x);
            const size_t t4 = tot >> 2;
            const size_t per = (t4 + Z - 1) / Z, lo = min(t4, per * z), hi = min(t4, lo + per);
            for (size_t i = lo + t; i < hi; i += 1024) {
                const float4 v = x4[i];
                m = fmaxf(m, fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))));
            }
            if (z == Z - 1)
                for (size_t i = (t4 << 2) + t; i < tot; i += 1024) m = fmaxf(m, fabsf(x[i]));
        } else {
            for (size_t i = (size_t)z * 1024 + t; i < tot; i += (size_t)Z * 1024) m = fmaxf(m, fabsf(x[i]));
        }
#pragma unroll
        for (int o = 32; o; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
        __shared__ float wm[16];
        if ((t & 63) == 0) wm[t >> 6] = m;
        __syncthreads();
        if (t == 0) {
            float r = wm[0];
            for (int w = 1; w < 16; ++w) r = fmaxf(r, wm[w]);
            mxp[((size_t)p * 2 + which) * Z + z] = __float_as_uint(r);  // r >= 0, never NaN
            if (which == 0 && z == 0) {  // gmax, fmax, gemax, femax: the repair packs max into them again
                clr[p] = 0u;
                clr[P + p] = 0u;
                clr[5 * P + p] = 0u;
                clr[6 * P + p] = 0u;
            }
        }
        __syncthreads();
    });
}

// the pair's max |element| from feat_maxabs' 2 Z partials (bits of non-negative
// floats: unsigned order = float order), reduced by every wave on its own
__device__ __forceinline__ unsigned pair_max_bits(const unsigned *mxp, int Z, int p) {
    const int l = threadIdx.x & 63;
    unsigned m = 0u;
    for (int k = l; k < 2 * Z; k += 64) m = max(m, mxp[(size_t)p * 2 * Z + k]);
#pragma unroll
    for (int o = 32; o; o >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, o, 64));
    return m;
}

// one atomic per workgroup: max of the four waves' values (bit patterns of
// non-negative floats; unsigned order = float order)
__device__ __forceinline__ void block_max_atomic(unsigned v, unsigned *wm, unsigned *dst) {
#pragma unroll
    for (int o = 32; o; o >>= 1) v = max(v, (unsigned)__shfl_xor((int)v, o, 64));
    if ((threadIdx.x & 63) == 0) wm[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned m = max(max(wm[0], wm[1]), max(wm[2], wm[3]));
        if (m != 0u) atomicMax(dst, m);
    }
}

template <class Body>
__device__ __forceinline__ void pack_pairs(const PackCtl &c, int T, Body body) {
    if (!c.repair) {
        const int p = blockIdx.y;
        const float s = pair_scale5(c.smax[p], T - kSpecMargin);
        if (blockIdx.x == 0 && threadIdx.x == 0) c.sc[p] = __float_as_uint(s);
        body(p, s, true);
    } else {
        for_flagged(c.bad, c.P, blockIdx.y, gridDim.y, [&](int p) {
            const float s = pair_scale5(pair_max_bits(c.mxp, c.Z, p), T);
            if (blockIdx.x == 0 && threadIdx.x == 0) c.sc[p] = __float_as_uint(s);
            body(p, s, false);
            __syncthreads();  // the block's LDS is reused by the next pair
        });
    }
}

// role 0: rows (A), role 1: columns (B).  256-thread blocks, one wave per
// 32-row tile; each tile is staged through LDS with coalesced loads (scaled,
// exact) and every lane emits its stored 16-byte operand fragments: NS = 2S + 1
// chunks per tile, or NS = S (compact: the hi segment alone, the same bits; the
// lo halves, the norm parts and c are then not computed).
__global__ __launch_bounds__(256) void feat_pack5(PackIO io, int D, int S, int NS, Split5 sp, PackCtl pc) {
    const int role = blockIdx.z;
    const float *X = io.X[role];
    const int32_t *n = io.n[role];
    const int Nmax = io.Nmax[role], ntiles = io.ntiles[role];
    f16x8 *Xp = io.Xp[role];
    float *nrm = io.nrm[role];
    unsigned *nmax = io.nmax[role];
    if ((int)blockIdx.x * 4 >= ntiles) return;  // whole block: the other cloud has more tiles
    __shared__ float xs[4][32][65];  // D <= 64 (+1 pad: conflict-free row reads)
    __shared__ unsigned wmax[4];
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    const int t = blockIdx.x * 4 + w;  // ntiles is a multiple of 8 (host pads)
    const float lim = __builtin_ldexpf(1.0f, sp.T);
    pack_pairs(pc, sp.T, [&](int p, float s, bool check) {
        const int cnt = count_of(n, p, Nmax);
        const int nrows = min(max(cnt - t * 32, 0), 32);
        const float *base = X + ((size_t)p * Nmax + (size_t)t * 32) * D;
        float (*x)[65] = xs[w];
        // e / D by a 64-bit reciprocal (exact for e < 2^16; 2^32/D + 1 needs 33 bits at D = 1)
        const unsigned long long invD = 0xFFFFFFFFull / (unsigned long long)D + 1ull;
        bool ok = true;
        for (int e = l; e < 32 * D; e += 64) {
            const int r = (int)(((unsigned long long)e * invD) >> 32), k = e - r * D;
            const float v = r < nrows ? base[e] * s : 0.0f;
            ok = ok && __builtin_fabsf(v) < lim;  // NaN / inf: not ok
            x[r][k] = v;
        }
        if (check && !ok) pc.bad[p] = 1;
        __syncthreads();
        const int rr = l & 31, h = l >> 5;
        const bool valid = rr < nrows;
        double acc = 0.0, ea = 0.0;
        for (int k = 0; k < D; ++k) {
            const double v = (double)x[rr][k];
            acc = acc + v * v;
            const double e = (double)(x[rr][k] - (float)(_Float16)x[rr][k]);  // exact in f32
            ea = ea + e * e;
        }
        // norm parts of acc / c (exact power-of-two division)
        _Float16 np[3] = {(_Float16)0.0f, (_Float16)0.0f, (_Float16)0.0f};
        if (NS == S) {
            // compact: no norm chunk
        } else if (valid) {
            double wv = acc * __builtin_ldexp(1.0, -sp.cs);
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                np[q] = (_Float16)(float)wv;  // |wv| < 2^15: double->float->half may round twice;
                wv = wv - (double)np[q];      // the bound charges 2^-11 per part regardless
            }
        } else {
            // finite sentinel 3 * 65504 * c > any real distance (<= 4 D 2^2T):
            // index bits are OR-ed into screen values, which must not be inf
            np[0] = (_Float16)65504.0f;
            np[1] = (_Float16)65504.0f;
            np[2] = (_Float16)65504.0f;
        }
        const _Float16 cval = (_Float16)__builtin_ldexpf(1.0f, sp.cs);
        f16x8 *dst = Xp + ((size_t)p * ntiles + t) * NS * 64 + l;
        for (int c = 0; c < NS; ++c) {
            f16x8 o;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int seg = c < S ? 0 : (c < 2 * S ? 1 : 2);   // hi | lo | norms
                const int k = 16 * (c - seg * S) + 8 * h + j;      // index inside the segment
                _Float16 v = (_Float16)0.0f;
                if (seg < 2) {
                    if (k < D) {
                        const float xv = x[rr][k];
                        const _Float16 hi = (_Float16)xv;
                        const _Float16 lo = (_Float16)(xv - (float)hi);
                        const _Float16 part = seg == 0 ? hi : lo;
                        v = role == 0 ? (_Float16)(-2.0f * (float)part) : part;
                    }
                } else {
                    if (k < 3) v = role == 0 ? np[k] : cval;
                    else if (k < 6) v = role == 0 ? cval : np[k - 3];
                    else if (k == 6 && role == 1) v = (_Float16)32768.0f;  // featnn_row8's biases
                    else if (k == 7 && role == 0) v = (_Float16)32768.0f;
                }
                o[j] = v;
            }
            dst[(size_t)c * 64] = o;
        }
        // the pair's max norm: one atomic per WORKGROUP.  The P words share a few
        // cache lines, and one atomic per wave (256 per cloud) serialised at the
        // L2: ~80 us per launch whatever the batch.  Max of the bit patterns: the
        // same word per-lane atomics would leave, NaN included.
        const float r = (h == 0 && valid) ? (float)__builtin_sqrt(acc) : 0.0f;
        if (h == 0) {
            nrm[(size_t)p * ntiles * 32 + t * 32 + rr] = r;
            io.rex[role][(size_t)p * ntiles * 32 + t * 32 + rr] = valid ? split_err_norm(ea) : 0.0f;
            io.ct[role][(size_t)p * ntiles * 32 + t * 32 + rr] = valid ? (float)acc : -1.0f;
        }
        block_max_atomic(__float_as_uint(r), wmax, nmax + p);
        __syncthreads();
        block_max_atomic(valid ? __float_as_uint(split_err_norm(ea)) : 0u, wmax, io.emax[role] + p);
    });
}

// Register-resident pack for a compile-time D (the hot D = 32): one lane per
// (row, half), the row loaded with 16-byte loads (both halves of the wave share
// the cache lines), the split computed once per element, and each 16-byte
// operand fragment selected between the two compile-time candidates of the
// lane's half -- no LDS, no per-half segment arithmetic.  Same values as
// feat_pack5 (same operations, same order).
template <int D>
__global__ __launch_bounds__(256) void feat_pack5r(PackIO io, Split5 sp, PackCtl pc) {
    const int role = blockIdx.z;
    const float *X = io.X[role];
    const int32_t *n = io.n[role];
    const int Nmax = io.Nmax[role], ntiles = io.ntiles[role];
    f16x8 *Xp = io.Xp[role];
    float *nrm = io.nrm[role];
    unsigned *nmax = io.nmax[role];
    if ((int)blockIdx.x * 4 >= ntiles) return;  // whole block: the other cloud has more tiles
    constexpr int S = (D + 15) / 16;  // chunks per segment
    constexpr int NM = 2 * S + 1;     // stored chunks
    constexpr int G = 2 * S;          // 8-half fragments per segment
    __shared__ unsigned wmax[4];
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    const int t = blockIdx.x * 4 + w;  // ntiles is a multiple of 8 (host pads)
    const float lim = __builtin_ldexpf(1.0f, sp.T);
    pack_pairs(pc, sp.T, [&](int p, float s, bool check) {
        const int cnt = count_of(n, p, Nmax);
        const int nrows = min(max(cnt - t * 32, 0), 32);
        const int rr = l & 31, h = l >> 5;
        const bool valid = rr < nrows;
        float x[D];
        if (valid) {
            const float4 *row = reinterpret_cast<const float4 *>(X + ((size_t)p * Nmax + (size_t)t * 32 + rr) * D);
#pragma unroll
            for (int q = 0; q < D / 4; ++q) {
                const float4 v = row[q];
                x[4 * q] = v.x * s; x[4 * q + 1] = v.y * s; x[4 * q + 2] = v.z * s; x[4 * q + 3] = v.w * s;
            }
        } else {
#pragma unroll
            for (int k = 0; k < D; ++k) x[k] = 0.0f;
        }
        if (check) {
            bool ok = true;
#pragma unroll
            for (int k = 0; k < D; ++k) ok = ok && __builtin_fabsf(x[k]) < lim;  // NaN / inf: not ok
            if (!ok) pc.bad[p] = 1;
        }
        double acc = 0.0, ea = 0.0;
#pragma unroll
        for (int k = 0; k < D; ++k) {
            const double v = (double)x[k];
            acc = acc + v * v;
            const double e = (double)(x[k] - (float)(_Float16)x[k]);  // exact in f32
            ea = ea + e * e;
        }
        _Float16 np[3];
        if (valid) {
            double wv = acc * __builtin_ldexp(1.0, -sp.cs);
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                np[q] = (_Float16)(float)wv;
                wv = wv - (double)np[q];
            }
        } else {
            np[0] = (_Float16)65504.0f;
            np[1] = (_Float16)65504.0f;
            np[2] = (_Float16)65504.0f;
        }
        const _Float16 cval = (_Float16)__builtin_ldexpf(1.0f, sp.cs);
        _Float16 s0[D], s1[D];  // the two stored segments of this role: hi | lo
#pragma unroll
        for (int k = 0; k < D; ++k) {
            const _Float16 hi = (_Float16)x[k];
            const _Float16 lo = (_Float16)(x[k] - (float)hi);
            if (role == 0) {
                s0[k] = (_Float16)(-2.0f * (float)hi);
                s1[k] = (_Float16)(-2.0f * (float)lo);
            } else {
                s0[k] = hi;
                s1[k] = lo;
            }
        }
        auto frag = [&](int g) {  // compile-time g after unrolling
            f16x8 o;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                _Float16 v = (_Float16)0.0f;
                const int k0 = 8 * (g % G) + j;
                if (g < G) v = k0 < D ? s0[k0 < D ? k0 : 0] : (_Float16)0.0f;
                else if (g < 2 * G) v = k0 < D ? s1[k0 < D ? k0 : 0] : (_Float16)0.0f;
                else if (g == 2 * G) {
                    if (j < 3) v = role == 0 ? np[j] : cval;
                    else if (j < 6) v = role == 0 ? cval : np[j - 3];
                    else if (j == 6 && role == 1) v = (_Float16)32768.0f;  // featnn_row8's biases
                    else if (j == 7 && role == 0) v = (_Float16)32768.0f;
                }
                o[j] = v;
            }
            return o;
        };
        f16x8 *dst = Xp + ((size_t)p * ntiles + t) * NM * 64 + l;
#pragma unroll
        for (int c = 0; c < NM; ++c) {
            const f16x8 a = frag(2 * c), b = frag(2 * c + 1);
            dst[(size_t)c * 64] = h ? b : a;
        }
        // the pair's max norm: one atomic per WORKGROUP (see feat_pack5)
        const float r = (h == 0 && valid) ? (float)__builtin_sqrt(acc) : 0.0f;
        if (h == 0) {
            nrm[(size_t)p * ntiles * 32 + t * 32 + rr] = r;
            io.rex[role][(size_t)p * ntiles * 32 + t * 32 + rr] = valid ? split_err_norm(ea) : 0.0f;
            io.ct[role][(size_t)p * ntiles * 32 + t * 32 + rr] = valid ? (float)acc : -1.0f;
        }
        block_max_atomic(__float_as_uint(r), wmax, nmax + p);
        __syncthreads();
        block_max_atomic(valid ? __float_as_uint(split_err_norm(ea)) : 0u, wmax, io.emax[role] + p);
    });
}

// The compact image's register-resident pack (round 11): the hi segment alone,
// S chunks per tile.  Without the lo and norm chunks a lane half has nothing of
// its own left to compute, and feat_pack5r's second half would only repeat the
// first one's row (the loads, the f64 sums, the conversions: the kernel is
// VALU-issue bound once its dead stores are gone).  So here a lane is ONE row
// and a wave two tiles (lane l: tile 2 w + l / 32, row l % 32): the row is
// loaded, scaled, checked and summed once, and the lane stores all 2 S
// fragments of its row -- per store the wave's halves write 512 contiguous
// bytes of their two tiles.  Same values as feat_pack5r's: the same operations
// in the same order per row (x s, the f64 sums over k ascending, f16(x s), -2 x
// for the row role), the same per-row arrays and per-pair maxima.
template <int D>
__global__ __launch_bounds__(256) void feat_pack5c(PackIO io, Split5 sp, PackCtl pc) {
    static_assert(D % 16 == 0, "whole chunks (no zero tail), float4 rows");
    const int role = blockIdx.z;
    const float *X = io.X[role];
    const int32_t *n = io.n[role];
    const int Nmax = io.Nmax[role], ntiles = io.ntiles[role];
    f16x8 *Xp = io.Xp[role];
    float *nrm = io.nrm[role];
    unsigned *nmax = io.nmax[role];
    if ((int)blockIdx.x * 8 >= ntiles) return;  // whole block: the other cloud has more tiles
    constexpr int S = D / 16;  // stored chunks
    __shared__ unsigned wmax[4];
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    const int t = blockIdx.x * 8 + 2 * w + (l >> 5);  // ntiles is a multiple of 8 (host pads)
    const int rr = l & 31;
    const float lim = __builtin_ldexpf(1.0f, sp.T);
    pack_pairs(pc, sp.T, [&](int p, float s, bool check) {
        const int cnt = count_of(n, p, Nmax);
        const bool valid = t * 32 + rr < cnt;
        float x[D];
        if (valid) {
            const float4 *row = reinterpret_cast<const float4 *>(X + ((size_t)p * Nmax + (size_t)t * 32 + rr) * D);
#pragma unroll
            for (int q = 0; q < D / 4; ++q) {
                const float4 v = row[q];
                x[4 * q] = v.x * s; x[4 * q + 1] = v.y * s; x[4 * q + 2] = v.z * s; x[4 * q + 3] = v.w * s;
            }
        } else {
#pragma unroll
            for (int k = 0; k < D; ++k) x[k] = 0.0f;
        }
        if (check) {
            bool ok = true;
#pragma unroll
            for (int k = 0; k < D; ++k) ok = ok && __builtin_fabsf(x[k]) < lim;  // NaN / inf: not ok
            if (!ok) pc.bad[p] = 1;
        }
        double acc = 0.0, ea = 0.0;
#pragma unroll
        for (int k = 0; k < D; ++k) {
            const double v = (double)x[k];
            acc = acc + v * v;
            const double e = (double)(x[k] - (float)(_Float16)x[k]);  // exact in f32
            ea = ea + e * e;
        }
        f16x8 *dst = Xp + ((size_t)p * ntiles + t) * S * 64 + rr;
#pragma unroll
        for (int g = 0; g < 2 * S; ++g) {  // fragment g: chunk g / 2, lane half g % 2
            f16x8 o;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const _Float16 hi = (_Float16)x[8 * g + j];
                o[j] = role == 0 ? (_Float16)(-2.0f * (float)hi) : hi;
            }
            dst[(size_t)(g >> 1) * 64 + 32 * (g & 1)] = o;
        }
        // the pair's maxima: one atomic per WORKGROUP (see feat_pack5)
        const float r = valid ? (float)__builtin_sqrt(acc) : 0.0f;
        const size_t ro = (size_t)p * ntiles * 32 + t * 32 + rr;
        nrm[ro] = r;
        io.rex[role][ro] = valid ? split_err_norm(ea) : 0.0f;
        io.ct[role][ro] = valid ? (float)acc : -1.0f;
        block_max_atomic(__float_as_uint(r), wmax, nmax + p);
        __syncthreads();
        block_max_atomic(valid ? __float_as_uint(split_err_norm(ea)) : 0u, wmax, io.emax[role] + p);
    });
}

// featnn_row9's column terms (after the packs and their repairs): the packs
// stored f32(|x s|^2) per row, -1 on padding rows; here ct = f32(that + B), B the
// pair's bias.  The sweep, the regroup and the finish order the screened values
//   v = fl(ct_j - 2 f16(x).f16(y_j))
// by their bit patterns as unsigned integers, which is the float order only for
// v >= 0, so B is sized against the screen's worst excursion, not against
// max |x|^2.  With M the larger of the two clouds' max norms (fmax, gmax), E the
// larger of their max split errors |x - f16(x)| (femax, gemax) and u = 2^-24:
//   2 f16(x).f16(y) <= |f16(x)|^2 + |f16(y)|^2          (|f16(x) - f16(y)|^2 >= 0)
//   |f16(x)|^2 <= (|x| + E)^2 <= M^2 + 2 M E + E^2
//   |f16(y)|^2 <= |y|^2 + 2 M E + E^2
//   ct_j >= |y_j|^2 + B - u (2 M^2 + B)(1 + 2^-20)       (f32 |y|^2, then + B)
//   the MFMA chain (C = ct_j, 16 S <= 32 products): 2 (16 S + 2) u (|C| +
//   sum |products|) <= 68 u (B + M^2 + 2 (M + E)^2)
// so v >= B - Q - u (2 M^2 + B)(1 + 2^-20) - 68 u (B + 3 Q), Q = M^2 + 4 M E +
// 2 E^2, which is > B (1 - 1.7e-5) - Q for Q < B: v > 0 whenever
//   B >= Q (1 + 2^-15)                                    ((1 + 2^-15)(1 - 1.7e-5) > 1)
// (f16 operands the MFMA flushes only shrink |f16(.)|; the f32 roundings of M and
// E, 2^-23 relative, are inside the margin's rest, 1.4e-5).  B is the smallest power
// of two above Q (1 + 2^-15) + 1.  Then also |y|^2 <= M^2 < B: ct lies in [B, 2B]
// and 2B - ct is exact; and v <= 2B + 2 (M + E)^2 < 4B: the padding rows' 16 B is
// above every real value.  row_tail / one_term_fails read B from cbias, so their
// u B terms follow it.
// Non-finite: the packs max the norms' bit patterns, so a cloud with a NaN row
// has the NaN pattern as its max and fmaxf against the other cloud's would drop
// it.  Each cloud's max is tested on its own: if either is not finite (or past
// the split's range) the pair takes B = 2^60, under which its rows certify
// nothing (u B is above every gap) and every finite value is ~2^60 > 0.
__global__ __launch_bounds__(256) void feat_colterms(float *fct, float *gct, int ntn, int ntm,
                                                     const unsigned *fmax, const unsigned *gmax,
                                                     const unsigned *femax, const unsigned *gemax, float *cbias) {
    const int p = blockIdx.y, role = blockIdx.z;
    const float mx = __uint_as_float(fmax[p]), my = __uint_as_float(gmax[p]);
    const float ex = __uint_as_float(femax[p]), ey = __uint_as_float(gemax[p]);
    double B = 0x1p60;
    // (each comparison is false for a NaN)
    if (mx < 0x1p50f && my < 0x1p50f && ex < 0x1p50f && ey < 0x1p50f) {
        const double M = (double)__builtin_fmaxf(mx, my), E = (double)__builtin_fmaxf(ex, ey);
        const double m2 = (M * M + 4.0 * M * E + 2.0 * E * E) * (1.0 + 0x1p-15) + 1.0;
        const int e = (int)((__double_as_longlong(m2) >> 52) & 0x7ff) - 1023;  // m2 in [2^e, 2^(e+1))
        B = __builtin_ldexp(1.0, e + 1);
    }
    if (blockIdx.x == 0 && role == 0 && threadIdx.x == 0) cbias[p] = (float)B;
    const int nt = role ? ntm : ntn;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nt * 32) return;
    float *ct = (role ? gct : fct) + (size_t)p * nt * 32 + i;
    const float x = *ct;
    *ct = x < 0.0f ? (float)(16.0 * B) : (float)((double)x + B);
}

// chunks per tile of the last prepare's images (diagnostic, pcr_featnn_image_chunks)
int g_image_chunks = 0;

}  // namespace

int v5_prepare(const float *F, const float *G, int P, int Nmax, int Mmax, int D, const int32_t *n_src,
               const int32_t *n_tgt, hipStream_t s, V5Buf &v, bool compact) {
    v.P = P;
    v.D = D;
    v.S = cdiv(D, 16);
    v.NM = 2 * v.S + 1;
    v.ich = compact ? v.S : v.NM;
    g_image_chunks = v.ich;
    v.NX = 3 * v.S + 1;
    v.sp = split5_params(D);
    v.W = 8;                                          // waves (32-row tiles) per workgroup
    v.nrb = cdiv(cdiv(Nmax, 32), v.W);                // dual screen row blocks
    const FeatTiles tiles = feat_tiles(Nmax, Mmax);
    const int ich = v.ich, ntn = tiles.ntn, ntm = tiles.ntm;
    V5Side &f = v.side[0], &g = v.side[1];
    f.X = F; f.n = n_src; f.Nmax = Nmax; f.nt = ntn;
    g.X = G; g.n = n_tgt; g.Nmax = Mmax; g.nt = ntm;
    v.ctbits = 1;
    while ((1 << v.ctbits) < std::max(ntm, ntn)) ++v.ctbits;
    PCR_REQUIRE(v.ctbits <= 16, PCR_ERR_ARG, "feature_match: N=%d / M=%d too large", Nmax, Mmax);
    const size_t ap = (size_t)P * ntn * ich * 64, bp = (size_t)P * ntm * ich * 64;  // f16x8
    const size_t nn_n = (size_t)P * ntn * 32, nn_m = (size_t)P * ntm * 32;
    const size_t pn = (size_t)P * Nmax, pm = (size_t)P * Mmax;
    unsigned *mxp, *smax;
    int *bad;
    WsLayout l;
    l.take(f.Xp, ap); l.take(g.Xp, bp);
    l.take(f.nr, nn_n); l.take(g.nr, nn_m);
    l.take(f.re, nn_n); l.take(g.re, nn_m);
    l.take(f.ct, nn_n); l.take(g.ct, nn_m);
    // nine [P] arrays, contiguous from G's max norm: max|y|, max|x|, the scale used, cnt12,
    // cnt21, G's and F's max split error, fbc12, fbc21 (feat_sample clears all but the scale)
    l.take(g.nmax, P); l.take(f.nmax, P); l.take(v.mx, P);
    l.take(v.cnt12, P); l.take(v.cnt21, P);
    l.take(g.emax, P); l.take(f.emax, P);
    l.take(v.fbc12, P); l.take(v.fbc21, P);
    l.take(v.list12, pn); l.take(v.list21, pm);  // per pair, stride Nmax / Mmax
    l.take(v.fbl12, pn); l.take(v.fbl21, pm);    // per pair, stride Nmax / Mmax
    l.take(mxp, 2 * (size_t)P * 8);  // [P][2][zr] partial maxima (repair)
    l.take(smax, P);                 // [P] sample maxima
    l.take(bad, P);                  // [P] repair flags
    l.take(v.cbias, P);              // [P] featnn_row9's B
    PCR_REQUIRE(workspace_bind(kWsFeatPack_NndRagged, l, kWsSlack), PCR_ERR_NOMEM, "feature_match: %s",
                pcr_last_error());
    prof_begin(s, kProfFeatPack);
    hipLaunchKernelGGL(feat_sample, dim3(P), dim3(256), 0, s, F, n_src, Nmax, G, n_tgt, Mmax, D, smax, g.nmax,
                       bad, P);
    PCR_LAUNCH_CHECK();
    const PackIO io{{f.X, g.X},   {f.n, g.n},       {f.Nmax, g.Nmax}, {f.nt, g.nt}, {f.Xp, g.Xp},
                    {f.nr, g.nr}, {f.nmax, g.nmax}, {f.emax, g.emax}, {f.re, g.re}, {f.ct, g.ct}};
    // the repair passes: few blocks walking the flags (empty in the common case)
    const int R = std::min(P, kRepairR), zr = 8;
    for (int rep = 0; rep < 2; ++rep) {
        PackCtl pc{smax, mxp, zr, P, rep, bad, v.mx};
        if (rep) {
            hipLaunchKernelGGL(feat_maxabs, dim3(R, 2, zr), dim3(1024), 0, s, F, n_src, Nmax, G, n_tgt, Mmax, D,
                               mxp, g.nmax, bad, P);
            PCR_LAUNCH_CHECK();
        }
        const int gy = rep ? R : P;
        const dim3 grid(cdiv(std::max(ntn, ntm), 4), gy, 2);
        // (the repair launch stores the layout of the first)
        static_assert(kRow8G % 8 == 0, "feat_pack5c: whole blocks of eight tiles");
        if (D == 32 && compact)  // a row per lane, eight tiles per block (ntn: a multiple of 16, ntm: of kRow8G)
            hipLaunchKernelGGL(feat_pack5c<32>, dim3(cdiv(std::max(ntn, ntm), 8), gy, 2), dim3(256), 0, s, io, v.sp, pc);
        else if (D == 32) hipLaunchKernelGGL(feat_pack5r<32>, grid, dim3(256), 0, s, io, v.sp, pc);  // register-resident
        else hipLaunchKernelGGL(feat_pack5, grid, dim3(256), 0, s, io, D, v.S, ich, v.sp, pc);
        PCR_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(feat_colterms, dim3(cdiv(std::max(ntn, ntm) * 32, 256), P, 2), dim3(256), 0, s, f.ct, g.ct,
                       ntn, ntm, f.nmax, g.nmax, f.emax, g.emax, v.cbias);
    PCR_LAUNCH_CHECK();
    prof_end(s, kProfFeatPack);
    return PCR_OK;
}

}  // namespace pcr

extern "C" int pcr_featnn_image_chunks(int32_t *chunks) {
    pcr::clear_error();
    PCR_REQUIRE(chunks, PCR_ERR_ARG, "featnn_image_chunks: null pointer");
    *chunks = pcr::g_image_chunks;
    return PCR_OK;
}
