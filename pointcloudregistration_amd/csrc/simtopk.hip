// Similarity top-k matching: the correspondence stage of ROPNet's TFMR
// (ROPNet/src/models/TFMR.py:226-257) without any (B,N1,M1) tensor.
//
// The reference forms the similarity with a bmm, takes the row maxima, sorts
// them, gathers the kept rows, runs a topk, writes a mask with index_put,
// normalises and multiplies the masked matrix with the target points.  Here:
//  * simtopk_sweep<K>: one 256-thread workgroup per (batch, 128 sources, 128
//    targets).  S = Y X^T on v_mfma_f32_32x32x2_f32 with the TARGETS on the
//    MFMA's row side and the SOURCES on the lane side, so a lane owns one
//    source row's 16 values of every 32x32 tile.  Both operands are staged
//    through LDS in chunks of 32 channels (rows padded to 36 floats, read as
//    float4: a lane takes the even or the odd channels of it, which is the
//    k order of the instruction); the next chunk's global loads fly while
//    the current one computes.  An accumulator carries its (target, source)
//    pair through every chunk, so each value is the contract's fmaf chain.
//    After the last chunk every lane pushes its values, target index
//    ascending, into a sorted list of K packed keys (monotone value bits <<
//    32 | ~index, as pcr_fps packs its maxima: one 64-bit compare orders by
//    value descending, then index ascending); the half-waves merge with one
//    shuffle per entry, the two waves that split the targets through LDS, and
//    the block's top-k of its 128 targets goes to the scratch.
//  * simtopk_merge: one thread per source row folds the target tiles' lists
//    into val / idx and leaves the row's selection key in the scratch.
//  * tfmr_select: one 1024-thread workgroup per batch.  A row's rank is the
//    number of keys above its own (the keys are distinct), counted against
//    the keys in LDS; a row ranked below n_keep writes sel, its idx, the
//    weights and tgt_corr at its rank.  No sort, no atomics.
// Numerics: include/pcr_api.h.  The MFMA adds one product per step to a
// single f32 accumulator, rounded once: bit for bit the fmaf chain in
// ascending channel order.  Channels past C are staged as +0 (fmaf(0, 0, s)
// = s for every s but -0, and -0 is reported as +0 anyway).
#include "pcr_internal.h"
#include "wave.h"

namespace {

using pcr::cdiv64, pcr::u64;
using pcr::f32x16;

constexpr int kSimThreads = 256;
constexpr int kSimTile = 128;              // sources and targets per workgroup
constexpr int kSimKC = 32;                 // channels per LDS chunk
constexpr int kSimLd = kSimKC + 4;         // LDS row stride in floats (16-byte rows, 9 slots)
constexpr int kSimLoads = kSimTile * kSimKC / 4 / kSimThreads;  // float4 per thread and operand: 4
constexpr int kMaxK = 8;
constexpr int kSelThreads = 1024;
constexpr int kSelChunk = 4096;            // keys per LDS stage (32 KiB)

// monotone bits of v: unsigned order = float order; -0 counts as +0
__device__ __forceinline__ unsigned mono_bits(float v) {
    unsigned u = __float_as_uint(v);
    u = u == 0x80000000u ? 0u : u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float mono_value(unsigned m) {
    return __uint_as_float((m & 0x80000000u) ? (m & 0x7fffffffu) : ~m);
}
// above 0 for every j >= 0: the low word ~j has its top bit set
__device__ __forceinline__ u64 sim_key(float v, int j) {
    return ((u64)mono_bits(v) << 32) | (unsigned)~j;
}

// L is sorted descending; keep the K largest of L and key
template <int K>
__device__ __forceinline__ void list_push(u64 (&L)[K], u64 key) {
    if (key > L[K - 1]) {
        L[K - 1] = key;
#pragma unroll
        for (int t = K - 1; t > 0; --t) {
            const u64 lo = L[t], hi = L[t - 1];
            const bool sw = lo > hi;
            L[t] = sw ? hi : lo;
            L[t - 1] = sw ? lo : hi;
        }
    }
}

struct SimArgs {
    const float *fx;  // (b,n1,c)
    const float *fy;  // (b,m1,c)
    u64 *part;        // (b,n1,ntt,k)
    int n1, m1, c, k, nst, ntt;
    int vec;          // c % 4 == 0 and both bases 16-byte aligned: float4 loads
};

__device__ __forceinline__ float4 sim_load4(const float *row, int c0, int c, bool vec) {
    if (vec) return c0 < c ? *reinterpret_cast<const float4 *>(row + c0) : make_float4(0.f, 0.f, 0.f, 0.f);
    float4 v;
    v.x = c0 + 0 < c ? row[c0 + 0] : 0.f;
    v.y = c0 + 1 < c ? row[c0 + 1] : 0.f;
    v.z = c0 + 2 < c ? row[c0 + 2] : 0.f;
    v.w = c0 + 3 < c ? row[c0 + 3] : 0.f;
    return v;
}

template <int K>
__global__ __launch_bounds__(kSimThreads) void simtopk_sweep(SimArgs a) {
    __shared__ __attribute__((aligned(16))) float smem[2 * kSimTile * kSimLd];
    float *Xs = smem;                      // [128 sources][36]
    float *Ys = smem + kSimTile * kSimLd;  // [128 targets][36]
    const int tid = threadIdx.x, l = tid & 63, wid = tid >> 6, h = l >> 5, lr = l & 31;
    const int wr = wid >> 1, wc = wid & 1;  // the wave's 64 targets / 64 sources
    const int tt = blockIdx.x % a.ntt;
    const int st = (blockIdx.x / a.ntt) % a.nst;
    const int bat = blockIdx.x / (a.ntt * a.nst);
    const int s0 = st * kSimTile, t0 = tt * kSimTile;
    const int c = a.c;
    const bool vec = a.vec != 0;

    // staging: element e = tid + 256 u of a chunk is row e >> 3, channels 4 (e & 7) ...
    const float *xrow[kSimLoads], *yrow[kSimLoads];
#pragma unroll
    for (int u = 0; u < kSimLoads; ++u) {
        const int row = (tid + kSimThreads * u) >> 3;
        xrow[u] = a.fx + ((size_t)bat * a.n1 + min(s0 + row, a.n1 - 1)) * c;  // rows past the end: the last one,
        yrow[u] = a.fy + ((size_t)bat * a.m1 + min(t0 + row, a.m1 - 1)) * c;  // dropped at the push / the store
    }
    const int cq = 4 * (tid & 7);
    float4 rx[kSimLoads], ry[kSimLoads];
    auto load = [&](int ch) {
#pragma unroll
        for (int u = 0; u < kSimLoads; ++u) {
            rx[u] = sim_load4(xrow[u], ch * kSimKC + cq, c, vec);
            ry[u] = sim_load4(yrow[u], ch * kSimKC + cq, c, vec);
        }
    };

    f32x16 acc[2][2];  // [target tile m][source tile n]
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[m][n][r] = 0.0f;

    const float *xa = Xs + (wc * 64 + lr) * kSimLd;
    const float *ya = Ys + (wr * 64 + lr) * kSimLd;
    const int nch = (c + kSimKC - 1) / kSimKC;
    load(0);
    for (int ch = 0; ch < nch; ++ch) {
#pragma unroll
        for (int u = 0; u < kSimLoads; ++u) {
            const int row = (tid + kSimThreads * u) >> 3;
            *reinterpret_cast<float4 *>(Xs + row * kSimLd + cq) = rx[u];
            *reinterpret_cast<float4 *>(Ys + row * kSimLd + cq) = ry[u];
        }
        __syncthreads();
        if (ch + 1 < nch) load(ch + 1);
#pragma unroll
        for (int t = 0; t < kSimKC / 4; ++t) {
            const float4 b0 = *reinterpret_cast<const float4 *>(xa + 4 * t);
            const float4 b1 = *reinterpret_cast<const float4 *>(xa + 32 * kSimLd + 4 * t);
            const float4 a0 = *reinterpret_cast<const float4 *>(ya + 4 * t);
            const float4 a1 = *reinterpret_cast<const float4 *>(ya + 32 * kSimLd + 4 * t);
            // k-step 2t: channels 4t (lanes 0-31) and 4t+1 (lanes 32-63); k-step 2t+1: 4t+2, 4t+3
            const float a0e = h ? a0.y : a0.x, a1e = h ? a1.y : a1.x;
            const float b0e = h ? b0.y : b0.x, b1e = h ? b1.y : b1.x;
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0e, b0e, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0e, b1e, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1e, b0e, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1e, b1e, acc[1][1], 0, 0, 0);
            const float a0o = h ? a0.w : a0.z, a1o = h ? a1.w : a1.z;
            const float b0o = h ? b0.w : b0.z, b1o = h ? b1.w : b1.z;
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0o, b0o, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0o, b1o, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1o, b0o, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1o, b1o, acc[1][1], 0, 0, 0);
        }
        __syncthreads();  // the chunk's readers are done: the next write pass (and the merge below) may go
    }

    // the lane's values, target index ascending: tile m, then register r
    // (row (r & 3) + 8 (r >> 2) + 4 h of the tile)
    u64 L[2][K];
#pragma unroll
    for (int n = 0; n < 2; ++n) {
#pragma unroll
        for (int t = 0; t < K; ++t) L[n][t] = 0;  // below every real key
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int j = t0 + wr * 64 + m * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                if (j < a.m1) list_push<K>(L[n], sim_key(acc[m][n][r], j));
            }
        // the other half-wave holds the tile's other 16 rows of the same source
        u64 O[K];
#pragma unroll
        for (int t = 0; t < K; ++t) O[t] = __shfl_xor(L[n][t], 32, 64);
#pragma unroll
        for (int t = 0; t < K; ++t) list_push<K>(L[n], O[t]);
    }
    // the waves wr = 1 hand their lists to the waves wr = 0: [wc][n][32][K]
    u64 *mk = reinterpret_cast<u64 *>(smem);
    if (wr == 1 && h == 0) {
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
            for (int t = 0; t < K; ++t) mk[((wc * 2 + n) * 32 + lr) * K + t] = L[n][t];
    }
    __syncthreads();
    if (wr == 0 && h == 0) {
#pragma unroll
        for (int n = 0; n < 2; ++n) {
#pragma unroll
            for (int t = 0; t < K; ++t) list_push<K>(L[n], mk[((wc * 2 + n) * 32 + lr) * K + t]);
            const int src = s0 + wc * 64 + n * 32 + lr;
            if (src < a.n1) {
                u64 *out = a.part + (((size_t)bat * a.n1 + src) * a.ntt + tt) * a.k;
#pragma unroll
                for (int t = 0; t < K; ++t)
                    if (t < a.k) out[t] = L[n][t];
            }
        }
    }
}

// one thread per source row: the target tiles' lists -> val, idx, the row's key
__global__ __launch_bounds__(256) void simtopk_merge(const u64 *part, long long rows, int n1, int ntt,
                                                     int k, float *val, int32_t *idx, u64 *rowkey) {
    const long long row = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= rows) return;
    u64 L[kMaxK];
#pragma unroll
    for (int t = 0; t < kMaxK; ++t) L[t] = 0;
    const u64 *p = part + (size_t)row * ntt * k;
    for (int e = 0; e < ntt * k; ++e) list_push<kMaxK>(L, p[e]);
    // k <= m1: the first k entries are real keys, their indices below m1
#pragma unroll
    for (int t = 0; t < kMaxK; ++t)
        if (t < k) {
            val[(size_t)row * k + t] = mono_value((unsigned)(L[t] >> 32));
            idx[(size_t)row * k + t] = (int32_t)~(unsigned)L[t];
        }
    const int i = (int)(row % n1);
    rowkey[row] = (L[0] & 0xffffffff00000000ull) | (unsigned)~i;
}

struct SelArgs {
    const u64 *rowkey;   // (b,n1)
    const float *val;    // (b,n1,k)
    const int32_t *idx;  // (b,n1,k)
    const float *tgt;    // (b,m1,3)
    int32_t *sel;        // (b,n_keep)
    float *w;            // (b,n_keep,k)
    float *corr;         // (b,n_keep,3)
    int32_t *idx_keep;   // (b,n_keep,k)
    int n1, m1, k, n_keep;
};

__global__ __launch_bounds__(kSelThreads) void tfmr_select(SelArgs a) {
    __shared__ u64 sk[kSelChunk];
    const int tid = threadIdx.x, bat = blockIdx.x;
    const int n1 = a.n1, k = a.k;
    const u64 *keys = a.rowkey + (size_t)bat * n1;
    for (int i0 = 0; i0 < n1; i0 += kSelThreads) {  // uniform: the barriers below
        const int i = i0 + tid;
        const u64 my = i < n1 ? keys[i] : ~0ull;
        int rank = 0;
        for (int c0 = 0; c0 < n1; c0 += kSelChunk) {
            const int len = min(kSelChunk, n1 - c0);
            __syncthreads();
            for (int e = tid; e < len; e += kSelThreads) sk[e] = keys[c0 + e];
            __syncthreads();
            for (int e = 0; e < len; ++e) rank += sk[e] > my ? 1 : 0;
        }
        if (i >= n1 || rank >= a.n_keep) continue;
        const size_t in = ((size_t)bat * n1 + i) * k, out = (size_t)bat * a.n_keep + rank;
        a.sel[out] = i;
        float v[kMaxK], wt[kMaxK];
        int j[kMaxK];
#pragma unroll
        for (int t = 0; t < kMaxK; ++t) {
            v[t] = t < k ? a.val[in + t] : 0.0f;
            const int jj = t < k ? a.idx[in + t] : 0;
            if (t < k) a.idx_keep[out * k + t] = jj;
            j[t] = (unsigned)jj < (unsigned)a.m1 ? jj : 0;  // never read outside tgt
        }
        float sum = v[0];
#pragma unroll
        for (int t = 1; t < kMaxK; ++t)
            if (t < k) sum = sum + v[t];
        const float den = sum + 1e-8f;
#pragma unroll
        for (int t = 0; t < kMaxK; ++t) {
            // f32 / f32 through f64 is the correctly rounded f32 quotient (53 >= 2 * 24 + 2)
            wt[t] = (float)((double)v[t] / (double)den);
            if (t < k) a.w[out * k + t] = wt[t];
        }
        const float *tg = a.tgt + (size_t)bat * a.m1 * 3;
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            float s = wt[0] * tg[(size_t)j[0] * 3 + d];
#pragma unroll
            for (int t = 1; t < kMaxK; ++t)
                if (t < k) s = s + wt[t] * tg[(size_t)j[t] * 3 + d];
            a.corr[out * 3 + d] = s;
        }
    }
}


constexpr int kMaxRows = 1 << 24;   // n1, m1
constexpr int kMaxC = 1 << 16;

// the sizes every entry shares; 0 when they are fine, else the message is set
int check_sizes(const char *who, int b, int n1, int m1, int c, int k) {
    PCR_REQUIRE(b >= 0, PCR_ERR_ARG, "%s: negative batch size", who);
    PCR_REQUIRE(n1 >= 1 && m1 >= 1, PCR_ERR_ARG, "%s: n1=%d, m1=%d (both must be >= 1)", who, n1, m1);
    PCR_REQUIRE(n1 <= kMaxRows && m1 <= kMaxRows, PCR_ERR_ARG, "%s: n1=%d or m1=%d too large (max %d)", who,
                n1, m1, kMaxRows);
    PCR_REQUIRE(c >= 1, PCR_ERR_ARG, "%s: c=%d (the feature width must be >= 1)", who, c);
    PCR_REQUIRE(c <= kMaxC, PCR_ERR_ARG, "%s: c=%d too wide (max %d)", who, c, kMaxC);
    PCR_REQUIRE(k >= 1 && k <= kMaxK, PCR_ERR_ARG, "%s: k=%d outside 1..%d", who, k, kMaxK);
    PCR_REQUIRE(k <= m1, PCR_ERR_ARG, "%s: k=%d exceeds m1=%d", who, k, m1);
    const long long blocks = (long long)b * cdiv64(n1, kSimTile) * cdiv64(m1, kSimTile);
    PCR_REQUIRE(blocks <= 0x7fffffffLL, PCR_ERR_ARG, "%s: b=%d x n1=%d x m1=%d too large", who, b, n1, m1);
    return PCR_OK;
}

// scratch: the target tiles' lists (b,n1,ntt,k) u64, then the row keys (b,n1) u64
long long part_words(int b, int n1, int m1, int k) { return (long long)b * n1 * cdiv64(m1, kSimTile) * k; }

int check_scratch(const char *who, const void *scratch) {
    PCR_REQUIRE(scratch, PCR_ERR_ARG, "%s: null scratch", who);
    PCR_REQUIRE(((uintptr_t)scratch & 255) == 0, PCR_ERR_ARG, "%s: scratch is not 256-byte aligned", who);
    return PCR_OK;
}

}  // namespace

extern "C" int64_t pcr_tfmr_scratch_bytes(int32_t b, int32_t n1, int32_t m1, int32_t c, int32_t k) {
    pcr::clear_error();
    if (check_sizes("tfmr_scratch_bytes", b, n1, m1, c, k) != PCR_OK) return -1;
    const long long words = part_words(b, n1, m1, k) + (long long)b * n1;
    return (words * 8 + 255) / 256 * 256;
}

extern "C" int pcr_similarity_topk(const float *fx, const float *fy, int32_t b, int32_t n1, int32_t m1,
                                   int32_t c, int32_t k, float *val, int32_t *idx, void *scratch,
                                   pcr_stream_t stream) {
    pcr::clear_error();
    int rc = check_sizes("similarity_topk", b, n1, m1, c, k);
    if (rc != PCR_OK) return rc;
    if (b == 0) return PCR_OK;
    PCR_REQUIRE(fx && fy && val && idx, PCR_ERR_ARG, "similarity_topk: null pointer");
    rc = check_scratch("similarity_topk", scratch);
    if (rc != PCR_OK) return rc;
    hipStream_t s = pcr::as_stream(stream);
    SimArgs a;
    a.fx = fx; a.fy = fy; a.part = (u64 *)scratch;
    a.n1 = n1; a.m1 = m1; a.c = c; a.k = k;
    a.nst = (int)cdiv64(n1, kSimTile); a.ntt = (int)cdiv64(m1, kSimTile);
    a.vec = (c % 4 == 0 && (((uintptr_t)fx | (uintptr_t)fy) & 15) == 0) ? 1 : 0;
    const dim3 grid((unsigned)((long long)b * a.nst * a.ntt));
    switch (k) {
        case 1: hipLaunchKernelGGL(simtopk_sweep<1>, grid, dim3(kSimThreads), 0, s, a); break;
        case 2: hipLaunchKernelGGL(simtopk_sweep<2>, grid, dim3(kSimThreads), 0, s, a); break;
        case 3: hipLaunchKernelGGL(simtopk_sweep<3>, grid, dim3(kSimThreads), 0, s, a); break;
        case 4: hipLaunchKernelGGL(simtopk_sweep<4>, grid, dim3(kSimThreads), 0, s, a); break;
        default: hipLaunchKernelGGL(simtopk_sweep<8>, grid, dim3(kSimThreads), 0, s, a); break;
    }
    PCR_LAUNCH_CHECK();
    const long long rows = (long long)b * n1;
    u64 *rowkey = a.part + part_words(b, n1, m1, k);
    hipLaunchKernelGGL(simtopk_merge, dim3((unsigned)cdiv64(rows, 256)), dim3(256), 0, s, a.part, rows, n1,
                       a.ntt, k, val, idx, rowkey);
    PCR_LAUNCH_CHECK();
    return PCR_OK;
}

extern "C" int pcr_tfmr_select(const float *val, const int32_t *idx, const float *tgt, int32_t b, int32_t n1,
                               int32_t m1, int32_t k, int32_t n_keep, int32_t *sel, float *w,
                               float *tgt_corr, int32_t *idx_keep, const void *scratch,
                               pcr_stream_t stream) {
    pcr::clear_error();
    int rc = check_sizes("tfmr_select", b, n1, m1, 1, k);
    if (rc != PCR_OK) return rc;
    PCR_REQUIRE(n_keep >= 0 && n_keep <= n1, PCR_ERR_ARG, "tfmr_select: n_keep=%d outside 0..n1=%d", n_keep,
                n1);
    if (b == 0 || n_keep == 0) return PCR_OK;
    PCR_REQUIRE(val && idx && tgt && sel && w && tgt_corr && idx_keep, PCR_ERR_ARG,
                "tfmr_select: null pointer");
    rc = check_scratch("tfmr_select", scratch);
    if (rc != PCR_OK) return rc;
    SelArgs a;
    a.rowkey = (const u64 *)scratch + part_words(b, n1, m1, k);
    a.val = val; a.idx = idx; a.tgt = tgt; a.sel = sel; a.w = w; a.corr = tgt_corr; a.idx_keep = idx_keep;
    a.n1 = n1; a.m1 = m1; a.k = k; a.n_keep = n_keep;
    hipLaunchKernelGGL(tfmr_select, dim3((unsigned)b), dim3(kSelThreads), 0, pcr::as_stream(stream), a);
    PCR_LAUNCH_CHECK();
    return PCR_OK;
}
