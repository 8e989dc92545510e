// k-nearest-neighbour graph and edge features of NgeNet's GCN.
//
// Reference: c2p-net/ngenet/models/information_interactive.py:7-23
// (get_graph_features), called twice per cloud by GCN.forward (:107-130).  The
// reference forms the (B,N,N) expanded-form distance matrix, runs
// topk(k + 1, largest=False, sorted=True) over it, drops column 0 and gathers
// [f_i, f_j - f_i] into (B,N,k,2C).
//
// MI355X design (no (b,n,n) array, no sort, no scratch):
//  * knn_graph: one wave per query, four queries per wave, the cloud staged
//    through LDS as SoA chunks like the ball query.  A wave keeps the running
//    kk + 1 best of a query sorted, one packed 64-bit key per lane (lane r holds
//    rank r; lanes past kk hold the maximum key): key = d2 bits << 32 | j.
//    Distances are >= +0, so their bits order like the values and the index in
//    the low word sends a tie to the lowest index.  Per 64 candidates: one key
//    per lane, a ballot of the keys below the wave's threshold (rank kk), and
//    for every set bit one insertion: the candidate's key is broadcast, the
//    lanes above its position take their lower neighbour's key (one DPP
//    wave_shr:1 per word).  All keys of a row are distinct, so the kk + 1
//    smallest are one set with one order whatever the chunking or the order of
//    insertion: the result cannot depend on either.  Rank 0 is dropped on the
//    way out.
//  * edge_features, channels_last (b,n,kk,2c): one wave per centre; lanes run
//    along the channels, so the reads of f_i / f_j and the stores of both
//    halves of a row are contiguous (16 bytes per lane when c is a multiple of
//    4 and the buffers are 16-byte aligned; the values are the same).  Four
//    neighbour rows are loaded before the first of their stores.
//  * edge_features, channels_first (b,2c,n,kk): a workgroup takes 64 consecutive
//    (i, rank) pairs and 64 channels; the rows f_i and f_j are read
//    row-contiguously (four rows in flight per wave) into two LDS tiles (row
//    stride 65 words: conflict-free both ways) and stored transposed, lanes
//    along the flattened (i, rank) axis.
// Numerics: d2 = (dx*dx + dy*dy) + dz*dz, each op rounded (built with
// -ffp-contract=off); f_j - f_i is one f32 subtraction.  Non-finite
// coordinates give unspecified results.
#include "pcr_internal.h"
#include "wave.h"

namespace {

using pcr::cdiv64, pcr::d2_direct, pcr::u64;

constexpr int kKnThreads = 256;
constexpr int kKnWaves = kKnThreads / 64;
constexpr int kKnPerWave = 4;                        // queries per wave
constexpr int kKnPerBlock = kKnWaves * kKnPerWave;   // 16
constexpr int kKnChunk = 2048;                       // points per LDS stage (24 KiB)
constexpr int kKnMaxK = 63;                          // kk + 1 keys fit one wave
constexpr u64 kKnNoKey = ~(u64)0;                    // above every real key

__device__ __forceinline__ u64 knn_key(float d, int j) {
    return ((u64)__float_as_uint(d) << 32) | (unsigned)j;
}

// lane `l` (wave-uniform) of v, left in every lane
__device__ __forceinline__ u64 lane_bcast(u64 v, int l) {
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, l);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), l);
    return ((u64)hi << 32) | lo;
}

// lane l takes lane l - 1's value; lane 0 keeps its own (DPP wave_shr:1)
__device__ __forceinline__ u64 wave_shift_up(u64 v) {
    const int lo = (int)(unsigned)v, hi = (int)(unsigned)(v >> 32);
    const unsigned olo = (unsigned)__builtin_amdgcn_update_dpp(lo, lo, 0x138, 0xf, 0xf, false);
    const unsigned ohi = (unsigned)__builtin_amdgcn_update_dpp(hi, hi, 0x138, 0xf, 0xf, false);
    return ((u64)ohi << 32) | olo;
}

struct KnnArgs {
    const float *xyz;  // (b,n,3)
    int32_t *idx;      // (b,n,kk)
    float *d2;         // (b,n,kk) or null
    int n, kk;
};

__global__ __launch_bounds__(kKnThreads) void knn_graph_kernel(KnnArgs a) {
    __shared__ float sx[kKnChunk], sy[kKnChunk], sz[kKnChunk];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int bat = blockIdx.y;
    const int n = a.n, kk = a.kk;
    const float *x = a.xyz + (size_t)bat * n * 3;
    const int q0 = blockIdx.x * kKnPerBlock + wave * kKnPerWave;

    float qx[kKnPerWave], qy[kKnPerWave], qz[kKnPerWave];
    u64 best[kKnPerWave], cut[kKnPerWave];
#pragma unroll
    for (int u = 0; u < kKnPerWave; ++u) {
        const int qi = q0 + u < n ? q0 + u : n - 1;
        qx[u] = x[qi * 3 + 0]; qy[u] = x[qi * 3 + 1]; qz[u] = x[qi * 3 + 2];
        best[u] = kKnNoKey;
        cut[u] = kKnNoKey;
    }

    for (int c0 = 0; c0 < n; c0 += kKnChunk) {
        const int len = min(kKnChunk, n - c0);
        if (c0) __syncthreads();  // the previous chunk's readers are done
        for (int e = tid; e < len * 3; e += kKnThreads) {
            const float v = x[(size_t)c0 * 3 + e];
            const int p = e / 3, c = e - 3 * p;
            (c == 0 ? sx : (c == 1 ? sy : sz))[p] = v;
        }
        __syncthreads();
        for (int s = 0; s < len; s += 64) {
            const int p = s + lane;
            const bool have = p < len;
            const int pc = have ? p : len - 1;
            const float px = sx[pc], py = sy[pc], pz = sz[pc];
#pragma unroll
            for (int u = 0; u < kKnPerWave; ++u) {
                if (q0 + u >= n) continue;  // wave-uniform
                const u64 key = have ? knn_key(d2_direct(qx[u], qy[u], qz[u], px, py, pz), c0 + p)
                                     : kKnNoKey;
                u64 mask = __ballot(key < cut[u]);
                while (mask) {
                    const int src = __builtin_ctzll(mask);
                    mask &= mask - 1;
                    const u64 cand = lane_bcast(key, src);
                    if (!(cand < cut[u])) continue;  // the threshold moved below it
                    // sorted lanes: the number of keys below cand is its rank
                    const int pos = __popcll(__ballot(best[u] < cand));
                    const u64 up = wave_shift_up(best[u]);
                    best[u] = lane < pos ? best[u] : (lane == pos ? cand : up);
                    cut[u] = lane_bcast(best[u], kk);
                }
            }
        }
    }

    // n >= kk + 1, so ranks 0 .. kk are real keys; rank 0 is dropped
#pragma unroll
    for (int u = 0; u < kKnPerWave; ++u) {
        if (q0 + u >= n) continue;
        if (lane >= 1 && lane <= kk) {
            const size_t at = ((size_t)bat * n + q0 + u) * kk + (lane - 1);
            a.idx[at] = (int32_t)(unsigned)best[u];
            if (a.d2) a.d2[at] = __uint_as_float((unsigned)(best[u] >> 32));
        }
    }
}

// ---------------------------------------------------------------------------
// edge features
// ---------------------------------------------------------------------------
struct EdgeArgs {
    const float *feats;  // (b,n,c)
    const int32_t *idx;  // (b,n,kk)
    float *out;
    int n, c, kk;
};

// precondition 0 <= j < n; never read outside the cloud
__device__ __forceinline__ int clamp_index(int j, int n) { return j < 0 ? 0 : (j >= n ? n - 1 : j); }

constexpr int kEfThreads = 256;
constexpr int kEfWaves = kEfThreads / 64;

constexpr int kEfBatch = 4;  // neighbour rows in flight per lane

// out (b,n,kk,2c): one wave per centre, V floats per lane
template <int V>
__global__ __launch_bounds__(kEfThreads) void edge_cl_kernel(EdgeArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long i = (long long)blockIdx.x * kEfWaves + wave;
    if (i >= a.n) return;  // no barrier below
    const int n = a.n, c = a.c, kk = a.kk;
    const size_t row = (size_t)blockIdx.y * n + i;
    const float *__restrict__ f = a.feats + (size_t)blockIdx.y * n * c;
    const int32_t *__restrict__ nb = a.idx + row * kk;
    float *__restrict__ o = a.out + row * kk * 2 * c;
    for (int ch = lane * V; ch < c; ch += 64 * V) {
        float fi[V];
        if constexpr (V == 4) *(float4 *)fi = *(const float4 *)(f + (size_t)i * c + ch);
        else fi[0] = f[(size_t)i * c + ch];
        // kEfBatch rows' loads are issued before the first of their stores
        for (int r0 = 0; r0 < kk; r0 += kEfBatch) {
            float fj[kEfBatch][V];
#pragma unroll
            for (int u = 0; u < kEfBatch; ++u) {
                const int j = clamp_index(nb[min(r0 + u, kk - 1)], n);
                if constexpr (V == 4) *(float4 *)fj[u] = *(const float4 *)(f + (size_t)j * c + ch);
                else fj[u][0] = f[(size_t)j * c + ch];
            }
#pragma unroll
            for (int u = 0; u < kEfBatch; ++u) {
                if (r0 + u >= kk) break;
                float *orow = o + (size_t)(r0 + u) * 2 * c;
                if constexpr (V == 4) {
                    *(float4 *)(orow + ch) = *(const float4 *)fi;
                    *(float4 *)(orow + c + ch) = make_float4(fj[u][0] - fi[0], fj[u][1] - fi[1],
                                                             fj[u][2] - fi[2], fj[u][3] - fi[3]);
                } else {
                    orow[ch] = fi[0];
                    orow[c + ch] = fj[u][0] - fi[0];
                }
            }
        }
    }
}

constexpr int kEfTile = 64;  // (i, rank) pairs and channels per workgroup

// out (b,2c,n,kk): lanes run along t = i * kk + rank
__global__ __launch_bounds__(kEfThreads) void edge_cf_kernel(EdgeArgs a) {
    __shared__ float si[kEfTile][kEfTile + 1], sj[kEfTile][kEfTile + 1];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int n = a.n, c = a.c, kk = a.kk;
    const long long total = (long long)n * kk;
    const long long t0 = (long long)blockIdx.x * kEfTile;
    const int ch0 = blockIdx.y * kEfTile;
    const float *__restrict__ f = a.feats + (size_t)blockIdx.z * n * c;
    const int32_t *__restrict__ nb = a.idx + (size_t)blockIdx.z * total;
    const int nch = min(kEfTile, c - ch0);
    const int rows = (int)min((long long)kEfTile, total - t0);  // >= 1

    // lane l holds pair t0 + l (the tile's last pair past the end): centre, neighbour
    const int i0 = (int)(t0 / kk), r0 = (int)(t0 - (long long)i0 * kk);
    const int ll = min(lane, rows - 1);
    const int il = i0 + (r0 + ll) / kk;
    const int jl = clamp_index(nb[t0 + ll], n);
    const int chl = ch0 + min(lane, nch - 1);
    // a wave's rows are wave, wave + 4, ...: kEfBatch rows' loads in flight
#pragma unroll
    for (int q0 = 0; q0 < kEfTile / kEfWaves; q0 += kEfBatch) {
        float vi[kEfBatch], vj[kEfBatch];
#pragma unroll
        for (int u = 0; u < kEfBatch; ++u) {
            const int tl = min(wave + (q0 + u) * kEfWaves, rows - 1);  // wave-uniform
            const int i = __builtin_amdgcn_readlane(il, tl), j = __builtin_amdgcn_readlane(jl, tl);
            vi[u] = f[(size_t)i * c + chl];
            vj[u] = f[(size_t)j * c + chl];
        }
#pragma unroll
        for (int u = 0; u < kEfBatch; ++u) {
            const int tl = wave + (q0 + u) * kEfWaves;
            if (tl < rows && lane < nch) {
                si[tl][lane] = vi[u];
                sj[tl][lane] = vj[u];
            }
        }
    }
    __syncthreads();
    const long long t = t0 + lane;
    if (t >= total) return;
    float *__restrict__ o = a.out + (size_t)blockIdx.z * 2 * c * total;
    for (int cl = wave; cl < nch; cl += kEfWaves) {
        const float fi = si[lane][cl];
        o[(size_t)(ch0 + cl) * total + t] = fi;
        o[(size_t)(c + ch0 + cl) * total + t] = sj[lane][cl] - fi;
    }
}


// the limit the grouping entries share: the kernels form point offsets 3 j in int
constexpr long long kMaxPoints = (1LL << 31) / 3 - 1;

}  // namespace

extern "C" int pcr_knn_graph(const float *xyz, int32_t b, int32_t n, int32_t k, int32_t *idx,
                             float *d2, pcr_stream_t stream) {
    pcr::clear_error();
    PCR_REQUIRE(b >= 0, PCR_ERR_ARG, "knn_graph: negative batch size");
    PCR_REQUIRE(n >= 1, PCR_ERR_ARG, "knn_graph: n=%d (must be >= 1)", n);
    PCR_REQUIRE(k >= 1 && k <= kKnMaxK, PCR_ERR_ARG, "knn_graph: k=%d outside 1..%d", k, kKnMaxK);
    PCR_REQUIRE(n <= kMaxPoints, PCR_ERR_ARG, "knn_graph: n=%d too large", n);
    PCR_REQUIRE(b <= 65535, PCR_ERR_ARG, "knn_graph: b=%d too large (max 65535)", b);
    const int kk = k < n - 1 ? k : n - 1;
    if (b == 0 || kk == 0) return PCR_OK;
    PCR_REQUIRE(xyz && idx, PCR_ERR_ARG, "knn_graph: null pointer");
    KnnArgs a{xyz, idx, d2, n, kk};
    hipLaunchKernelGGL(knn_graph_kernel, dim3((unsigned)cdiv64(n, kKnPerBlock), b), dim3(kKnThreads), 0,
                       pcr::as_stream(stream), a);
    PCR_LAUNCH_CHECK();
    return PCR_OK;
}

extern "C" int pcr_edge_features(const float *feats, const int32_t *idx, int32_t b, int32_t n,
                                 int32_t c, int32_t kk, int32_t channels_first, float *out,
                                 pcr_stream_t stream) {
    pcr::clear_error();
    PCR_REQUIRE(b >= 0, PCR_ERR_ARG, "edge_features: negative batch size");
    PCR_REQUIRE(n >= 1 && c >= 1, PCR_ERR_ARG, "edge_features: n=%d, c=%d (both must be >= 1)", n, c);
    PCR_REQUIRE(kk >= 0 && kk <= kKnMaxK, PCR_ERR_ARG, "edge_features: kk=%d outside 0..%d", kk, kKnMaxK);
    PCR_REQUIRE(n <= kMaxPoints, PCR_ERR_ARG, "edge_features: n=%d too large", n);
    PCR_REQUIRE(b <= 65535 && cdiv64(c, kEfTile) <= 65535, PCR_ERR_ARG,
                "edge_features: b=%d or c=%d too large", b, c);
    if (b == 0 || kk == 0) return PCR_OK;
    PCR_REQUIRE(feats && idx && out, PCR_ERR_ARG, "edge_features: null pointer");
    hipStream_t s = pcr::as_stream(stream);
    EdgeArgs a{feats, idx, out, n, c, kk};
    if (channels_first) {
        const dim3 grid((unsigned)cdiv64((long long)n * kk, kEfTile), (unsigned)cdiv64(c, kEfTile), b);
        hipLaunchKernelGGL(edge_cf_kernel, grid, dim3(kEfThreads), 0, s, a);
    } else {
        const dim3 grid((unsigned)cdiv64(n, kEfWaves), b);
        const bool wide = c % 4 == 0 && (((uintptr_t)feats | (uintptr_t)out) & 15) == 0;
        if (wide) hipLaunchKernelGGL(edge_cl_kernel<4>, grid, dim3(kEfThreads), 0, s, a);
        else hipLaunchKernelGGL(edge_cl_kernel<1>, grid, dim3(kEfThreads), 0, s, a);
    }
    PCR_LAUNCH_CHECK();
    return PCR_OK;
}
