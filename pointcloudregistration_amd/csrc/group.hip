// Point-set sampling and grouping front end: farthest-point sampling, ball
// query and the point-pair-feature group of ROPNet's LocalFeatue / NgeNet's PPF.
//
// Reference: ROPNet/src/models/model_utils.py:6-102 (fps, ball_query,
// sample_and_group), TFMR.py:48-71 (LocalFeatue.forward);
// c2p-net/ngenet/utils/process.py:57-115, models/information_interactive.py:48-84.
//
// MI355X design (none of it follows the reference's tensor program, which
// forms a (B,N,N) distance matrix and sorts a (B,N,N) int64 index tensor):
//  * fps: one 1024-thread workgroup per cloud.  Every thread owns P points and
//    their running distances in registers (slot p of thread t is point
//    t + 1024 p); the cloud also sits in LDS so the current centre is one
//    broadcast read.  One step = P distance updates, one packed 64-bit max
//    (distance bits << 32 | ~index: distances are >= +0, so their bits order
//    like the values, and ~index makes the lowest index win a tie), reduced in
//    the wave (DPP row rotates, then two cross-row shuffles) and across the 16
//    waves through double-buffered LDS slots: one barrier per step.  Clouds
//    above 8192 points keep the first 8192 in registers and walk the rest
//    through global memory (coordinates re-read, distances in the workspace);
//    the key is the same, so both paths give identical results.
//  * ball query: one wave per query, the cloud staged through LDS as SoA
//    chunks.  The wave walks the indices 64 at a time; a ballot and a prefix
//    popcount append the neighbours in ascending order; a wave whose rows all
//    hold k neighbours stops scanning unless the counts are wanted.
//  * group_ppf: the ball query above with every point a centre, then one
//    element-wise kernel over (centre, neighbour) tiles.  channels_first
//    stores run along the centre axis (lane-consecutive); channels_last tiles
//    are staged in LDS and written out as contiguous rows.
// Numerics: d2 = (dx*dx + dy*dy) + dz*dz, each op rounded (built with
// -ffp-contract=off); neighbour iff !(d2 > r2).  Non-finite coordinates give
// unspecified results.
#include "pcr_internal.h"
#include "wave.h"
#include <math.h>

namespace {

using pcr::cdiv, pcr::d2_direct, pcr::u64;

constexpr int kFpsThreads = 1024;
constexpr int kFpsWaves = kFpsThreads / 64;
constexpr int kFpsRegPoints = 8 * kFpsThreads;  // 8192: the register path's capacity

__device__ __forceinline__ u64 fps_key(float d, int j) {
    return ((u64)__float_as_uint(d) << 32) | (unsigned)~j;
}

// max over the 16 lanes of a DPP row, left in every lane of the row
template <int kRor>
__device__ __forceinline__ u64 row_ror_max(u64 v) {
    const int lo = (int)(unsigned)v, hi = (int)(unsigned)(v >> 32);
    const unsigned olo = (unsigned)__builtin_amdgcn_update_dpp(lo, lo, 0x120 + kRor, 0xf, 0xf, false);
    const unsigned ohi = (unsigned)__builtin_amdgcn_update_dpp(hi, hi, 0x120 + kRor, 0xf, 0xf, false);
    const u64 o = ((u64)ohi << 32) | olo;
    return o > v ? o : v;
}

__device__ __forceinline__ u64 xor_max(u64 v, int mask) {
    const u64 o = __shfl_xor(v, mask, 64);
    return o > v ? o : v;
}

// max over the wave, left in every lane
__device__ __forceinline__ u64 wave_max(u64 v) {
    v = row_ror_max<8>(v);
    v = row_ror_max<4>(v);
    v = row_ror_max<2>(v);
    v = row_ror_max<1>(v);
    v = xor_max(v, 16);
    v = xor_max(v, 32);
    return v;
}

struct FpsArgs {
    const float *xyz;      // (b,n,3)
    const int32_t *start;  // (b)
    int32_t *idx;          // (b,m)
    float *over;           // (b, n - 8192) running distances of the overflow points, or null
    int n, m;
};

// P points per thread in registers; kOver: n > P * 1024 (P = 8), the cloud is
// not staged in LDS and points >= 8192 are walked through global memory
template <int P, bool kOver>
__global__ __launch_bounds__(kFpsThreads) void fps_kernel(FpsArgs a) {
    __shared__ float sxyz[kOver ? 3 : P * kFpsThreads * 3];
    __shared__ u64 slot[2][kFpsWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = a.n;
    const float *x = a.xyz + (size_t)blockIdx.x * n * 3;
    int32_t *out = a.idx + (size_t)blockIdx.x * a.m;
    float *over = kOver ? a.over + (size_t)blockIdx.x * (n - kFpsRegPoints) : nullptr;

    float px[P], py[P], pz[P], dist[P];
#pragma unroll
    for (int p = 0; p < P; ++p) {
        const int j = tid + p * kFpsThreads;
        const int jc = j < n ? j : n - 1;
        px[p] = x[jc * 3 + 0];
        py[p] = x[jc * 3 + 1];
        pz[p] = x[jc * 3 + 2];
        dist[p] = 1e10f;
    }
    if constexpr (kOver) {
        for (int j = kFpsRegPoints + tid; j < n; j += kFpsThreads) over[j - kFpsRegPoints] = 1e10f;
    } else {
        for (int e = tid; e < n * 3; e += kFpsThreads) sxyz[e] = x[e];
        __syncthreads();
    }

    int cur = a.start[blockIdx.x];
    cur = cur < 0 ? 0 : (cur >= n ? n - 1 : cur);  // precondition 0 <= start < n; never read outside
    for (int i = 0; i < a.m; ++i) {
        if (tid == 0) out[i] = cur;
        float cx, cy, cz;
        if constexpr (kOver) {
            cx = x[cur * 3 + 0]; cy = x[cur * 3 + 1]; cz = x[cur * 3 + 2];
        } else {
            cx = sxyz[cur * 3 + 0]; cy = sxyz[cur * 3 + 1]; cz = sxyz[cur * 3 + 2];
        }
        u64 best = 0;  // below every real key: a real key's low word ~j is > 0
#pragma unroll
        for (int p = 0; p < P; ++p) {
            const int j = tid + p * kFpsThreads;
            const float d = d2_direct(cx, cy, cz, px[p], py[p], pz[p]);
            dist[p] = d < dist[p] ? d : dist[p];
            const u64 k = j < n ? fps_key(dist[p], j) : 0;
            best = k > best ? k : best;
        }
        if constexpr (kOver) {
            for (int j = kFpsRegPoints + tid; j < n; j += kFpsThreads) {
                const float d = d2_direct(cx, cy, cz, x[j * 3 + 0], x[j * 3 + 1], x[j * 3 + 2]);
                const float o = over[j - kFpsRegPoints];
                const float v = d < o ? d : o;
                over[j - kFpsRegPoints] = v;
                const u64 k = fps_key(v, j);
                best = k > best ? k : best;
            }
        }
        best = wave_max(best);
        // slots alternate: a wave still reading step i's slots has not reached
        // step i+1's barrier, which every writer of step i+2 has passed
        if (lane == 0) slot[i & 1][wave] = best;
        __syncthreads();
        u64 v = slot[i & 1][lane & (kFpsWaves - 1)];
        v = row_ror_max<8>(v);
        v = row_ror_max<4>(v);
        v = row_ror_max<2>(v);
        v = row_ror_max<1>(v);
        cur = (int)~(unsigned)v;
    }
}

// ---------------------------------------------------------------------------
// ball query
// ---------------------------------------------------------------------------
constexpr int kBqThreads = 256;
constexpr int kBqWaves = kBqThreads / 64;
constexpr int kBqPerWave = 4;                         // queries per wave
constexpr int kBqPerBlock = kBqWaves * kBqPerWave;    // 16
constexpr int kBqChunk = 2048;                        // points per LDS stage (24 KiB)

struct BqArgs {
    const float *xyz;    // (b,n,3)
    const float *query;  // (b,q,3)
    int32_t *idx;        // (b,q,k)
    int32_t *count;      // (b,q) or null
    float r2;
    int n, q, k;
};

__global__ __launch_bounds__(kBqThreads) void ball_query_kernel(BqArgs a) {
    __shared__ float sx[kBqChunk], sy[kBqChunk], sz[kBqChunk];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int bat = blockIdx.y;
    const int n = a.n, k = a.k;
    const float *x = a.xyz + (size_t)bat * n * 3;
    const int q0 = blockIdx.x * kBqPerBlock + wave * kBqPerWave;
    const bool want_count = a.count != nullptr;

    float qx[kBqPerWave], qy[kBqPerWave], qz[kBqPerWave];
    int found[kBqPerWave], first[kBqPerWave];
#pragma unroll
    for (int u = 0; u < kBqPerWave; ++u) {
        const int qi = q0 + u < a.q ? q0 + u : a.q - 1;
        const float *qp = a.query + ((size_t)bat * a.q + qi) * 3;
        qx[u] = qp[0]; qy[u] = qp[1]; qz[u] = qp[2];
        found[u] = 0;
        first[u] = n;
    }
    const u64 lt_mask = ((u64)1 << lane) - 1;

    for (int c0 = 0; c0 < n; c0 += kBqChunk) {
        const int len = min(kBqChunk, n - c0);
        for (int e = tid; e < len * 3; e += kBqThreads) {
            const float v = x[(size_t)c0 * 3 + e];
            const int p = e / 3, c = e - 3 * p;
            (c == 0 ? sx : (c == 1 ? sy : sz))[p] = v;
        }
        __syncthreads();
        int active = 0;
#pragma unroll
        for (int u = 0; u < kBqPerWave; ++u) {
            if (q0 + u >= a.q) continue;  // wave-uniform
            int32_t *row = a.idx + ((size_t)bat * a.q + q0 + u) * k;
            for (int s = 0; s < len; s += 64) {
                if (!want_count && found[u] >= k) break;  // wave-uniform
                const int p = s + lane;
                bool in = false;
                if (p < len) in = !(d2_direct(qx[u], qy[u], qz[u], sx[p], sy[p], sz[p]) > a.r2);
                const u64 mask = __ballot(in);
                if (mask == 0) continue;
                const int pos = found[u] + __popcll(mask & lt_mask);
                if (in && pos < k) row[pos] = c0 + p;
                if (found[u] == 0) first[u] = c0 + s + __builtin_ctzll(mask);
                found[u] += __popcll(mask);
            }
            active |= want_count || found[u] < k;
        }
        // also the barrier between this chunk's readers and the next stage
        if (!__syncthreads_or(active)) break;
    }

#pragma unroll
    for (int u = 0; u < kBqPerWave; ++u) {
        if (q0 + u >= a.q) continue;
        const size_t r = (size_t)bat * a.q + q0 + u;
        int32_t *row = a.idx + r * k;
        // columns past the last neighbour repeat the first one; no neighbour: n
        for (int pos = min(found[u], k) + lane; pos < k; pos += 64) row[pos] = first[u];
        if (want_count && lane == 0) a.count[r] = found[u];
    }
}

// ---------------------------------------------------------------------------
// point-pair features of a group
// ---------------------------------------------------------------------------
constexpr int kPfThreads = 256;
constexpr int kPfTileI = 64;   // centres per tile
constexpr int kPfTileK = 16;   // neighbours per tile
constexpr int kPfElems = kPfTileI * kPfTileK / kPfThreads;  // 4 per thread

struct PpfArgs {
    const float *xyz;      // (b,n,3)
    const float *normals;  // (b,n,3) or null
    const int32_t *idx;    // (b,n,k)
    float *feat;
    int n, k;
};

// angle(a, b) = atan2f(|a x b|, a . b).  The dot's sum starts from +0 like the
// reference's reduction: three products of -0 (a zero vector against negative
// components, or a negative normal against a centre's own g = 0) then give +0
// and the angle 0, where a bare sum would give -0 and the angle pi.
__device__ __forceinline__ float angle3(const float a[3], const float b[3]) {
    const float c0 = a[1] * b[2] - a[2] * b[1];
    const float c1 = a[2] * b[0] - a[0] * b[2];
    const float c2 = a[0] * b[1] - a[1] * b[0];
    const float cn = sqrtf((c0 * c0 + c1 * c1) + c2 * c2);
    const float dt = ((0.0f + a[0] * b[0]) + a[1] * b[1]) + a[2] * b[2];
    return atan2f(cn, dt);
}

template <int C>
__device__ __forceinline__ void ppf_element(const PpfArgs &a, int bat, int i, int kk, float f[C]) {
    const int n = a.n;
    const float *x = a.xyz + (size_t)bat * n * 3;
    int j = a.idx[((size_t)bat * n + i) * a.k + kk];
    if ((unsigned)j >= (unsigned)n) j = i;  // never read outside (a centre is its own neighbour)
    float g[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float xi = x[i * 3 + c];
        f[c] = xi;
        g[c] = x[j * 3 + c] - xi;
        f[3 + c] = g[c];
    }
    if constexpr (C == 10) {
        const float *nr = a.normals + (size_t)bat * n * 3;
        const float ni[3] = {nr[i * 3 + 0], nr[i * 3 + 1], nr[i * 3 + 2]};
        const float nj[3] = {nr[j * 3 + 0], nr[j * 3 + 1], nr[j * 3 + 2]};
        f[6] = angle3(ni, g);
        f[7] = angle3(nj, g);
        f[8] = angle3(ni, nj);
        f[9] = sqrtf((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]);
    }
}

// feat (b,C,k,n): lanes run along the centre axis, every store is 64
// consecutive floats
template <int C>
__global__ __launch_bounds__(kPfThreads) void ppf_cf_kernel(PpfArgs a) {
    const int bat = blockIdx.z;
    const int i = blockIdx.x * kPfTileI + (threadIdx.x & (kPfTileI - 1));
    if (i >= a.n) return;
#pragma unroll
    for (int e = 0; e < kPfElems; ++e) {
        const int kk = blockIdx.y * kPfTileK + e * (kPfThreads / kPfTileI) + threadIdx.x / kPfTileI;
        if (kk >= a.k) continue;
        float f[C];
        ppf_element<C>(a, bat, i, kk, f);
#pragma unroll
        for (int c = 0; c < C; ++c)
            a.feat[(((size_t)bat * C + c) * a.k + kk) * a.n + i] = f[c];
    }
}

// feat (b,n,k,C): a centre's tile is kPfTileK * C consecutive floats; staged in
// LDS in output order, then copied out lane-consecutively
template <int C>
__global__ __launch_bounds__(kPfThreads) void ppf_cl_kernel(PpfArgs a) {
    __shared__ float sf[kPfTileI * kPfTileK * C];
    const int bat = blockIdx.z;
    const int i0 = blockIdx.x * kPfTileI, k0 = blockIdx.y * kPfTileK;
#pragma unroll
    for (int e = 0; e < kPfElems; ++e) {
        const int l = e * kPfThreads + threadIdx.x;
        const int i = i0 + l / kPfTileK, kk = k0 + l % kPfTileK;
        if (i >= a.n || kk >= a.k) continue;
        float f[C];
        ppf_element<C>(a, bat, i, kk, f);
#pragma unroll
        for (int c = 0; c < C; ++c) sf[l * C + c] = f[c];
    }
    __syncthreads();
    const int kw = min(kPfTileK, a.k - k0) * C;  // floats of this tile in one centre's row
    for (int t = threadIdx.x; t < kPfTileI * kPfTileK * C; t += kPfThreads) {
        const int il = t / (kPfTileK * C), r = t - il * (kPfTileK * C);
        if (i0 + il >= a.n || r >= kw) continue;
        a.feat[(((size_t)bat * a.n + i0 + il) * a.k + k0) * C + r] = sf[t];
    }
}


int launch_ball_query(const float *xyz, const float *query, int b, int n, int q, float r2, int k,
                      int32_t *idx, int32_t *count, hipStream_t s) {
    BqArgs a{xyz, query, idx, count, r2, n, q, k};
    hipLaunchKernelGGL(ball_query_kernel, dim3(cdiv(q, kBqPerBlock), b), dim3(kBqThreads), 0, s, a);
    PCR_LAUNCH_CHECK();
    return PCR_OK;
}

// the limit every entry shares: the kernels form point offsets 3 j in int
constexpr long long kMaxPoints = (1LL << 31) / 3 - 1;

}  // namespace

extern "C" int pcr_fps(const float *xyz, const int32_t *start, int32_t b, int32_t n, int32_t m,
                       int32_t *idx, pcr_stream_t stream) {
    pcr::clear_error();
    PCR_REQUIRE(b >= 0, PCR_ERR_ARG, "fps: negative batch size");
    PCR_REQUIRE(n >= 1 && m >= 1, PCR_ERR_ARG, "fps: n=%d, m=%d (both must be >= 1)", n, m);
    PCR_REQUIRE(n <= kMaxPoints, PCR_ERR_ARG, "fps: n=%d too large", n);
    if (b == 0) return PCR_OK;
    PCR_REQUIRE(xyz && start && idx, PCR_ERR_ARG, "fps: null pointer");
    hipStream_t s = pcr::as_stream(stream);
    FpsArgs a{xyz, start, idx, nullptr, n, m};
    if (n <= 2 * kFpsThreads) {
        hipLaunchKernelGGL((fps_kernel<2, false>), dim3(b), dim3(kFpsThreads), 0, s, a);
    } else if (n <= kFpsRegPoints) {
        hipLaunchKernelGGL((fps_kernel<8, false>), dim3(b), dim3(kFpsThreads), 0, s, a);
    } else {
        a.over = (float *)pcr::workspace(pcr::kWsFpsOver_PpfIdx, sizeof(float) * (size_t)b * (n - kFpsRegPoints));
        PCR_REQUIRE(a.over, PCR_ERR_NOMEM, "fps: %s", pcr_last_error());
        hipLaunchKernelGGL((fps_kernel<8, true>), dim3(b), dim3(kFpsThreads), 0, s, a);
    }
    PCR_LAUNCH_CHECK();
    return PCR_OK;
}

extern "C" int pcr_ball_query(const float *xyz, const float *query, int32_t b, int32_t n, int32_t q,
                              float r2, int32_t k, int32_t *idx, int32_t *count,
                              pcr_stream_t stream) {
    pcr::clear_error();
    PCR_REQUIRE(b >= 0 && q >= 0, PCR_ERR_ARG, "ball_query: negative size");
    PCR_REQUIRE(n >= 1 && k >= 1, PCR_ERR_ARG, "ball_query: n=%d, k=%d (both must be >= 1)", n, k);
    PCR_REQUIRE(n <= kMaxPoints, PCR_ERR_ARG, "ball_query: n=%d too large", n);
    PCR_REQUIRE(b <= 65535, PCR_ERR_ARG, "ball_query: b=%d too large (max 65535)", b);
    if (b == 0 || q == 0) return PCR_OK;
    PCR_REQUIRE(xyz && query && idx, PCR_ERR_ARG, "ball_query: null pointer");
    return launch_ball_query(xyz, query, b, n, q, r2, k, idx, count, pcr::as_stream(stream));
}

extern "C" int pcr_group_ppf(const float *xyz, const float *normals, int32_t b, int32_t n, float r2,
                             int32_t k, int32_t channels_first, float *feat, int32_t *idx,
                             pcr_stream_t stream) {
    pcr::clear_error();
    PCR_REQUIRE(b >= 0, PCR_ERR_ARG, "group_ppf: negative batch size");
    PCR_REQUIRE(n >= 1 && k >= 1, PCR_ERR_ARG, "group_ppf: n=%d, k=%d (both must be >= 1)", n, k);
    PCR_REQUIRE(n <= kMaxPoints, PCR_ERR_ARG, "group_ppf: n=%d too large", n);
    PCR_REQUIRE(b <= 65535 && cdiv(k, kPfTileK) <= 65535, PCR_ERR_ARG,
                "group_ppf: b=%d or k=%d too large", b, k);
    if (b == 0) return PCR_OK;
    PCR_REQUIRE(xyz && feat, PCR_ERR_ARG, "group_ppf: null pointer");
    hipStream_t s = pcr::as_stream(stream);
    if (!idx) {
        idx = (int32_t *)pcr::workspace(pcr::kWsFpsOver_PpfIdx, sizeof(int32_t) * (size_t)b * n * k);
        PCR_REQUIRE(idx, PCR_ERR_NOMEM, "group_ppf: %s", pcr_last_error());
    }
    const int rc = launch_ball_query(xyz, xyz, b, n, n, r2, k, idx, nullptr, s);
    if (rc != PCR_OK) return rc;
    PpfArgs a{xyz, normals, idx, feat, n, k};
    const dim3 grid(cdiv(n, kPfTileI), cdiv(k, kPfTileK), b);
    if (normals) {
        if (channels_first) hipLaunchKernelGGL(ppf_cf_kernel<10>, grid, dim3(kPfThreads), 0, s, a);
        else hipLaunchKernelGGL(ppf_cl_kernel<10>, grid, dim3(kPfThreads), 0, s, a);
    } else {
        if (channels_first) hipLaunchKernelGGL(ppf_cf_kernel<6>, grid, dim3(kPfThreads), 0, s, a);
        else hipLaunchKernelGGL(ppf_cl_kernel<6>, grid, dim3(kPfThreads), 0, s, a);
    }
    PCR_LAUNCH_CHECK();
    return PCR_OK;
}
