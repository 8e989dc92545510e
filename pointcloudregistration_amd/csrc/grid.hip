// Batched hashed-grid construction over target clouds (one launch per stage
// for all P pairs).  See grid.h for the layout and query semantics.
#include "pcr_internal.h"
#include "grid.h"
#include "scan.h"
#include <cstdlib>
#include <cstring>
#include <vector>

namespace pcr {
namespace {

struct BuildArgs {
    const float *tgt;
    const int32_t *n_tgt;
    int Mmax, S;
    double cell;
    int *cnt;      // P*S
    int *start;    // P*(S+1)
    float4 *pts;   // P*Mmax: x, y, z, index bits (one 16-B store per point)
};

__global__ void grid_count(BuildArgs a) {
    const int p = blockIdx.y;
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= count_of(a.n_tgt, p, a.Mmax)) return;
    const float *q = a.tgt + ((size_t)p * a.Mmax + j) * 3;
    const unsigned h = cell_hash(cell_coord((double)q[0], a.cell), cell_coord((double)q[1], a.cell),
                                 cell_coord((double)q[2], a.cell), a.S);
    atomicAdd(a.cnt + (size_t)p * a.S + h, 1);
}

__global__ __launch_bounds__(1024) void grid_scan(BuildArgs a) {
    const int p = blockIdx.x;
    block_exclusive_scan_1024(a.cnt + (size_t)p * a.S, a.start + (size_t)p * (a.S + 1), a.S, true);
}

__global__ void grid_scatter(BuildArgs a) {
    const int p = blockIdx.y;
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= count_of(a.n_tgt, p, a.Mmax)) return;
    const float *q = a.tgt + ((size_t)p * a.Mmax + j) * 3;
    const unsigned h = cell_hash(cell_coord((double)q[0], a.cell), cell_coord((double)q[1], a.cell),
                                 cell_coord((double)q[2], a.cell), a.S);
    const int pos = a.start[(size_t)p * (a.S + 1) + h] + atomicAdd(a.cnt + (size_t)p * a.S + h, 1);
    a.pts[(size_t)p * a.Mmax + pos] = make_float4(q[0], q[1], q[2], __int_as_float(j));
}

// count, scan and scatter of one pair's grid in one workgroup, the slot
// counters in LDS (S <= kLdsSlots): the per-point atomics stay on the CU
// (the global count / scatter passes took ~0.19 ms per grid per C4 step).
// Points land in a cell in atomic order, as before: every query takes the
// lexicographic (d2, j) minimum, so the order within a cell changes no result.
constexpr int kLdsSlots = 32768;

__global__ __launch_bounds__(1024) void grid_build_lds(BuildArgs a) {
    extern __shared__ int cnt[];  // S + 1: counts -> exclusive starts -> cursors
    const int p = blockIdx.x, S = a.S;
    const int m = count_of(a.n_tgt, p, a.Mmax);
    const float *q = a.tgt + (size_t)p * a.Mmax * 3;
    for (int i = threadIdx.x; i < S; i += 1024) cnt[i] = 0;
    __syncthreads();
    for (int j = threadIdx.x; j < m; j += 1024)
        atomicAdd(&cnt[cell_hash(cell_coord((double)q[3 * j], a.cell), cell_coord((double)q[3 * j + 1], a.cell),
                                 cell_coord((double)q[3 * j + 2], a.cell), S)],
                  1);
    __syncthreads();
    block_exclusive_scan_1024(cnt, cnt, S, false);
    int *st = a.start + (size_t)p * (S + 1);
    for (int i = threadIdx.x; i <= S; i += 1024) st[i] = cnt[i];
    __syncthreads();
    for (int j = threadIdx.x; j < m; j += 1024) {
        const float x = q[3 * j], y = q[3 * j + 1], z = q[3 * j + 2];
        const unsigned h = cell_hash(cell_coord((double)x, a.cell), cell_coord((double)y, a.cell),
                                     cell_coord((double)z, a.cell), S);
        a.pts[(size_t)p * a.Mmax + atomicAdd(&cnt[h], 1)] = make_float4(x, y, z, __int_as_float(j));
    }
}

// One workgroup per cloud chooses the layout and builds it (grid.h, grid_dense.h).
//
// Dense: the bounding box in cells of d.dcell, then -- when it has at most
// kDenseCellCap cells -- a counting sort by linear cell id with one u16 counter
// per cell, two to an LDS word (counts and cursors stay below 2^15, so a half
// never carries into its neighbour).  One thread per 32-cell bitmap word turns
// its 16 counter words into the word's bits, point count and occupied count;
// a block scan of the packed (points << 16 | occupied) sums gives each word
// its rank and first point offset; a second walk writes bits, rank and the
// occupied cells' offsets to the pair's table area and leaves each cell's
// cursor in its counter; the scatter writes the points.  If the tables do not
// fit tab_bytes (or the cloud is too large), the hashed grid of grid_build_lds
// is built instead, in the same LDS.  hdr[p] records the choice.
struct DenseArgs {
    double dcell;
    GridHdr *hdr;
    char *tab;
    int tab_bytes;
};

constexpr int kAutoLdsInts = kDenseCellCap / 2 + kDenseWordCap + 1;
static_assert(kAutoLdsInts >= kLdsSlots + 1, "the hashed fallback's slot counters share the dense build's LDS");

__device__ __forceinline__ void word_summary(const int *cnt, int w, int nw32, unsigned &bits, int &npts) {
    bits = 0u;
    npts = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const int i = 16 * w + k;
        const unsigned v = i < nw32 ? (unsigned)cnt[i] : 0u;
        const unsigned c0 = v & 0xffffu, c1 = v >> 16;
        bits |= (c0 ? 1u : 0u) << (2 * k) | (c1 ? 1u : 0u) << (2 * k + 1);
        npts += (int)(c0 + c1);
    }
}

__global__ __launch_bounds__(1024) void grid_build_auto(BuildArgs a, DenseArgs d) {
    extern __shared__ int cnt[];  // dense: cells / 2 packed counters, then words + 1 sums; hashed: S + 1
    __shared__ int smin[3][16], smax[3][16];
    const int p = blockIdx.x, t = threadIdx.x, S = a.S;
    const int m = count_of(a.n_tgt, p, a.Mmax);
    const float *q = a.tgt + (size_t)p * a.Mmax * 3;
    float4 *pts = a.pts + (size_t)p * a.Mmax;
    GridHdr h{};
    uint32_t *tbits = (uint32_t *)(d.tab + (size_t)p * d.tab_bytes);
    if (m == 0) {  // an empty cloud is trivially dense: one empty bitmap word
        if (t == 0) {
            tbits[0] = 0u;
            tbits[1] = 0u;  // rank[0], start[0]
            h.mode = 1;
            h.words = 1;
            d.hdr[p] = h;
        }
        int *st = a.start + (size_t)p * (S + 1);
        for (int i = t; i <= S; i += 1024) st[i] = 0;
        return;
    }
    auto cellq = [&](int j, int c) {
        const double v = __builtin_floor((double)q[3 * j + c] / d.dcell);
        // (NaN and out-of-range coordinates land beyond kDenseMaxCoord: not dense)
        return v >= -2147483000.0 && v <= 2147483000.0 ? (int)v : 0x7fffffff;
    };
    int mn[3] = {0x7fffffff, 0x7fffffff, 0x7fffffff}, mx[3] = {-0x7fffffff, -0x7fffffff, -0x7fffffff};
    for (int j = t; j < m; j += 1024)
        for (int c = 0; c < 3; ++c) {
            const int v = cellq(j, c);
            mn[c] = min(mn[c], v);
            mx[c] = max(mx[c], v);
        }
    for (int c = 0; c < 3; ++c) {
        for (int off = 32; off; off >>= 1) {
            mn[c] = min(mn[c], __shfl_xor(mn[c], off, 64));
            mx[c] = max(mx[c], __shfl_xor(mx[c], off, 64));
        }
        if ((t & 63) == 0) { smin[c][t >> 6] = mn[c]; smax[c][t >> 6] = mx[c]; }
    }
    __syncthreads();
    int o[3], D[3];
    bool dense = m <= kDenseMaxPoints;
    for (int c = 0; c < 3; ++c) {
        int lo = smin[c][0], hi = smax[c][0];
        for (int w = 1; w < 16; ++w) { lo = min(lo, smin[c][w]); hi = max(hi, smax[c][w]); }
        dense = dense && lo > -kDenseMaxCoord && hi < kDenseMaxCoord;
        o[c] = lo;
        D[c] = dense ? hi - lo + 1 : 0;
    }
    const int cells = dense ? dense_cells(D[0], D[1], D[2]) : -1;
    const int words = (cells + 31) >> 5;
    dense = cells > 0 && dense_table_bytes(words, 1) <= (size_t)d.tab_bytes;
    if (dense) {
        const int nw32 = (cells + 1) >> 1;
        int *wsum = cnt + kDenseCellCap / 2;
        auto id_of = [&](int j) {
            return dense_id(cellq(j, 0) - o[0], cellq(j, 1) - o[1], cellq(j, 2) - o[2], D[0], D[1]);
        };
        for (int i = t; i < nw32; i += 1024) cnt[i] = 0;
        __syncthreads();
        for (int j = t; j < m; j += 1024) {
            const int id = id_of(j);
            atomicAdd(&cnt[id >> 1], 1 << ((id & 1) * 16));
        }
        __syncthreads();
        for (int w = t; w < words; w += 1024) {
            unsigned bits;
            int npts;
            word_summary(cnt, w, nw32, bits, npts);
            wsum[w] = (npts << 16) | __popc(bits);
        }
        __syncthreads();
        block_exclusive_scan_1024(wsum, wsum, words, false);
        const int occ = wsum[words] & 0xffff;
        dense = dense_table_bytes(words, occ) <= (size_t)d.tab_bytes;
        if (dense) {
            uint16_t *trank = (uint16_t *)(tbits + words), *tstart = trank + words;
            for (int w = t; w < words; w += 1024) {
                unsigned bits;
                int npts;
                word_summary(cnt, w, nw32, bits, npts);
                int rk = wsum[w] & 0xffff, ps = (int)((unsigned)wsum[w] >> 16);
                tbits[w] = bits;
                trank[w] = (uint16_t)rk;
#pragma unroll 1
                for (int k = 0; k < 16; ++k) {
                    const int i = 16 * w + k;
                    if (i >= nw32) break;
                    const unsigned v = (unsigned)cnt[i];
                    const int c0 = (int)(v & 0xffffu), c1 = (int)(v >> 16);
                    if (c0) tstart[rk++] = (uint16_t)ps;
                    const unsigned cur0 = (unsigned)ps;
                    ps += c0;
                    if (c1) tstart[rk++] = (uint16_t)ps;
                    cnt[i] = (int)(cur0 | ((unsigned)ps << 16));  // counts -> cursors
                    ps += c1;
                }
            }
            if (t == 0) {
                tstart[occ] = (uint16_t)m;
                h.mode = 1;
                h.ox = o[0]; h.oy = o[1]; h.oz = o[2];
                h.DX = D[0]; h.DY = D[1]; h.DZ = D[2];
                h.occ = occ;
                h.words = words;
                d.hdr[p] = h;
            }
            __syncthreads();
            for (int j = t; j < m; j += 1024) {
                const int id = id_of(j), sh = (id & 1) * 16;
                const int pos = (int)(((unsigned)atomicAdd(&cnt[id >> 1], 1 << sh) >> sh) & 0xffffu);
                pts[pos] = make_float4(q[3 * j], q[3 * j + 1], q[3 * j + 2], __int_as_float(j));
            }
            return;
        }
        __syncthreads();  // wsum was read by all before the counters are reused
    }
    // hashed (grid_build_lds)
    if (t == 0) d.hdr[p] = h;  // mode 0
    for (int i = t; i < S; i += 1024) cnt[i] = 0;
    __syncthreads();
    for (int j = t; j < m; j += 1024)
        atomicAdd(&cnt[cell_hash(cell_coord((double)q[3 * j], a.cell), cell_coord((double)q[3 * j + 1], a.cell),
                                 cell_coord((double)q[3 * j + 2], a.cell), S)],
                  1);
    __syncthreads();
    block_exclusive_scan_1024(cnt, cnt, S, false);
    int *st = a.start + (size_t)p * (S + 1);
    for (int i = t; i <= S; i += 1024) st[i] = cnt[i];
    __syncthreads();
    for (int j = t; j < m; j += 1024) {
        const float x = q[3 * j], y = q[3 * j + 1], z = q[3 * j + 2];
        const unsigned hs = cell_hash(cell_coord((double)x, a.cell), cell_coord((double)y, a.cell),
                                      cell_coord((double)z, a.cell), S);
        pts[atomicAdd(&cnt[hs], 1)] = make_float4(x, y, z, __int_as_float(j));
    }
}

// Spatial order of a cloud: points bucketed by the Morton code of their grid
// cell, 5 bits per axis relative to the cloud's minimum cell (cells merged in
// powers of two until the cloud's extent fits 32), by a counting sort in LDS --
// one 1024-thread workgroup per cloud: count, scan, scatter (the bitonic sort
// of full 30-bit codes it replaces took 128 us per C4 call).  Sweeps that walk
// a cloud in this order give each wave neighbouring queries: the same hash
// cells, similar candidate counts, coherent LDS reads.  Order within a bucket is
// atomic order; it changes timing only (every sweep's result is independent of
// the order: fixed-point or integer sums, per-point outputs, and an early stop
// that only fires on hypotheses that cannot win).
__device__ __forceinline__ unsigned spread10(unsigned v) {
    v &= 1023u;
    v = (v | (v << 16)) & 0x030000FFu;
    v = (v | (v << 8)) & 0x0300F00Fu;
    v = (v | (v << 4)) & 0x030C30C3u;
    v = (v | (v << 2)) & 0x09249249u;
    return v;
}

constexpr int kOrdBits = 5, kOrdBuckets = 1 << (3 * kOrdBits);

__global__ __launch_bounds__(1024) void spatial_order_kernel(const float *pts, const int32_t *n, int Nmax,
                                                             double inv_cell, int32_t *order, float *perm) {
    extern __shared__ int bk[];  // kOrdBuckets + 1: counts -> starts -> cursors
    __shared__ int smin[3][16], smax[3][16];
    constexpr int kReg = 8;      // points per thread whose cell coordinates stay in registers
    const int p = blockIdx.x, t = threadIdx.x;
    const int m = count_of(n, p, Nmax);
    const float *P = pts + (size_t)p * Nmax * 3;
    int32_t *o = order + (size_t)p * Nmax;
    float *pm = perm ? perm + (size_t)p * Nmax * 3 : nullptr;
    auto put = [&](int pos, int i) {
        o[pos] = i;
        if (pm) { pm[3 * pos] = P[3 * i]; pm[3 * pos + 1] = P[3 * i + 1]; pm[3 * pos + 2] = P[3 * i + 2]; }
    };
    auto cellq = [&](int i, int c) { return (int)__builtin_floor((double)P[3 * i + c] * inv_cell); };
    int qr[kReg][3];
    int mn[3] = {0x7fffffff, 0x7fffffff, 0x7fffffff}, mx[3] = {-0x7fffffff, -0x7fffffff, -0x7fffffff};
#pragma unroll
    for (int u = 0; u < kReg; ++u) {
        const int i = t + 1024 * u;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            qr[u][c] = i < m ? cellq(i, c) : 0;
            if (i < m) { mn[c] = min(mn[c], qr[u][c]); mx[c] = max(mx[c], qr[u][c]); }
        }
    }
    for (int i = t + 1024 * kReg; i < m; i += 1024)
        for (int c = 0; c < 3; ++c) {
            const int q = cellq(i, c);
            mn[c] = min(mn[c], q);
            mx[c] = max(mx[c], q);
        }
    for (int c = 0; c < 3; ++c) {
        for (int off = 32; off; off >>= 1) {
            mn[c] = min(mn[c], __shfl_xor(mn[c], off, 64));
            mx[c] = max(mx[c], __shfl_xor(mx[c], off, 64));
        }
        if ((t & 63) == 0) { smin[c][t >> 6] = mn[c]; smax[c][t >> 6] = mx[c]; }
    }
    for (int i = t; i < kOrdBuckets; i += 1024) bk[i] = 0;
    __syncthreads();
    int base[3], ext = 0;
    for (int c = 0; c < 3; ++c) {
        int lo = smin[c][0], hi = smax[c][0];
        for (int w = 1; w < 16; ++w) { lo = min(lo, smin[c][w]); hi = max(hi, smax[c][w]); }
        base[c] = lo;
        ext = max(ext, (int)min((long long)hi - lo, (long long)0x3fffffff));
    }
    int shift = 0;
    while ((ext >> shift) >= (1 << kOrdBits)) ++shift;
    auto key_of = [&](const int (&q)[3]) -> unsigned {
        unsigned k = 0;
        for (int c = 0; c < 3; ++c) {
            const int v = (q[c] - base[c]) >> shift;
            k |= spread10((unsigned)min(max(v, 0), (1 << kOrdBits) - 1)) << c;
        }
        return k;
    };
    auto key = [&](int i) -> unsigned {
        const int q[3] = {cellq(i, 0), cellq(i, 1), cellq(i, 2)};
        return key_of(q);
    };
    unsigned kr[kReg];
#pragma unroll
    for (int u = 0; u < kReg; ++u) {
        kr[u] = key_of(qr[u]);
        if (t + 1024 * u < m) atomicAdd(&bk[kr[u]], 1);
    }
    for (int i = t + 1024 * kReg; i < m; i += 1024) atomicAdd(&bk[key(i)], 1);
    __syncthreads();
    block_exclusive_scan_1024(bk, bk, kOrdBuckets, false);
#pragma unroll
    for (int u = 0; u < kReg; ++u) {
        const int i = t + 1024 * u;
        if (i < m) put(atomicAdd(&bk[kr[u]], 1), i);
    }
    for (int i = t + 1024 * kReg; i < m; i += 1024) put(atomicAdd(&bk[key(i)], 1), i);
    for (int i = m + t; i < Nmax; i += 1024) o[i] = i;
}

}  // namespace

int spatial_order(const float *pts, const int32_t *n, int P, int Nmax, double cell, hipStream_t s,
                  WsSlot ws_slot, const int32_t **order, const float **perm, WsSlot perm_slot) {
    int32_t *o = (int32_t *)workspace(ws_slot, sizeof(int32_t) * (size_t)P * Nmax + 64);
    PCR_REQUIRE(o, PCR_ERR_NOMEM, "spatial_order: %s", pcr_last_error());
    float *pm = nullptr;
    if (perm) {
        pm = (float *)workspace(perm_slot, sizeof(float) * 3 * (size_t)P * Nmax + 64);
        PCR_REQUIRE(pm, PCR_ERR_NOMEM, "spatial_order: %s", pcr_last_error());
    }
    const size_t sm = sizeof(int) * (size_t)(kOrdBuckets + 1);
    PCR_HIP_CHECK(hipFuncSetAttribute((const void *)spatial_order_kernel,
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)sm));
    hipLaunchKernelGGL(spatial_order_kernel, dim3(P), dim3(1024), sm, s, pts, n, Nmax, 1.0 / cell, o, pm);
    PCR_LAUNCH_CHECK();
    *order = o;
    if (perm) *perm = pm;
    return PCR_OK;
}

int build_grids(const float *tgt, const int32_t *n_tgt, int P, int Mmax, double r, hipStream_t s,
                WsSlot ws_slot, GridBatch &out, double cell_factor, int slot_num) {
    int S = 256;
    while (S < Mmax) S <<= 1;
    S = S / 2 * slot_num;
    const size_t cnt_b = sizeof(int) * (size_t)P * S;
    BuildArgs a;
    WsLayout l;
    l.take(a.cnt, (size_t)P * S);
    l.take(a.start, (size_t)P * (S + 1));
    l.take(a.pts, (size_t)P * (Mmax > 0 ? Mmax : 1));  // 16-byte aligned
    PCR_REQUIRE(workspace_bind(ws_slot, l, kWsSlack), PCR_ERR_NOMEM, "grid workspace: %s", pcr_last_error());
    a.tgt = tgt;
    a.n_tgt = n_tgt;
    a.Mmax = Mmax;
    a.S = S;
    a.cell = cell_factor * r;
    if (S <= kLdsSlots) {
        PCR_HIP_CHECK(hipFuncSetAttribute((const void *)grid_build_lds, hipFuncAttributeMaxDynamicSharedMemorySize,
                                          (int)(sizeof(int) * (kLdsSlots + 1))));
        hipLaunchKernelGGL(grid_build_lds, dim3(P), dim3(1024), sizeof(int) * (size_t)(S + 1), s, a);
        PCR_LAUNCH_CHECK();
    } else {
        PCR_HIP_CHECK(hipMemsetAsync(a.cnt, 0, cnt_b, s));
        const dim3 g((Mmax + 255) / 256 > 0 ? (Mmax + 255) / 256 : 1, P);
        hipLaunchKernelGGL(grid_count, g, dim3(256), 0, s, a);
        PCR_LAUNCH_CHECK();
        hipLaunchKernelGGL(grid_scan, dim3(P), dim3(1024), 0, s, a);
        PCR_LAUNCH_CHECK();
        hipLaunchKernelGGL(grid_scatter, g, dim3(256), 0, s, a);
        PCR_LAUNCH_CHECK();
    }
    out.pts = a.pts;
    out.start = (uint32_t *)a.start;
    out.S = S;
    out.mstride = Mmax;
    out.cell = a.cell;
    return PCR_OK;
}

int build_grids_auto(const float *tgt, const int32_t *n_tgt, int P, int Mmax, double r, hipStream_t s,
                     WsSlot ws_slot, GridBatch &out, int tab_bytes, int slot_num) {
    const int S = grid_slots(Mmax, slot_num);
    PCR_REQUIRE(S <= kLdsSlots && tab_bytes >= 16 && tab_bytes % 16 == 0, PCR_ERR_ARG,
                "grid: auto layout with %d slots, %d table bytes", S, tab_bytes);
    BuildArgs a;
    DenseArgs d;
    WsLayout l;
    l.take(a.start, (size_t)P * (S + 1));
    l.take(a.pts, (size_t)P * (Mmax > 0 ? Mmax : 1));  // 16-byte aligned
    l.take(d.hdr, P);
    l.take(d.tab, (size_t)P * tab_bytes, 16);
    PCR_REQUIRE(workspace_bind(ws_slot, l, kWsSlack), PCR_ERR_NOMEM, "grid workspace: %s", pcr_last_error());
    a.tgt = tgt;
    a.n_tgt = n_tgt;
    a.Mmax = Mmax;
    a.S = S;
    a.cell = 2.01 * r;
    a.cnt = nullptr;
    d.dcell = kDenseCellFactor * r;
    d.tab_bytes = tab_bytes;
    const size_t sm = sizeof(int) * (size_t)kAutoLdsInts;
    PCR_HIP_CHECK(hipFuncSetAttribute((const void *)grid_build_auto, hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)sm));
    hipLaunchKernelGGL(grid_build_auto, dim3(P), dim3(1024), sm, s, a, d);
    PCR_LAUNCH_CHECK();
    out.pts = a.pts;
    out.start = (uint32_t *)a.start;
    out.S = S;
    out.mstride = Mmax;
    out.cell = a.cell;
    out.hdr = d.hdr;
    out.tab = d.tab;
    out.tab_bytes = tab_bytes;
    out.dcell = d.dcell;
    return PCR_OK;
}

int require_all_dense(const GridBatch &g, int P, hipStream_t s, const char *who) {
    PCR_REQUIRE(g.hdr, PCR_ERR_ARG, "%s: the dense grid layout was asked for but cannot be built for these sizes", who);
    std::vector<GridHdr> h((size_t)P);
    PCR_HIP_CHECK(hipMemcpyAsync(h.data(), g.hdr, sizeof(GridHdr) * (size_t)P, hipMemcpyDeviceToHost, s));
    PCR_HIP_CHECK(hipStreamSynchronize(s));
    for (int p = 0; p < P; ++p)
        PCR_REQUIRE(h[p].mode == 1, PCR_ERR_ARG, "%s: pair %d does not fit the dense grid layout", who, p);
    return PCR_OK;
}

namespace {
__global__ void radius_nn_kernel(GridBatch g, const double *q, const int32_t *n_q, int Qmax,
                                 double r, double thr, int32_t *idx, double *d2o) {
    const int p = blockIdx.y;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= Qmax) return;
    const int nq = n_q ? min(max(n_q[p], 0), Qmax) : Qmax;
    int j = -1;
    double d2 = __builtin_inf();
    if (i < nq) {
        const double *x = q + ((size_t)p * Qmax + i) * 3;
        if (g.dense(p)) j = grid_query_dense<2>(g.dense_view(p), r, thr, x[0], x[1], x[2], d2);
        else j = grid_query(g.view(p), r, thr, x[0], x[1], x[2], d2);
    }
    idx[(size_t)p * Qmax + i] = j;
    if (d2o) d2o[(size_t)p * Qmax + i] = d2;
}
}  // namespace

}  // namespace pcr

extern "C" int pcr_radius_nn(const float *tgt_xyz, int32_t P, int32_t Mmax, const int32_t *n_tgt,
                             const double *queries, int32_t Qmax, const int32_t *n_q, double r,
                             int32_t *idx, double *d2, pcr_stream_t stream) {
    pcr::clear_error();
    PCR_REQUIRE(P >= 0 && Mmax >= 0 && Qmax >= 0, PCR_ERR_ARG, "radius_nn: negative size");
    if (P == 0 || Qmax == 0) return PCR_OK;
    PCR_REQUIRE(tgt_xyz && queries && idx, PCR_ERR_ARG, "radius_nn: null pointer");
    PCR_REQUIRE(r > 0.0, PCR_ERR_ARG, "radius_nn: r must be > 0");
    PCR_REQUIRE(P <= 65535, PCR_ERR_ARG, "radius_nn: P=%d > 65535", P);
    hipStream_t s = pcr::as_stream(stream);
    // PCR_RADIUS_NN_GRID=dense|auto (test hook; default hash): the dense r-cell
    // layout of grid.h, built per pair and queried from HBM, with the table area
    // an 8192-point RANSAC sweep has
    const char *ge = getenv("PCR_RADIUS_NN_GRID");
    const bool want_dense = ge && !strcmp(ge, "dense"), want_auto = ge && !strcmp(ge, "auto");
    PCR_REQUIRE(!ge || !*ge || want_dense || want_auto || !strcmp(ge, "hash"), PCR_ERR_ARG,
                "radius_nn: PCR_RADIUS_NN_GRID=%s (hash, dense or auto)", ge);
    pcr::GridBatch g{};
    int rc;
    const bool can = Mmax <= pcr::kDenseMaxPoints && pcr::grid_slots(Mmax, 2) <= 32768;
    const pcr::WsSlot slot = pcr::kWsIcpPartials_RadiusNnGrid;
    if ((want_dense || want_auto) && can) rc = pcr::build_grids_auto(tgt_xyz, n_tgt, P, Mmax, r, s, slot, g, 32 * 1024, 2);
    else rc = pcr::build_grids(tgt_xyz, n_tgt, P, Mmax, r, s, slot, g);
    if (rc != PCR_OK) return rc;
    if (want_dense) {
        rc = pcr::require_all_dense(g, P, s, "radius_nn");
        if (rc != PCR_OK) return rc;
    }
    hipLaunchKernelGGL(pcr::radius_nn_kernel, dim3((Qmax + 255) / 256, P), dim3(256), 0, s, g,
                       queries, n_q, Qmax, r, pcr::radius_thr(r), idx, d2);
    PCR_LAUNCH_CHECK();
    return PCR_OK;
}
